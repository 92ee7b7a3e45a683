"""CPU: RNN's fixture, Python surface and C ABI surface (no device needed).

The restatement of tests/rnn_cases.py is tied to the reference's own module through tests/golden/rnn_golden.npz,
and the conditions the GPU bounds rest on are asserted here.
"""
import ctypes as C
import io
import os
import pickletools
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import abd_amd
from abd_amd import _lib as L, training as T
from abd_amd.models_rnn import RNN, PARAM_ORDER, tile_info
import rnn_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "rnn_golden.npz"))


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_restatement_reproduces_the_reference(name):
    """The reference's forward casts to float32, so its results are float32: the float32 restatement (the same
    torch primitives) reproduces them to rounding, the float64 one within the float32 margin of 1e-5."""
    for dtype, tol in ((torch.float32, 2e-6), (torch.float64, 1e-5)):
        r = rc.run_case(name, dtype, states=False)
        assert rc.rel_err(r["logits"], GOLD[f"{name}/logits"]) < tol
        g = float(GOLD[f"{name}/loss"])
        assert abs(float(r["loss"]) - g) <= tol * abs(g)
        for n in ("fc.weight", "fc.bias"):
            assert rc.rel_err(r["grads"][n], GOLD[f"{name}/grad/{n}"]) < tol, n
        for n in rc.LSTM_GRADS:
            stats, sample = rc.digest(r["grads"][n].numpy())
            want = GOLD[f"{name}/gradstats/{n}"]
            scale = float(want[1])   # the L2 norm bounds what rounding can move the sum by
            assert abs(stats[1] - want[1]) <= tol * scale, n
            assert abs(stats[0] - want[0]) <= tol * scale * np.sqrt(r["grads"][n].numel()), n
            assert rc.rel_err(sample, GOLD[f"{name}/gradsample/{n}"]) < tol or scale == 0.0, n


def test_golden_file_is_small_and_outputs_only():
    assert os.path.getsize(os.path.join(HERE, "golden", "rnn_golden.npz")) < 1 << 20
    kinds = {k.split("/")[1] for k in GOLD.files}
    assert kinds == {"logits", "loss", "grad", "gradstats", "gradsample"}
    assert all(GOLD[k].size <= rc.SAMPLE_MAX for k in GOLD.files if "/gradsample/" in k)


@pytest.mark.parametrize("name", list(rc.CASES))
def test_fixture_float32_margin_and_logit_gaps(name):
    """float32 on the CPU stays within 1e-5 of float64 (a 10x margin under the device's 1e-4 bound) -- or, where
    rc.BOUNDS records a measured device bound, within a tenth of it -- and every row's top-2 logit gap exceeds
    1e-3 of the largest logit (predictions must match exactly)."""
    B, Tn, Fd, K, _ = rc.CASES[name]
    a, b = rc.run_case(name, torch.float64), rc.run_case(name, torch.float32, states=False)
    assert a["logits"].shape == (B, K)
    assert rc.rel_err(b["logits"], a["logits"]) < 1e-5
    if K > 1:
        top = a["logits"].topk(2, dim=1).values
        assert float(((top[:, 0] - top[:, 1]) / a["logits"].abs().max()).min()) > 1e-3
    for n in rc.PARAM_ORDER:
        assert rc.rel_err(b["grads"][n], a["grads"][n]) < 0.1 * rc.bound(name, n), n
    if name == "one_class":
        assert float(a["loss"]) == 0.0 and all(float(g.abs().max()) == 0.0 for g in a["grads"].values())
    if name == "one_step":
        assert all(float(a["grads"][f"lstm.weight_hh_l{k}"].abs().max()) == 0.0 for k in range(rc.LAYERS))
    # the unrolled stack (saved h / c / gates oracle) is the library LSTM
    m = a["_model"]
    with torch.no_grad():
        x = torch.tensor(rc.make_inputs(name)[0], dtype=torch.float64).squeeze(1)
        z = x.new_zeros((rc.LAYERS, B, rc.H))
        out, _ = m.lstm(x, (z, z))
    assert rc.rel_err(a["states"][-1][0], out) < 1e-12
    # a dropped bias would move the logits far past the bound
    st = rc.make_state(name)
    st["lstm.bias_hh_l1"] = np.zeros_like(st["lstm.bias_hh_l1"])
    with torch.no_grad():
        moved = rc.Restated(st)(torch.tensor(rc.make_inputs(name)[0], dtype=torch.float64))
    assert rc.rel_err(moved, a["logits"]) > 1e-2


def test_case_sizes_follow_the_kernels_thresholds():
    B, Tn = rc.CASES["big_batch"][:2]
    assert B * Tn > rc.COLSUM_ROWS >= (B - 1) * Tn and (B * Tn) // rc.SLICE_ROWS == 2 > ((B - 1) * Tn) // rc.SLICE_ROWS
    large = -(-B * Tn // rc.LARGE_TILE) * (4 * rc.H // rc.LARGE_TILE)
    assert large >= rc.LARGE_MIN_BLOCKS and (B * Tn) % rc.LARGE_TILE
    B, Tn = rc.CASES["ragged_tiles"][:2]
    assert B == 2 * rc.REC_ROWS + 1 and (B * Tn) % rc.SMALL_TILE
    assert rc.CASES["wide"][3] > rc.SMALL_TILE and rc.CASES["tiny"][0] < rc.REC_ROWS
    lib = abd_amd.load_library()
    assert [lib.abd_rnn_tile_info(i) for i in range(7)] == [rc.REC_ROWS, rc.SMALL_TILE, rc.LARGE_TILE, rc.SLICE_ROWS,
                                                            rc.COLSUM_ROWS, rc.LARGE_MIN_BLOCKS, -1]
    assert tile_info("rec_rows") == rc.REC_ROWS


@pytest.mark.parametrize("geo", rc.DIGEST_MODELS)
def test_seeded_init_and_state_dict_match_a_plain_build(geo):
    """utils/models.py:231-257 builds nn.LSTM(time_len, 768, 3, batch_first=True) then nn.Linear(768, classes):
    the same construction order consumes torch's generator alike."""
    K, Fd = geo
    torch.manual_seed(rc.DIGEST_SEED)
    m = RNN(K, Fd)
    torch.manual_seed(rc.DIGEST_SEED)
    lstm = nn.LSTM(Fd, 768, 3, batch_first=True)
    fc = nn.Linear(768, K)
    sd = m.state_dict()
    want = {**{f"lstm.{k}": v for k, v in lstm.state_dict().items()}, **{f"fc.{k}": v for k, v in fc.state_dict().items()}}
    assert list(sd) == list(want) == list(PARAM_ORDER) == list(rc.PARAM_ORDER)
    assert [n for n, _ in m.named_parameters()] == list(PARAM_ORDER)
    for k in sd:
        assert sd[k].shape == want[k].shape == rc.param_shapes(Fd, K)[k] and torch.equal(sd[k], want[k]), k
    assert (m.hidden_size, m.num_layers) == (768, 3)
    assert isinstance(m.lstm, nn.LSTM) and m.lstm.batch_first and not m.lstm.bidirectional
    assert isinstance(m.fc, nn.Linear)


def test_header_symbols_are_exported():
    with open(os.path.join(ROOT, "include", "abd.h")) as f:
        names = sorted(set(re.findall(r"\b(abd_rnn_\w+)\s*\(", f.read())))
    assert len(names) == 11, names
    for n in ("abd_rnn_create", "abd_rnn_destroy", "abd_rnn_param_count", "abd_rnn_param_offsets",
              "abd_rnn_workspace_bytes", "abd_rnn_workspace_offset", "abd_rnn_forward", "abd_rnn_backward",
              "abd_rnn_train_step", "abd_rnn_eval"):
        assert n in names
    lib = abd_amd.load_library()
    for n in names:
        assert hasattr(lib, n), n
        assert n in L.EXPORTS, n
    assert C.sizeof(L.RnnArgs) == 120   # abd_rnn_args on LP64


def test_create_limits_offsets_and_workspace_names():
    lib = abd_amd.load_library()
    h = C.c_void_p()
    for geo in ((32, 129, 10), (0, 13, 10), (1025, 13, 10), (32, 0, 10), (32, 13, 0), (32, 13, 4097)):
        assert lib.abd_rnn_create(*geo, C.byref(h)) == 1002, geo
    for geo in ((1, 13, 10), (1024, 13, 10), (32, 1, 10), (32, 128, 10), (32, 13, 1), (32, 13, 4096)):   # the limits
        assert lib.abd_rnn_create(*geo, C.byref(h)) == 0, geo
        lib.abd_rnn_destroy(h)
    assert lib.abd_rnn_create(100, 40, 10, C.byref(h)) == 0
    offs = (C.c_int64 * 15)()
    assert lib.abd_rnn_param_offsets(h, offs) == 0
    sizes = [int(np.prod(s)) for s in rc.param_shapes(40, 10).values()]
    assert list(offs) == [0] + list(np.cumsum(sizes))
    assert lib.abd_rnn_param_count(h) == sum(sizes) == sum(p.numel() for p in RNN(10, 40).parameters())
    names = [f"{k}{i}" for k in ("h", "c", "gates") for i in (1, 2, 3)] + ["logits", "dlogits", "rowinfo"]
    got = [lib.abd_rnn_workspace_offset(h, 4, n.encode()) for n in names]
    assert all(o >= 0 for o in got) and len(set(got)) == len(got)
    assert lib.abd_rnn_workspace_offset(h, 4, b"nope") == -1
    # the documented size: h, c, gates of three layers and one (B*T, 768) gradient buffer dominate
    need = lib.abd_rnn_workspace_bytes(h, 256)
    assert 4 * 256 * 100 * (3 * (768 + 768 + 3072) + 768) <= need < 1.7e9
    a = L.RnnArgs()
    a.x = a.params = a.grads = 16   # never dereferenced: the calls return before any launch
    a.batch = 2
    assert lib.abd_rnn_train_step(h, C.byref(a), None, 0, None) == 1001 and b"labels" in lib.abd_last_error()
    a.labels = 16
    assert lib.abd_rnn_train_step(h, C.byref(a), None, 0, None) == 1003
    assert lib.abd_rnn_forward(h, C.byref(a), None, 0, None) == 1003
    lib.abd_rnn_destroy(h)


def test_dropin_resolves_rnn_without_the_reference_module():
    code = ("import sys; from utils.models import RNN, smallcnn, lstmwithattention; import utils.models as um; "
            "print(RNN.__module__, 'utils._reference_models' in sys.modules, "
            "sorted(set(um._OTHERS)) == ['ResNet', 'ResidualBlock', 'largecnn', 'smalllstm'])")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "audio-backdoor-attack_amd", "dropin"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=HERE)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["abd_amd.models_rnn", "False", "True"]


def test_training_accepts_the_model():
    m = RNN(10, 13)
    assert RNN in T.ACCELERATED
    assert T.fusable(m, torch.optim.Adam(m.parameters()), nn.CrossEntropyLoss())
    assert not T.fusable(m, torch.optim.Adam(m.parameters(), weight_decay=0.1), nn.CrossEntropyLoss())
    assert not T.fusable(m, torch.optim.SGD(m.parameters(), lr=0.1), nn.CrossEntropyLoss())
    with pytest.raises(L.AbdError):   # SGD
        T.train(m, [], "cpu", torch.optim.SGD(m.parameters(), lr=0.1), nn.CrossEntropyLoss())
    with pytest.raises(L.AbdError):
        T.clean_train(m, [], "cpu", torch.optim.SGD(m.parameters(), lr=0.1), nn.CrossEntropyLoss())


def test_cpu_tensors_and_bf16_are_refused():
    m = RNN(10, 13)
    with pytest.raises(L.AbdError):
        m(torch.zeros(2, 1, 8, 13))
    with pytest.raises(L.AbdError):
        m.eval()(torch.zeros(2, 1, 8, 13, dtype=torch.float64))
    with pytest.raises(L.AbdError):
        T.rnn_train_step(m, torch.zeros(2, 1, 8, 13), torch.zeros(2, dtype=torch.int64), None, None, None)
    with pytest.raises(ValueError):
        m(torch.zeros(2, 8, 13))
    with pytest.raises(L.AbdError):
        m.set_gemm_precision("bf16")
    with pytest.raises(ValueError):
        m.set_gemm_precision("fp8")
    assert m.set_gemm_precision("f32") is m


class _FakeDevice(torch.Tensor):
    """A CPU tensor that claims to live on the device: gets past require_device, so the refusal under test
    is the one that fires (nothing is launched before it)."""
    is_cuda = True


def test_geometry_mismatch_raises():
    m = RNN(10, 13)
    with pytest.raises(ValueError):
        m(torch.zeros((2, 1, 8, 14)).as_subclass(_FakeDevice))


def test_smallcnn_only_paths_refuse_the_model():
    """Data parallelism / SyncBN (ResidentTrainer, training.train_step), SGD fine-tuning and every defence entry
    point refuse RNN with AbdError -- also once an engine is bound, when the flat buffers exist."""
    from abd_amd import defense as D, pipeline as P

    class Eng:   # what a bound engine looks like to the duck-typed smallcnn paths
        device = torch.device("cpu")
        params = torch.zeros(4)
        running = torch.zeros(22)

    for bound in (False, True):
        m = RNN(10, 13)
        if bound:
            m._engine = Eng()
            m._bound = lambda eng: True
        opt = torch.optim.Adam(m.parameters())
        x = torch.zeros((4, 1, 8, 13)).as_subclass(_FakeDevice)
        y = torch.zeros(4, dtype=torch.int64).as_subclass(_FakeDevice)
        calls = {
            "train_step": lambda: T.train_step(m, x, y, None, None, None, mask1=x, mask2=x),
            "ResidentTrainer": lambda: P.ResidentTrainer(None, None, None, m, opt, 4),
            "SgdBinding": lambda: T.SgdBinding(m, torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)),
            "check_sgd": lambda: T.check_sgd(m, torch.optim.SGD(m.parameters(), lr=0.1)),
            "flat_state": lambda: D._flat_state(m, torch.device("cpu")),
            "ablation_sweep": lambda: D.ablation_sweep(m, x, y, torch.zeros((1, 160), dtype=torch.uint8)),
            "neuron_loss_change": lambda: D.neuron_loss_change(m, x, y),
            "hidden_activation": lambda: D.hidden_activation(m, x),
            "fc_prune_sweep": lambda: D.fc_prune_sweep(m, x, y, torch.zeros((1, 128), dtype=torch.uint8)),
            "neuron_names": lambda: D.neuron_names(m),
            "param_offsets": lambda: D.param_offsets(m),
            "row_table": lambda: D.row_table(m),
            "neuron_weight_change": lambda: D.neuron_weight_change(m, torch.zeros(4)),
            "absdiff_rows": lambda: D.absdiff_rows(m, torch.zeros(4)),
            "reinit_selection": lambda: D.reinit_selection(m, [("conv1.weight", 0, 1.0)], [0.1], 0.7),
            "reinit_models": lambda: D.reinit_models(m, [("conv1.weight", 0, 1.0)], torch.zeros(4), [0.1], 0.7),
            "model_with_params": lambda: D.model_with_params(m, torch.zeros(4)),
            "final_gradients": lambda: D.final_gradients(m),
            "finetune_epoch": lambda: D.finetune_epoch(m, x, y, torch.optim.SGD(m.parameters(), lr=0.1)),
            "finetune_reg_epoch": lambda: D.finetune_reg_epoch(m, x, y, torch.optim.SGD(m.parameters(), lr=0.1),
                                                               0.1, 0.5),
            "unlearn_epoch": lambda: D.unlearn_epoch(m, x, y, opt),
            "unlearn_run": lambda: D.unlearn_run(m, x, y, opt, 1),
            "pruned_finetune_epoch": lambda: D.pruned_finetune_epoch(m, x, y, opt, torch.zeros(128)),
            "adam_binding": lambda: D._adam_binding(m, opt, "unlearn_epoch"),
        }
        for what, call in calls.items():
            with pytest.raises(L.AbdError):
                call()
                pytest.fail(f"{what} (bound={bound}) did not refuse RNN")


def test_flowmur_and_daba_refuse_the_model():
    """FlowMur's trigger optimisation (its input gradient) and pretrain_model are smallcnn's; DABA's per-utterance
    forward is too."""
    from abd_amd import daba, flowmur
    m = RNN(10, 13)
    with pytest.raises(L.AbdError):
        flowmur._as_abd_smallcnn(m)
    with pytest.raises(L.AbdError):
        flowmur.TriggerOptimizer(m.eval(), 4000)
    for fn in (daba.one_sotamax_entropy,):
        with pytest.raises(L.AbdError):
            fn("RNN", m, "nowhere.wav")
    with pytest.raises(L.AbdError):
        daba._require_cnn("RNN", m)


def test_checkpoint_is_a_reference_pickle(tmp_path):
    torch.manual_seed(3)
    m = RNN(10, 13)
    p = tmp_path / "ckpt.pt"
    T.save_reference_checkpoint(m, str(p))
    import zipfile
    with zipfile.ZipFile(p) as z:
        data = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    ops = [(o.name, a) for o, a, _ in pickletools.genops(io.BytesIO(data))]
    assert "utils.models RNN" in [a for n, a in ops if n == "GLOBAL"]
    assert not any("abd_amd" in str(a) for _, a in ops if a is not None)
    state = T.reference_module_state(m)
    plain = nn.Module()
    plain.__dict__.update(state)
    assert list(plain.state_dict().keys()) == list(m.state_dict().keys())
    for k, v in m.state_dict().items():
        assert torch.equal(plain.state_dict()[k], v), k
    assert isinstance(plain.lstm, nn.LSTM) and isinstance(plain.fc, nn.Linear)
    # the attributes the reference's forward reads
    assert (state["hidden_size"], state["num_layers"], state["device"]) == (768, 3, torch.device("cpu"))
    assert "_engine" not in state and "gemm_precision" not in state


def test_getstate_drops_the_engine():
    m = RNN(10, 13)
    m._engine = object()
    st = m.__getstate__()
    assert st["_engine"] is None
    n = RNN.__new__(RNN)
    n.__setstate__({k: v for k, v in st.items() if k not in ("_engine", "gemm_precision", "hidden_size")})
    assert n._engine is None and n.gemm_precision == "f32" and n.hidden_size == 768
