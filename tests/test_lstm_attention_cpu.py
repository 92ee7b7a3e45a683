"""CPU: lstmwithattention's fixture, Python surface and C ABI surface (no device needed).

The float64 restatement of tests/lstm_attention_cases.py is tied to the reference's own module through
tests/golden/lstm_attention_golden.npz, and the conditions the GPU bounds rest on are asserted here.
"""
import ctypes as C
import io
import os
import pickletools
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import abd_amd
from abd_amd import _lib as L, training as T
from abd_amd.models_lstm import lstmwithattention, PARAM_ORDER
import lstm_attention_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "lstm_attention_golden.npz"))
CASES = list(lc.CASES)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    r = lc.run_case(name)
    assert lc.rel_err(r["eval_logits"], GOLD[f"{name}/eval_logits"]) < 1e-9
    assert lc.rel_err(r["train_logits"], GOLD[f"{name}/train_logits"]) < 1e-9
    assert abs(float(r["loss"]) - float(GOLD[f"{name}/loss"])) < 1e-9 * abs(float(GOLD[f"{name}/loss"]))
    for n in lc.BUFFERS:
        g = GOLD[f"{name}/running/{n}"]
        if n.endswith("num_batches_tracked"):
            assert int(r["running"][n]) == int(g)
        else:
            assert lc.rel_err(r["running"][n], g) < 1e-9, n
    for n in lc.PARAM_ORDER:
        assert lc.rel_err(lc.sample(r["grads"][n].numpy()), GOLD[f"{name}/grad/{n}"]) < 1e-9, n


@pytest.mark.parametrize("name", CASES)
def test_fixture_float32_margin_and_logit_gaps(name):
    """float32 on the CPU stays within 1e-5 of float64 (a 10x margin under the device's 1e-4 bound), and
    every row's top-2 logit gap exceeds 1e-3 of the largest logit (predictions must match exactly)."""
    a, b = lc.run_case(name, torch.float64), lc.run_case(name, torch.float32)
    for k in ("eval_logits", "train_logits"):
        assert lc.rel_err(b[k], a[k]) < 1e-5, k
        top = a[k].topk(2, dim=1).values
        assert float(((top[:, 0] - top[:, 1]) / a[k].abs().max()).min()) > 1e-3, k
    for n in lc.PARAM_ORDER:
        assert lc.rel_err(b["grads"][n], a["grads"][n]) < 1e-5, n
    # the unrolled layer (saved h / c oracle) is the library LSTM
    assert lc.rel_err(torch.cat([a["h2"][0], a["h2"][1]], -1), a["y2"]) < 1e-12
    assert lc.rel_err(torch.cat([a["h1"][0], a["h1"][1]], -1), a["y1"]) < 1e-12


@pytest.mark.parametrize("name", list(lc.ENVELOPE))
def test_envelope_float32_margin_and_logit_gaps(name):
    """The same conditions for the accepted-shape-range cases (lc.ENVELOPE), which the GPU bounds of
    tests/test_gpu_lstm_envelope.py rest on: float32 logits within 1e-5 of float64, the top-2 gap above 1e-3
    (one_class has one logit), every gradient tensor within 1e-5 -- or, where lc.ENVELOPE_BOUNDS records a
    measured device bound, within a tenth of it."""
    B, Tn, Fd, K, _ = lc.ENVELOPE[name]
    a, b = lc.run_case(name, torch.float64), lc.run_case(name, torch.float32)
    assert a["eval_logits"].shape == (B, K) and a["y2"].shape == (B, Tn, 128)
    for k in ("eval_logits", "train_logits"):
        assert lc.rel_err(b[k], a[k]) < 1e-5, k
        if K > 1:
            top = a[k].topk(2, dim=1).values
            assert float(((top[:, 0] - top[:, 1]) / a[k].abs().max()).min()) > 1e-3, k
    for n in lc.PARAM_ORDER:
        assert lc.rel_err(b["grads"][n], a["grads"][n]) < 0.1 * lc.grad_bound(name, n), n
    if name == "one_class":
        assert float(a["loss"]) == 0.0 and all(float(g.abs().max()) == 0.0 for g in a["grads"].values())
    assert lc.rel_err(torch.cat([a["h2"][0], a["h2"][1]], -1), a["y2"]) < 1e-12
    assert lc.rel_err(torch.cat([a["h1"][0], a["h1"][1]], -1), a["y1"]) < 1e-12


@pytest.mark.parametrize("geo", lc.DIGEST_MODELS)
def test_seeded_init_and_state_dict_match_the_reference(geo):
    K, Fd, Tn = geo
    torch.manual_seed(lc.DIGEST_SEED)
    m = lstmwithattention(K, Fd, Tn)
    sd = m.state_dict()
    keys = [k.split("/", 2)[2] for k in GOLD.files if k.startswith(f"digest/{K}_{Fd}_{Tn}/")]
    assert list(sd.keys()) == keys
    assert [n for n, _ in m.named_parameters()] == list(PARAM_ORDER) == list(lc.PARAM_ORDER)
    for k, d in lc.state_digest(sd).items():
        np.testing.assert_allclose(d, GOLD[f"digest/{K}_{Fd}_{Tn}/{k}"], rtol=1e-14, atol=0, err_msg=k)


def test_cpu_forward_raises():
    m = lstmwithattention(10, 13, 32)
    with pytest.raises(L.AbdError):
        m(torch.zeros(2, 1, 32, 13))


def test_geometry_mismatch_raises():
    m = lstmwithattention(10, 13, 32)

    class FakeDevice(torch.Tensor):
        is_cuda = True

    for shape in ((2, 1, 31, 13), (2, 1, 32, 14)):
        x = torch.zeros(shape).as_subclass(FakeDevice)
        with pytest.raises(ValueError):
            m(x)


def test_bf16_is_refused():
    m = lstmwithattention(10, 13, 32)
    with pytest.raises(L.AbdError):
        m.set_gemm_precision("bf16")
    with pytest.raises(ValueError):
        m.set_gemm_precision("fp8")
    assert m.set_gemm_precision("f32") is m


def test_checkpoint_is_a_reference_pickle(tmp_path):
    torch.manual_seed(3)
    m = lstmwithattention(10, 13, 32)
    p = tmp_path / "ckpt.pt"
    T.save_reference_checkpoint(m, str(p))
    import zipfile
    with zipfile.ZipFile(p) as z:
        data = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    ops = [(o.name, a) for o, a, _ in pickletools.genops(io.BytesIO(data))]
    globals_ = [a for n, a in ops if n == "GLOBAL"]
    assert "utils.models lstmwithattention" in globals_
    assert not any("abd_amd" in str(a) for _, a in ops if a is not None)
    # the state loads into a plain nn.Module of the same structure
    state = T.reference_module_state(m)
    plain = nn.Module()
    plain.__dict__.update(state)
    assert list(plain.state_dict().keys()) == list(m.state_dict().keys())
    for k, v in m.state_dict().items():
        assert torch.equal(plain.state_dict()[k], v), k
    assert isinstance(plain.rnn1, nn.LSTM) and isinstance(plain.dropout, nn.Dropout)
    assert "_engine" not in state and "dropout_source" not in state


def test_getstate_drops_the_engine():
    m = lstmwithattention(10, 13, 32)
    m._engine = object()
    st = m.__getstate__()
    assert st["_engine"] is None
    n = lstmwithattention.__new__(lstmwithattention)
    n.__setstate__({k: v for k, v in st.items() if k not in ("_step", "dropout_source")})
    assert n._step == 0 and n.dropout_source == "device" and n._engine is None


def test_header_symbols_are_exported():
    with open(os.path.join(HERE, "..", "include", "abd.h")) as f:
        names = sorted(set(re.findall(r"\b(abd_lstmattn_\w+)\s*\(", f.read())))
    assert len(names) == 11, names
    lib = abd_amd.load_library()
    for n in names:
        assert hasattr(lib, n), n
        assert n in L.EXPORTS, n


def test_create_refuses_unsupported_geometry():
    lib = abd_amd.load_library()
    h = C.c_void_p()
    assert lib.abd_lstmattn_create(32, 129, 10, C.byref(h)) == 1002
    assert lib.abd_lstmattn_create(0, 13, 10, C.byref(h)) == 1002
    assert lib.abd_lstmattn_create(1025, 13, 10, C.byref(h)) == 1002
    assert lib.abd_lstmattn_create(32, 0, 10, C.byref(h)) == 1002
    assert lib.abd_lstmattn_create(32, 13, 0, C.byref(h)) == 1002
    assert lib.abd_lstmattn_create(32, 13, 4097, C.byref(h)) == 1002
    for geo in ((1, 13, 10), (1024, 13, 10), (32, 1, 10), (32, 128, 10), (32, 13, 1), (32, 13, 4096)):   # the limits
        assert lib.abd_lstmattn_create(*geo, C.byref(h)) == 0, geo
        lib.abd_lstmattn_destroy(h)
    assert lib.abd_lstmattn_create(101, 40, 10, C.byref(h)) == 0
    offs = (C.c_int64 * 35)()
    assert lib.abd_lstmattn_param_offsets(h, offs) == 0
    sizes = [int(np.prod(s)) for s in lc.param_shapes(101, 40, 10).values()]
    assert list(offs) == [0] + list(np.cumsum(sizes))
    assert lib.abd_lstmattn_param_count(h) == sum(sizes)
    assert lib.abd_lstmattn_tile_rows() == lc.TILE
    assert lib.abd_lstmattn_workspace_offset(h, 4, b"y2") > 0
    assert lib.abd_lstmattn_workspace_offset(h, 4, b"nope") == -1
    lib.abd_lstmattn_destroy(h)


def test_train_still_refuses_a_foreign_module():
    class Foreign(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc = nn.Linear(4, 2)

    m = Foreign()
    opt = torch.optim.Adam(m.parameters())
    with pytest.raises(L.AbdError):
        T.train(m, [], "cpu", opt, nn.CrossEntropyLoss())
    with pytest.raises(L.AbdError):
        T.clean_test(m, "cpu", [], nn.CrossEntropyLoss())
    # the new model under an optimizer the fused step does not reproduce is refused as well
    lm = lstmwithattention(10, 13, 32)
    assert not T.fusable(lm, torch.optim.SGD(lm.parameters(), lr=0.1), nn.CrossEntropyLoss())
    assert T.fusable(lm, torch.optim.Adam(lm.parameters()), nn.CrossEntropyLoss())
    assert not T.fusable(lm, torch.optim.Adam(lm.parameters(), weight_decay=0.1), nn.CrossEntropyLoss())


class _FakeDevice(torch.Tensor):
    """A CPU tensor that claims to live on the device: gets past require_device, so the refusal under test
    is the one that fires (nothing is launched before it)."""
    is_cuda = True


def test_smallcnn_only_paths_refuse_the_model():
    """Data parallelism / SyncBN (ResidentTrainer, training.train_step), SGD fine-tuning and every defence entry
    point refuse lstmwithattention with AbdError -- also once an engine is bound, when the flat buffers exist."""
    from abd_amd import defense as D, pipeline as P

    class Eng:   # what a bound engine looks like to the duck-typed smallcnn paths
        device = torch.device("cpu")
        params = torch.zeros(4)
        running = torch.zeros(22)

    for bound in (False, True):
        m = lstmwithattention(10, 13, 32)
        if bound:
            m._engine = Eng()
            m._bound = lambda eng: True
        opt = torch.optim.Adam(m.parameters())
        x = torch.zeros((4, 1, 32, 13)).as_subclass(_FakeDevice)
        y = torch.zeros(4, dtype=torch.int64).as_subclass(_FakeDevice)
        calls = {
            "train_step": lambda: T.train_step(m, x, y, None, None, None, mask1=x, mask2=x),
            "ResidentTrainer": lambda: P.ResidentTrainer(None, None, None, m, opt, 4),
            "SgdBinding": lambda: T.SgdBinding(m, torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)),
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
                pytest.fail(f"{what} (bound={bound}) did not refuse lstmwithattention")


def test_flowmur_and_daba_refuse_the_model():
    from abd_amd import daba, flowmur
    m = lstmwithattention(10, 13, 32)
    with pytest.raises(L.AbdError):
        flowmur._as_abd_smallcnn(m)
    with pytest.raises((L.AbdError, NotImplementedError)):
        daba._require_cnn("lstmwithattention", m)


def test_train_mode_refuses_a_single_value_per_channel():
    """B*T*F == 1: BatchNorm has no variance to normalise by (torch raises as well); nothing is launched."""
    lib = abd_amd.load_library()
    h = C.c_void_p()
    assert lib.abd_lstmattn_create(1, 1, 3, C.byref(h)) == 0
    a = L.LstmAttnArgs()
    a.x = a.labels = a.params = a.grads = a.running = 16   # never dereferenced: the call returns before any launch
    a.batch = 1
    assert lib.abd_lstmattn_train_step(h, C.byref(a), None, 0, None) == 1001
    assert lib.abd_lstmattn_forward(h, C.byref(a), 1, None, 0, None) == 1001
    assert b"more than one value" in lib.abd_last_error()
    a.batch = 2
    assert lib.abd_lstmattn_train_step(h, C.byref(a), None, 0, None) == 1003   # past that check: no workspace
    lib.abd_lstmattn_destroy(h)
