"""CPU: the smalllstm fixture against the reference's golden file, the C ABI's host side, adoption and refusals."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import abd_amd
from abd_amd import _lib as L, training as T
from abd_amd.models_smalllstm import (smalllstm, PARAM_ORDER, BUFFER_ORDER, RUNNING_ORDER, adopt, adoptable,
                                      rnn_features, net_handle, tile_info)
import smalllstm_cases as sc
from test_gpu_smalllstm import Reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "smalllstm_golden.npz")
CASES = list(sc.CASES)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(golden, name):
    """float64 restate == the reference's own module in .double() (1e-11 relative; the gradients kept in full are
    stored as float32, and every gradient's float64 digest is compared as well)."""
    r = sc.run_case(name)
    grads = {k: v.numpy() for k, v in r["grads"].items()}
    mine = sc.golden_record(name, r["eval_logits"].numpy(), r["acts"]["logits"].numpy(), float(r["loss"]), grads,
                            {k: v.numpy() for k, v in r["running"].items()})
    assert sorted(k for k in golden if k.startswith(name + "/")) == sorted(mine)
    for k, v in mine.items():
        g = golden[k]
        scale = max(1.0, float(np.abs(g).max())) if g.size else 1.0
        tol = 1e-6 if g.dtype == np.float32 else 1e-11
        assert v.shape == g.shape and float(np.abs(np.asarray(v, dtype=np.float64) - g).max()) <= tol * scale, k


def test_golden_file_is_small_and_outputs_only(golden):
    assert os.path.getsize(GOLDEN) <= 1 << 20
    assert all(v.dtype in (np.float64, np.float32) for v in golden.values())
    B, H, W, K, _ = sc.CASES["ultrasonic"]
    assert golden["ultrasonic/eval_logits"].shape == (B, K)
    assert golden["daba/grad/fc2.weight"].shape == (10, 128) and not golden["daba/grad/fc1.bias"].any()


def _f32_distances(name):
    r64, r32 = sc.run_case(name, torch.float64), sc.run_case(name, torch.float32)
    d = {}
    for grp in ("acts", "grads", "running"):
        for k, v in r64[grp].items():
            if k.startswith("var"):   # compared as 1 / sqrt(var + eps), what the device saves
                a, b = (v + sc.BN_EPS).rsqrt(), (r32[grp][k] + sc.BN_EPS).rsqrt().double()
                d["invstd" + k[3:]] = float((a - b).abs().max())
            else:
                what = {"acts": k, "grads": f"grad {k}", "running": f"running {k}"}[grp]
                d["train_logits" if what == "logits" else what] = (
                    float((r32[grp][k].double() - v.double()).abs().max()) if v.numel() else 0.0)
    d["eval_logits"] = float((r32["eval_logits"].double() - r64["eval_logits"]).abs().max())
    return d


@pytest.mark.parametrize("name", CASES)
def test_fixture_float32_margin(name):
    """The float32 CPU restatement is within the bound of float64 on every tensor, and BOUNDS holds exactly the
    tensors where it is not within 1e-4 (at four times the distance measured when the fixture was written)."""
    d = _f32_distances(name)
    print(f"{name}: float32 restatement within {max(d.values()):.3e}")
    for k, e in d.items():
        assert e < sc.bound(name, k), (name, k, e)
        assert (e >= 1e-4) <= ((name, k) in sc.BOUNDS), (name, k, e)
    if sc.CASES[name][3] == 1:
        r64 = sc.run_case(name)
        assert all(not g.any() for g in r64["grads"].values()) and float(r64["loss"]) == 0.0


def test_ties_and_offset_cases_do_what_they_are_for():
    a = sc.run_case("ties")["acts"]
    assert all(float((a[f"z{i}"] == 0).double().mean()) > 0.5 for i in (1, 2, 3))
    assert (sc.make_state("ties")["bn2.weight"] < 0).all()
    o = sc.run_case("offset")["acts"]
    assert float((o["mean1"].abs() / (o["var1"] + sc.BN_EPS).sqrt()).max()) >= 10.0   # many standard deviations from 0


def test_case_sizes_follow_the_kernels_constants():
    abd_amd.load_library()
    got = [tile_info(k) for k in ("tile_rows", "k_step", "slice_rows", "max_slices", "stat_rows", "stat_blocks",
                                  "rec_rows")]
    assert got == [sc.TILE_ROWS, sc.K_STEP, sc.SLICE_ROWS, sc.MAX_SLICES, sc.STAT_ROWS, sc.STAT_BLOCKS, sc.REC_ROWS]
    B = sc.RAGGED_B
    assert sc.CASES["ragged"][0] == B == sc.ragged_batch(*[got[i] for i in (4, 2, 0, 3, 1, 6)]) <= 64
    g = sc.geometry(*sc.RAGGED_HW)
    px = g[3] * g[4] * B
    assert px > sc.STAT_ROWS and sc.plan_slices(px)[0] >= 2 and px % sc.TILE_ROWS
    assert B > sc.REC_ROWS and B % sc.REC_ROWS


def test_header_symbols_are_exported():
    with open(os.path.join(ROOT, "include", "abd.h")) as f:
        names = sorted(set(re.findall(r"\b(abd_smalllstm_\w+)\s*\(", f.read())))
    assert len(names) == 14 and "abd_smalllstm_create" in names, names
    lib = abd_amd.load_library()
    for n in names:
        assert hasattr(lib, n), n
        assert n in L.EXPORTS, n
    assert C.sizeof(L.SmallLstmArgs) == C.sizeof(L.LstmAttnArgs) == 176   # abd_smalllstm_args on LP64


def test_geometry_offsets_and_workspace_names(golden):
    lib = abd_amd.load_library()
    for H, W, T_, F_ in ((100, 40, 24, 128), (101, 40, 24, 128), (32, 40, 7, 128), (32, 13, 7, 32), (6, 10, 1, 32)):
        assert rnn_features(H, W) == F_ == sc.rnn_features(H, W) and sc.geometry(H, W)[-2] == T_
    for H in range(1, 40):
        for W in range(1, 60):
            assert rnn_features(H, W) == sc.rnn_features(H, W), (H, W)
    # the reference's own module accepted the geometry of every case: the golden shapes are (B, K)
    for name, (B, H, W, K, _) in sc.CASES.items():
        assert golden[f"{name}/train_logits"].shape == (B, K)
    h = C.c_void_p()
    for H, W, K in ((5, 10, 3), (6, 9, 3), (4097, 13, 3), (6, 4097, 3), (6, 10, 0), (6, 10, 4097)):
        assert lib.abd_smalllstm_create(H, W, K, C.byref(h)) == 1002   # ABD_E_UNSUPPORTED
    assert lib.abd_smalllstm_create(6, 10, 3, None) != 0
    for name in ("tiny", "jingleback", "k35"):
        B, H, W, K, _ = sc.CASES[name]
        h = net_handle(H, W, K)
        shapes = sc.param_shapes(sc.rnn_features(H, W), K)
        offs = (C.c_int64 * 25)()
        assert lib.abd_smalllstm_param_offsets(h, offs) == 0
        want = np.cumsum([0] + [int(np.prod(shapes[n])) for n in PARAM_ORDER])
        assert list(offs) == list(want) and lib.abd_smalllstm_param_count(h) == want[-1]
        roffs = (C.c_int64 * 4)()
        assert lib.abd_smalllstm_running_offsets(h, roffs) == 0
        assert list(roffs) == list(np.cumsum([0] + [2 * c for _, c in RUNNING_ORDER]))
        assert lib.abd_smalllstm_running_count(h) == 320
        total = lib.abd_smalllstm_workspace_bytes(h, B)
        H1, W1, Wp1, H2, W2, Hp2, Wp2, H3, W3, TS, Wf = sc.geometry(H, W)
        sizes = {"z1": H1 * W1 * 64, "a1": H1 * W1 * 64, "p1": H1 * Wp1 * 64, "z2": H2 * W2 * 64, "a2": H2 * W2 * 64,
                 "p2": Hp2 * Wp2 * 64, "z3": H3 * W3 * 32, "a3": H3 * W3 * 32, "p3": TS * Wf * 32, "seq": TS * Wf * 32,
                 "h0": TS * 128, "c0": TS * 128, "g0": TS * 512, "h1": TS * 128, "c1": TS * 128, "g1": TS * 512,
                 "logits": K}
        seen = []
        for k, per in sizes.items():
            off = lib.abd_smalllstm_workspace_offset(h, B, k.encode())
            assert off >= 0 and off % 256 == 0 and off + 4 * B * per <= total, k
            seen.append((off, 4 * B * per))
        for k, c in (("s1", 64), ("s2", 64), ("s3", 32)):
            off = lib.abd_smalllstm_workspace_offset(h, B, k.encode())
            assert off >= 0 and off % 256 == 0 and off + 8 * c <= total
            seen.append((off, 8 * c))
        seen.sort()
        assert all(a + n <= b for (a, n), (b, _) in zip(seen, seen[1:]))   # no two saved maps overlap
        for bad in (b"z4", b"a0", b"s", b"nothing", b"h2"):
            assert lib.abd_smalllstm_workspace_offset(h, B, bad) == -1
        assert lib.abd_smalllstm_workspace_bytes(h, 0) == 0
        lib.abd_smalllstm_destroy(h)


def test_argument_checks_return_the_expected_codes():
    """NULL pointers, a missing label, a bad batch, a short or misaligned workspace: refused before any launch (no
    device is present here), with abd_resnet_*'s codes."""
    lib = abd_amd.load_library()
    h = net_handle(6, 10, 3)
    need = lib.abd_smalllstm_workspace_bytes(h, 2)
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    a = L.SmallLstmArgs()
    invalid, workspace = 1001, 1003
    assert lib.abd_smalllstm_train_step(h, None, p, need, None) == invalid
    assert lib.abd_smalllstm_forward(h, C.byref(a), 1, p, need, None) == invalid           # NULL x
    a.x, a.batch, a.params, a.grads = p, 2, p, p
    assert lib.abd_smalllstm_train_step(h, C.byref(a), p, need, None) == invalid           # no labels
    a.labels = p
    a.do_update = 1
    assert lib.abd_smalllstm_train_step(h, C.byref(a), p, need, None) == invalid           # no Adam moments
    a.do_update = 0
    assert lib.abd_smalllstm_train_step(h, C.byref(a), p, need - 1, None) == workspace
    assert lib.abd_smalllstm_train_step(h, C.byref(a), None, need, None) == workspace
    assert lib.abd_smalllstm_train_step(h, C.byref(a), p + 4, need, None) == invalid       # misaligned
    assert lib.abd_smalllstm_forward(h, C.byref(a), 0, p, need, None) == invalid           # eval without running
    assert lib.abd_smalllstm_backward(h, C.byref(a), None, p, need, None) == invalid
    a.batch = 0
    assert lib.abd_smalllstm_train_step(h, C.byref(a), p, need, None) == invalid
    a.batch = 1 << 40
    assert lib.abd_smalllstm_train_step(h, C.byref(a), p, need, None) == invalid
    assert lib.abd_smalllstm_eval(h, None, 2, p, p, None, None, p, None, p, need, None) == invalid
    assert lib.abd_smalllstm_eval(h, p, 2, p, None, None, None, p, None, p, need, None) == invalid
    assert lib.abd_smalllstm_eval(h, p, 2, p, p, None, None, p, None, p, 16, None) == workspace
    lib.abd_smalllstm_destroy(h)


def test_class_matches_the_reference_shape():
    torch.manual_seed(3)
    a = smalllstm(10, 128)
    torch.manual_seed(3)
    b = Reference(10, 128)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [n for n, _ in a.named_parameters()] == list(PARAM_ORDER) == list(sc.PARAM_ORDER)
    assert [n for n, _ in a.named_buffers()] == list(BUFFER_ORDER) == list(sc.BUFFER_ORDER)
    assert [n for n, _ in a.named_children()] == [n for n, _ in b.named_children()]
    assert sum(p.numel() for p in a.parameters()) == 319594
    assert {k: tuple(v.shape) for k, v in sa.items() if k in PARAM_ORDER} == sc.param_shapes(128, 10)


def test_fusable_truth_table_and_adoption():
    crit = nn.CrossEntropyLoss()
    for m in (smalllstm(10, 32), Reference(10, 32)):
        assert isinstance(T.accelerated(m), smalllstm)
        assert T.fusable(m, torch.optim.Adam(m.parameters()), crit)
        assert not T.fusable(m, torch.optim.SGD(m.parameters(), lr=0.1), crit)
        assert not T.fusable(m, torch.optim.Adam(m.parameters(), weight_decay=1e-4), crit)
        assert not T.fusable(m, torch.optim.Adam(list(m.parameters())[:-1]), crit)
        assert not T.fusable(m, torch.optim.Adam(m.parameters()), nn.NLLLoss())
        with pytest.raises(L.AbdError, match="smalllstm"):
            T.train(m, [], "cpu", torch.optim.SGD(m.parameters(), lr=0.1), crit)
    assert smalllstm in T.ACCELERATED


def test_adopt_shares_modules_parameters_and_buffers():
    ref = Reference(10, 32)
    assert adoptable(ref) and not adoptable(smalllstm(10, 32)) and not adoptable(nn.Linear(2, 2))
    ad = adopt(ref)
    assert ad is adopt(ref) and adopt(ad) is ad and isinstance(ad, smalllstm) and not hasattr(ref, "_engine")
    assert [id(p) for p in ad.parameters()] == [id(p) for p in ref.parameters()]
    assert [id(b) for b in ad.buffers()] == [id(b) for b in ref.buffers()]
    assert ad.rnn is ref.rnn and list(ad.state_dict()) == list(ref.state_dict())
    assert ad.training == ref.training
    ref.bn2 = nn.BatchNorm2d(64)          # the cache notices a replaced layer
    ad2 = adopt(ref)
    assert ad2 is not ad and ad2.bn2 is ref.bn2


EDITS = {
    "3x3 conv": lambda m: setattr(m, "conv2", nn.Conv2d(64, 64, 3)),
    "padded conv": lambda m: setattr(m, "conv1", nn.Conv2d(1, 64, 2, padding=1)),
    "pool padding": lambda m: setattr(m, "pool2", nn.MaxPool2d((2, 2), padding=(0, 1))),
    "ceil_mode": lambda m: setattr(m, "pool3", nn.MaxPool2d((2, 2), padding=(0, 1), ceil_mode=True)),
    "pool kernel": lambda m: setattr(m, "pool1", nn.MaxPool2d((1, 2))),
    "bidirectional": lambda m: setattr(m, "rnn", nn.LSTM(32, 128, 2, batch_first=True, bidirectional=True)),
    "3 layers": lambda m: setattr(m, "rnn", nn.LSTM(32, 128, 3, batch_first=True)),
    "64 wide": lambda m: setattr(m, "rnn", nn.LSTM(32, 64, 2, batch_first=True)),
    "batch_first=False": lambda m: setattr(m, "rnn", nn.LSTM(32, 128, 2)),
    "LSTM dropout": lambda m: setattr(m, "rnn", nn.LSTM(32, 128, 2, batch_first=True, dropout=0.1)),
    "GRU": lambda m: setattr(m, "rnn", nn.GRU(32, 128, 2, batch_first=True)),
    "dropout p": lambda m: setattr(m, "drop1", nn.Dropout(0.5)),
    "BatchNorm momentum": lambda m: setattr(m.bn1, "momentum", 0.2),
    "BatchNorm eps": lambda m: setattr(m.bn3, "eps", 1e-3),
    "double": lambda m: m.double(),
    "extra parameter": lambda m: m.register_parameter("scale", nn.Parameter(torch.ones(1))),
    "extra buffer": lambda m: m.register_buffer("seen", torch.zeros(1)),
    "missing fc1": lambda m: delattr(m, "fc1"),
    "fc1 width": lambda m: setattr(m, "fc1", nn.Linear(672, 128)),
}


@pytest.mark.parametrize("edit", list(EDITS))
def test_adopt_refuses_another_structure(edit):
    m = Reference(10, 32)
    EDITS[edit](m)
    with pytest.raises(L.AbdError):
        adopt(m)
    with pytest.raises(L.AbdError):
        T.fusable(m, torch.optim.Adam(m.parameters()), nn.CrossEntropyLoss())
    with pytest.raises(L.AbdError):
        T.test(m, "cpu", [], [], None)


def test_adopt_refuses_other_names():
    class Other(nn.Module):
        pass
    with pytest.raises(L.AbdError):
        adopt(Other())
    with pytest.raises(L.AbdError):
        adopt(nn.Linear(2, 2))


def test_cpu_tensors_bf16_and_geometry_are_refused():
    m = smalllstm(10, 32)
    with pytest.raises(L.AbdError):
        m(torch.zeros(2, 1, 32, 13))                      # a CPU tensor
    with pytest.raises(L.AbdError):
        m.set_gemm_precision("bf16")
    assert m.set_gemm_precision("f32") is m
    with pytest.raises(ValueError):
        m.set_gemm_precision("fp8")
    with pytest.raises(L.AbdError):
        adopt(Reference(10, 32)).set_gemm_precision("bf16")


def test_smallcnn_only_paths_refuse_the_model():
    """Data parallelism / SyncBN, SGD, FlowMur, DABA's victim loader and the defences refuse smalllstm, this
    package's class and a reference-shaped instance alike."""
    from abd_amd import daba, defense as D, flowmur, pipeline as P
    for make in (lambda: smalllstm(10, 32), lambda: Reference(10, 32)):
        m = make()
        opt = torch.optim.Adam(m.parameters())
        x, y = torch.zeros((4, 1, 32, 13)), torch.zeros(4, dtype=torch.int64)
        calls = {
            "train_step": lambda: T.train_step(m, x, y, None, None, None, mask1=x, mask2=x),
            "ResidentTrainer": lambda: P.ResidentTrainer(None, None, None, m, opt, 4),
            "SgdBinding": lambda: T.SgdBinding(m, torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)),
            "check_sgd": lambda: T.check_sgd(m, torch.optim.SGD(m.parameters(), lr=0.1)),
            "flat_state": lambda: D._flat_state(m, torch.device("cpu")),
            "ablation_sweep": lambda: D.ablation_sweep(m, x, y, torch.zeros((1, 160), dtype=torch.uint8)),
            "neuron_loss_change": lambda: D.neuron_loss_change(m, x, y),
            "hidden_activation": lambda: D.hidden_activation(m, x),
            "neuron_names": lambda: D.neuron_names(m),
            "param_offsets": lambda: D.param_offsets(m),
            "row_table": lambda: D.row_table(m),
            "neuron_weight_change": lambda: D.neuron_weight_change(m, torch.zeros(4)),
            "model_with_params": lambda: D.model_with_params(m, torch.zeros(4)),
            "final_gradients": lambda: D.final_gradients(m),
            "finetune_epoch": lambda: D.finetune_epoch(m, x, y, torch.optim.SGD(m.parameters(), lr=0.1)),
            "unlearn_epoch": lambda: D.unlearn_epoch(m, x, y, opt),
            "pruned_finetune_epoch": lambda: D.pruned_finetune_epoch(m, x, y, opt, torch.zeros(128)),
            "flowmur_as_smallcnn": lambda: flowmur._as_abd_smallcnn(m),
            "flowmur_trigger": lambda: flowmur.TriggerOptimizer(m.eval(), 4000),
            "daba_victim": lambda: daba.load_victim_model(types.SimpleNamespace(model="smalllstm", num_classes=10,
                                                                                n_mfcc=40)),
        }
        for what, call in calls.items():
            with pytest.raises(L.AbdError):
                call()
                pytest.fail(f"{what} did not refuse {type(m).__module__}.smalllstm")


def test_reference_checkpoint_names_the_reference_class(tmp_path):
    m = smalllstm(3, 32)
    path = str(tmp_path / "m.pkl")
    T.save_reference_checkpoint(m, path)
    with open(path, "rb") as f:
        blob = f.read()
    assert b"utils.models" in blob and b"smalllstm" in blob and b"abd_amd" not in blob


def test_dropin_names_are_untouched():
    path = os.path.join(ROOT, "audio-backdoor-attack_amd", "dropin", "utils", "models.py")
    with open(path) as f:
        assert '_OTHERS = ("largecnn", "smalllstm", "ResNet", "ResidualBlock")' in f.read()


def test_getstate_drops_the_engine():
    m = smalllstm(10, 32)
    m._engine = object()
    assert m.__getstate__()["_engine"] is None
