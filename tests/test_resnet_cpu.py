"""CPU: the ResNet fixture against the reference's golden file, the C ABI's host side, adoption and refusals."""
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
from abd_amd.models_resnet import (ResNet, ResidualBlock, PARAM_ORDER, BUFFER_ORDER, RUNNING_ORDER, adopt, adoptable,
                                   linear_features, net_handle, tile_info)
import resnet_cases as rc
from test_gpu_resnet import Reference, RefBlock, conv3x3, state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resnet_golden.npz")
CASES = list(rc.CASES)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(golden, name):
    """float64 restate == the reference's own module in .double() (1e-12 relative; the gradients kept in full are
    stored as float32, 6e-8 relative, and every gradient's float64 digest is compared as well)."""
    r = rc.run_case(name)
    grads = {k: v.numpy() for k, v in r["grads"].items()}
    mine = rc.golden_record(name, r["eval_logits"].numpy(), r["acts"]["logits"].numpy(), float(r["loss"]), grads,
                            {k: v.numpy() for k, v in r["running"].items()})
    assert sorted(k for k in golden if k.startswith(name + "/")) == sorted(mine)
    for k, v in mine.items():
        g = golden[k]
        scale = max(1.0, float(np.abs(g).max())) if g.size else 1.0
        tol = 1e-6 if g.dtype == np.float32 else 1e-11
        assert v.shape == g.shape and float(np.abs(np.asarray(v, dtype=np.float64) - g).max()) <= tol * scale, k


def test_golden_file_is_small_and_outputs_only(golden):
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "largecnn_golden.npz"))
    assert all(v.dtype in (np.float64, np.float32) for v in golden.values())


@pytest.mark.parametrize("name", CASES)
def test_fixture_float32_margin(name):
    """The float32 CPU restatement is within the bound of float64 on every tensor: no relu of the case sits on a
    rounding boundary, and the bound has room for float32 arithmetic."""
    r64, r32 = rc.run_case(name, torch.float64), rc.run_case(name, torch.float32)
    worst = 0.0
    for grp in ("acts", "grads", "running"):
        for k, v in r64[grp].items():
            e = float((r32[grp][k].double() - v.double()).abs().max()) if v.numel() else 0.0
            worst = max(worst, e)
            assert e < rc.bound(name, k), (name, grp, k, e)
    e = float((r32["eval_logits"].double() - r64["eval_logits"]).abs().max())
    print(f"{name}: float32 restatement within {max(worst, e):.3e}")
    assert e < rc.bound(name, "eval_logits")
    if rc.CASES[name][3] == 1:
        assert all(not g.any() for g in r64["grads"].values()) and float(r64["loss"]) == 0.0


def test_offset_case_has_a_large_mean():
    a = rc.run_case("offset")["acts"]
    assert float((a["mean0"].abs() / a["var0"].sqrt()).min()) >= 10.0


def test_case_sizes_follow_the_kernels_constants():
    abd_amd.load_library()
    got = [tile_info(k) for k in ("tile_rows", "k_step", "slice_rows", "max_slices", "stat_rows", "stat_blocks")]
    assert got == [rc.TILE_ROWS, rc.K_STEP, rc.SLICE_ROWS, rc.MAX_SLICES, rc.STAT_ROWS, rc.STAT_BLOCKS]
    B = rc.RAGGED_B
    assert rc.CASES["ragged"][0] == B == rc.ragged_batch(*[got[i] for i in (4, 2, 0, 3, 1)])
    assert 325 * B > rc.STAT_ROWS and rc.plan_slices(325 * B)[0] >= 2 and (325 * B) % rc.TILE_ROWS
    assert not (325 * (B - 1) > rc.STAT_ROWS and rc.plan_slices(325 * (B - 1))[0] >= 2 and (325 * (B - 1)) % rc.TILE_ROWS)


def test_header_symbols_are_exported():
    with open(os.path.join(ROOT, "include", "abd.h")) as f:
        names = sorted(set(re.findall(r"\b(abd_resnet_\w+)\s*\(", f.read())))
    assert len(names) == 14, names
    lib = abd_amd.load_library()
    for n in names:
        assert hasattr(lib, n), n
        assert n in L.EXPORTS, n
    assert C.sizeof(L.ResNetArgs) == 136   # abd_resnet_args on LP64


def test_create_limits_offsets_and_workspace_names():
    lib = abd_amd.load_library()
    for H, W, lf in ((100, 40, 384), (101, 40, 384), (32, 40, 128), (32, 13, 64), (25, 13, 64), (24, 13, -1),
                     (25, 12, -1)):
        assert linear_features(H, W) == lf == rc.linear_features(H, W)
    h = C.c_void_p()
    for H, W, K in ((24, 13, 3), (25, 12, 3), (4097, 13, 3), (25, 4097, 3), (25, 13, 0), (25, 13, 4097)):
        assert lib.abd_resnet_create(H, W, K, C.byref(h)) == 1002   # ABD_E_UNSUPPORTED
    assert lib.abd_resnet_create(25, 13, 3, None) != 0
    for name in ("tiny", "jingleback", "k35"):
        B, H, W, K, _ = rc.CASES[name]
        h = net_handle(H, W, K)
        shapes = rc.param_shapes(rc.linear_features(H, W), K)
        offs = (C.c_int64 * 50)()
        assert lib.abd_resnet_param_offsets(h, offs) == 0
        want = np.cumsum([0] + [int(np.prod(shapes[n])) for n in PARAM_ORDER])
        assert list(offs) == list(want) and lib.abd_resnet_param_count(h) == want[-1]
        roffs = (C.c_int64 * 16)()
        assert lib.abd_resnet_running_offsets(h, roffs) == 0
        assert list(roffs) == list(np.cumsum([0] + [2 * c for _, c in RUNNING_ORDER]))
        assert lib.abd_resnet_running_count(h) == 1120
        total = lib.abd_resnet_workspace_bytes(h, B)
        seen = []
        for u in range(15):
            shp = rc.unit_shape(u, B, H, W)
            n = 4 * int(np.prod(shp))
            for k, size in (("z", n), ("a", n), ("s", 8 * shp[1])):
                off = lib.abd_resnet_workspace_offset(h, B, f"{k}{u}".encode())
                assert off >= 0 and off % 256 == 0 and off + size <= total
                seen.append((off, size))
        H2, W2, H3, W3, H4, PH, PW = rc.geometry(H, W)
        for k, size in (("sub", 4 * B * H4 * W3 * 64), ("c2", 4 * B * H4 * W3 * 64), ("pool", 4 * B * 64 * PH * PW),
                        ("logits", 4 * B * K), ("dlogits", 4 * B * K), ("rowinfo", 16 * B)):
            off = lib.abd_resnet_workspace_offset(h, B, k.encode())
            assert off >= 0 and off % 256 == 0 and off + size <= total
            seen.append((off, size))
        seen.sort()
        assert all(a + n <= b for (a, n), (b, _) in zip(seen, seen[1:]))   # no two saved maps overlap
        for bad in (b"z15", b"a-1", b"s", b"nothing", b"z1x"):
            assert lib.abd_resnet_workspace_offset(h, B, bad) == -1
        assert lib.abd_resnet_workspace_bytes(h, 0) == 0
        lib.abd_resnet_destroy(h)


def test_argument_checks_return_the_expected_codes():
    """NULL pointers, a missing label, a bad batch, a short or misaligned workspace: refused before any launch (no
    device is present here), with abd_largecnn_*'s codes."""
    lib = abd_amd.load_library()
    h = net_handle(25, 13, 3)
    need = lib.abd_resnet_workspace_bytes(h, 2)
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    a = L.ResNetArgs()
    invalid, workspace = 1001, 1003
    assert lib.abd_resnet_train_step(h, None, p, need, None) == invalid
    assert lib.abd_resnet_forward(h, C.byref(a), 1, p, need, None) == invalid           # NULL x
    a.x, a.batch, a.params, a.grads = p, 2, p, p
    assert lib.abd_resnet_train_step(h, C.byref(a), p, need, None) == invalid           # no labels
    a.labels = p
    a.do_update = 1
    assert lib.abd_resnet_train_step(h, C.byref(a), p, need, None) == invalid           # no Adam moments
    a.do_update = 0
    assert lib.abd_resnet_train_step(h, C.byref(a), p, need - 1, None) == workspace
    assert lib.abd_resnet_train_step(h, C.byref(a), None, need, None) == workspace
    assert lib.abd_resnet_train_step(h, C.byref(a), p + 4, need, None) == invalid       # misaligned
    assert lib.abd_resnet_forward(h, C.byref(a), 0, p, need, None) == invalid           # eval without running
    assert lib.abd_resnet_backward(h, C.byref(a), None, p, need, None) == invalid
    a.batch = 0
    assert lib.abd_resnet_train_step(h, C.byref(a), p, need, None) == invalid
    a.batch = 1 << 40
    assert lib.abd_resnet_train_step(h, C.byref(a), p, need, None) == invalid
    assert lib.abd_resnet_eval(h, None, 2, p, p, None, None, p, None, p, need, None) == invalid
    assert lib.abd_resnet_eval(h, p, 2, p, None, None, None, p, None, p, need, None) == invalid
    assert lib.abd_resnet_eval(h, p, 2, p, p, None, None, p, None, p, 16, None) == workspace
    lib.abd_resnet_destroy(h)


def test_class_matches_the_reference_shape():
    torch.manual_seed(3)
    a = ResNet(ResidualBlock, [2, 2, 2], 10, 384)
    torch.manual_seed(3)
    b = Reference(10, 384)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [n for n, _ in a.named_parameters()] == list(PARAM_ORDER) == list(rc.PARAM_ORDER)
    assert [n for n, _ in a.named_buffers()] == list(BUFFER_ORDER) == list(rc.BUFFER_ORDER)
    assert sum(p.numel() for p in a.parameters()) == 202810
    with pytest.raises(L.AbdError):
        ResNet(ResidualBlock, [1, 1, 1], 10, 384)
    with pytest.raises(L.AbdError):
        ResNet(RefBlock, [2, 2, 2], 10, 384)


def test_fusable_truth_table_and_adoption():
    crit = nn.CrossEntropyLoss()
    for m in (ResNet(ResidualBlock, [2, 2, 2], 10, 64), Reference(10, 64)):
        assert isinstance(T.accelerated(m), ResNet)
        assert T.fusable(m, torch.optim.Adam(m.parameters()), crit)
        assert not T.fusable(m, torch.optim.SGD(m.parameters(), lr=0.1), crit)
        assert not T.fusable(m, torch.optim.Adam(m.parameters(), weight_decay=1e-4), crit)
        assert not T.fusable(m, torch.optim.Adam(m.parameters(), amsgrad=True), crit)
        assert not T.fusable(m, torch.optim.Adam(list(m.parameters())[:-1]), crit)
        assert not T.fusable(m, torch.optim.Adam(m.parameters()), nn.NLLLoss())
        assert not T.fusable(m, torch.optim.Adam(m.parameters()), nn.CrossEntropyLoss(label_smoothing=0.1))
        with pytest.raises(L.AbdError, match="ResNet"):
            T.train(m, [], "cpu", torch.optim.SGD(m.parameters(), lr=0.1), crit)
    assert ResNet in T.ACCELERATED


def test_adopt_shares_modules_parameters_and_buffers():
    ref = Reference(10, 64)
    assert adoptable(ref) and not adoptable(ResNet(ResidualBlock, [2, 2, 2], 10, 64)) and not adoptable(nn.Linear(2, 2))
    ad = adopt(ref)
    assert ad is adopt(ref) and adopt(ad) is ad and isinstance(ad, ResNet) and not hasattr(ref, "_engine")
    assert [id(p) for p in ad.parameters()] == [id(p) for p in ref.parameters()]
    assert [id(b) for b in ad.buffers()] == [id(b) for b in ref.buffers()]
    assert ad.layer2[0].downsample[1] is ref.layer2[0].downsample[1] and list(ad.state_dict()) == list(ref.state_dict())
    assert ad.training == ref.training
    ref.layer3[1].bn2 = nn.BatchNorm2d(64)          # the cache notices a replaced layer
    ad2 = adopt(ref)
    assert ad2 is not ad and ad2.layer3[1].bn2 is ref.layer3[1].bn2


def _edit_layers(m):
    m.layer1 = nn.Sequential(RefBlock(16, 16))
    m.layer2 = nn.Sequential(RefBlock(16, 32, 2, nn.Sequential(conv3x3(16, 32, 2), nn.BatchNorm2d(32))))
    m.layer3 = nn.Sequential(RefBlock(32, 64, 2, nn.Sequential(conv3x3(32, 64, 2), nn.BatchNorm2d(64))))


EDITS = {
    "layers [1, 1, 1]": _edit_layers,
    "biased conv3x3": lambda m: setattr(m.layer1[0], "conv1", nn.Conv2d(16, 16, 3, padding=1, bias=True)),
    "5x5 kernel": lambda m: setattr(m.layer1[1], "conv2", nn.Conv2d(16, 16, 5, padding=2, bias=False)),
    "missing downsample": lambda m: setattr(m.layer2[0], "downsample", None),
    "extra downsample": lambda m: setattr(m.layer1[0], "downsample", nn.Sequential(conv3x3(16, 16), nn.BatchNorm2d(16))),
    "AvgPool2d(2)": lambda m: setattr(m, "avg_pool", nn.AvgPool2d(2)),
    "double": lambda m: m.double(),
    "extra parameter": lambda m: m.register_parameter("scale", nn.Parameter(torch.ones(1))),
    "extra buffer": lambda m: m.register_buffer("seen", torch.zeros(1)),
    "conv2d stride": lambda m: setattr(m, "conv2d", nn.Conv2d(64, 64, 1, stride=2)),
    "BatchNorm momentum": lambda m: setattr(m.bn, "momentum", 0.2),
    "stride-1 stage": lambda m: setattr(m.layer2[0], "conv1", conv3x3(16, 32, 1)),
}


@pytest.mark.parametrize("edit", list(EDITS))
def test_adopt_refuses_another_structure(edit):
    m = Reference(10, 64)
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
    m = ResNet(ResidualBlock, [2, 2, 2], 10, 64)
    with pytest.raises(L.AbdError):
        m(torch.zeros(2, 1, 32, 13))                      # a CPU tensor
    with pytest.raises(L.AbdError):
        m.set_gemm_precision("bf16")
    assert m.set_gemm_precision("f32") is m
    with pytest.raises(ValueError):
        m.set_gemm_precision("fp8")
    with pytest.raises(L.AbdError):
        adopt(Reference(10, 64)).set_gemm_precision("bf16")


def test_smallcnn_only_paths_refuse_the_model():
    """Data parallelism / SyncBN, SGD, FlowMur, DABA's victim loader and the defences refuse ResNet, this package's
    class and a reference-shaped instance alike."""
    from abd_amd import daba, defense as D, flowmur, pipeline as P
    for make in (lambda: ResNet(ResidualBlock, [2, 2, 2], 10, 64), lambda: Reference(10, 64)):
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
            "daba_victim": lambda: daba.load_victim_model(types.SimpleNamespace(model="ResNet", num_classes=10,
                                                                                n_mfcc=40)),
        }
        for what, call in calls.items():
            with pytest.raises(L.AbdError):
                call()
                pytest.fail(f"{what} did not refuse {type(m).__module__}.ResNet")


def test_dropin_names_are_untouched():
    path = os.path.join(ROOT, "audio-backdoor-attack_amd", "dropin", "utils", "models.py")
    with open(path) as f:
        assert '_OTHERS = ("largecnn", "smalllstm", "ResNet", "ResidualBlock")' in f.read()


def test_getstate_drops_the_engine():
    m = ResNet(ResidualBlock, [2, 2, 2], 10, 64)
    m._engine = object()
    assert m.__getstate__()["_engine"] is None
