"""CPU: largecnn's fixture, Python surface and C ABI surface (no device needed).

The restatement of tests/largecnn_cases.py is tied to the reference's own module through
tests/golden/largecnn_golden.npz, and the conditions the GPU bounds rest on are asserted here.
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
from abd_amd.models_largecnn import largecnn, PARAM_ORDER, adopt, linear_features, tile_info
import largecnn_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "largecnn_golden.npz"))
SCRIPT_GEOMETRIES = (((100, 40), 12288), ((101, 40), 12288), ((32, 40), 3072), ((32, 13), 768))


@pytest.mark.parametrize("name", list(lc.CASES))
def test_restatement_reproduces_the_reference(name):
    """The golden values are the reference's module in float64: the float64 restatement (the same torch
    primitives) reproduces them to rounding."""
    tol = 1e-9
    r = lc.run_case(name, torch.float64)
    assert lc.rel_err(r["eval_logits"], GOLD[f"{name}/eval_logits"]) < tol
    assert lc.rel_err(r["acts"]["logits"], GOLD[f"{name}/train_logits"]) < tol
    g = float(GOLD[f"{name}/loss"])
    assert abs(float(r["loss"]) - g) <= tol * max(abs(g), 1.0)
    for n in lc.PARAM_ORDER:
        got = r["grads"][n].numpy()
        if n in lc.FULL_GRADS:
            assert lc.rel_err(got, GOLD[f"{name}/grad/{n}"]) < tol, n
            continue
        stats, sample = lc.digest(got)
        want = GOLD[f"{name}/gradstats/{n}"]
        scale = float(want[1])   # the L2 norm bounds what rounding can move the sum by
        assert abs(stats[1] - want[1]) <= tol * scale, n
        assert abs(stats[0] - want[0]) <= tol * scale * np.sqrt(got.size), n
        assert lc.rel_err(sample, GOLD[f"{name}/gradsample/{n}"]) < tol or scale == 0.0, n


def test_golden_file_is_small_and_outputs_only():
    assert os.path.getsize(os.path.join(HERE, "golden", "largecnn_golden.npz")) < 1 << 20
    kinds = {k.split("/")[1] for k in GOLD.files}
    assert kinds == {"eval_logits", "train_logits", "loss", "grad", "gradstats", "gradsample"}
    assert all(GOLD[k].size <= lc.SAMPLE_MAX for k in GOLD.files if "/gradsample/" in k)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_fixture_float32_margin_and_logit_gaps(name):
    """float32 on the CPU stays within 1e-5 of float64 (a 10x margin under the device's 1e-4 bound) -- or, where
    lc.BOUNDS records a bound, within a quarter of it -- and every row's top-2 gap exceeds 1e-3 of the largest
    log-probability (predictions must match exactly).  The distances are printed (profiles/largecnn/parity.md)."""
    B, H, W, K, _ = lc.CASES[name]
    a, b = lc.run_case(name, torch.float64), lc.run_case(name, torch.float32)
    assert a["eval_logits"].shape == (B, K)
    for which in ("eval_logits",):
        assert lc.rel_err(b[which], a[which]) < 1e-5
    assert lc.rel_err(b["acts"]["logits"], a["acts"]["logits"]) < 1e-5
    if K > 1:
        for lp in (a["eval_logits"], a["acts"]["logits"]):
            top = lp.topk(2, dim=1).values
            assert float(((top[:, 0] - top[:, 1]) / lp.abs().max()).min()) > 1e-3
    for n in lc.PARAM_ORDER:
        e = lc.rel_err(b["grads"][n], a["grads"][n])
        print(f"{name} float32 CPU grad {n}: {e:.3e}")
        assert e < (0.25 * lc.BOUNDS[(name, n)] if (name, n) in lc.BOUNDS else 1e-5), n
    if name == "k1":
        assert float(a["loss"]) == 0.0 and all(float(g.abs().max()) == 0.0 for g in a["grads"].values())
    else:
        assert all(float(g.abs().max()) > 0.0 for g in a["grads"].values())
    # a dropped bias would move the log-probabilities far past the bound
    if K > 1:
        st = {k: torch.tensor(v, dtype=torch.float64) for k, v in lc.make_state(name).items()}
        st["conv4.bias"] = torch.zeros_like(st["conv4.bias"])
        with torch.no_grad():
            moved = lc.restate(st, torch.tensor(lc.make_inputs(name)[0], dtype=torch.float64))["logits"]
        assert lc.rel_err(moved, a["eval_logits"]) > 1e-3   # ten times the device bound


def test_case_sizes_follow_the_kernels_thresholds():
    lib = abd_amd.load_library()
    assert [lib.abd_largecnn_tile_info(i) for i in range(7)] == [lc.SMALL_TILE, lc.LARGE_TILE, lc.SLICE_ROWS,
                                                                 lc.COLSUM_ROWS, lc.LARGE_MIN_BLOCKS, lc.MAX_SLICES, -1]
    assert tile_info("slice_rows") == lc.SLICE_ROWS
    B, H, W, K, _ = lc.CASES["ragged_batch"]
    px2, px4 = B * (H // 2) * (W // 2), B * (H // 4) * (W // 4)
    for px in (px2, px4):
        assert px % lc.SMALL_TILE and px % lc.LARGE_TILE
    assert px2 // lc.SLICE_ROWS == 2 > ((B - 1) * 48) // lc.SLICE_ROWS     # conv2's weight gradient: two slices
    assert px2 > lc.COLSUM_ROWS >= (B - 1) * 48                            # conv1's / conv2's bias: two stages
    assert lc.CASES["tiny"][1:3] == (12, 12) and lc.linear_features(12, 12) == 256
    B, H, W, K, _ = lc.CASES["odd"]
    assert H % 2 and W % 2 and (W // 2) % 2                                # pool1 drops a row and a column, pool2 a column
    assert lc.CASES["jingleback"][1] % 2 and lc.linear_features(*lc.CASES["jingleback"][1:3]) == 12288
    assert lc.linear_features(*lc.CASES["flowmur"][1:3]) == 768 and (lc.CASES["flowmur"][2] // 4 - 3) // 2 + 1 == 1
    assert lc.linear_features(*lc.CASES["daba"][1:3]) == 3072
    # Which tile the kernels choose.  jingleback: every conv weight gradient runs the 128 x 128 tile (the pixel
    # gather in the B loader), over slices that are no multiple of the K-step; at B - 1 conv3..conv5 would not.
    # No case's forward or data gradient reaches the threshold (conv2's data gradient would need 96 x 128 pixels):
    # tests/test_gpu_largecnn.py::test_both_tiles_on_every_product sets the threshold instead.
    B, H, W, K, _ = lc.CASES["jingleback"]
    blocks = lc.large_blocks("jingleback")
    assert all(blocks[layer, "wgrad"] >= lc.LARGE_MIN_BLOCKS for layer in ("conv2", "conv3", "conv4", "conv5"))
    px4 = B * (H // 4) * (W // 4)
    assert lc.plan_slices(px4)[0] == 2 and px4 % lc.plan_slices(px4)[1] % 32
    assert 3 * 3 * 9 * lc.plan_slices((B - 1) * (H // 4) * (W // 4))[0] < lc.LARGE_MIN_BLOCKS
    for name in lc.CASES:
        assert all(v < lc.LARGE_MIN_BLOCKS for (layer, kind), v in lc.large_blocks(name).items() if kind != "wgrad")
        if name != "jingleback":
            assert all(v < lc.LARGE_MIN_BLOCKS for v in lc.large_blocks(name).values()), name
    assert lc.plan_slices(500) == (1, 512) and lc.plan_slices(528) == (2, 288) and lc.plan_slices(10 ** 6)[0] == 16


def test_float_split_is_exact_to_the_side_limit():
    """The weight-gradient loader splits a pixel's row / column with (int)((n + 0.5f) * (1.0f / side)) in float32.
    That equals n // side for every side the library accepts (up to 4096) and every numerator it forms
    (n < side + 32: a K-step's 32 pixels past the first one's column, or the row plus the wrapped columns)."""
    for side in range(1, 4097):
        n = np.arange(side + 64, dtype=np.int32)
        inv = np.float32(1.0) / np.float32(side)
        q = ((n.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)
        assert np.array_equal(q, n // side), side


@pytest.mark.parametrize("geo", lc.DIGEST_MODELS)
def test_seeded_init_and_state_dict_match_a_plain_build(geo):
    """utils/models.py:70-92 builds conv1, pool1, conv2, pool2, conv3..conv5, pool3, flat, fc1, dropout1, fc2,
    dropout2, fc3 in that order: the same construction order consumes torch's generator alike."""
    K, lf = geo
    torch.manual_seed(lc.DIGEST_SEED)
    m = largecnn(K, lf)
    torch.manual_seed(lc.DIGEST_SEED)
    layers = {n: nn.Conv2d(cin, cout, (3, 3), stride=1, padding=1) for n, cin, cout in lc.CONVS}
    layers.update(fc1=nn.Linear(lf, 256), fc2=nn.Linear(256, 128), fc3=nn.Linear(128, K))
    want = {f"{n}.{k}": v for n, layer in layers.items() for k, v in layer.state_dict().items()}
    sd = m.state_dict()
    assert list(sd) == list(want) == list(PARAM_ORDER) == list(lc.PARAM_ORDER)
    assert [n for n, _ in m.named_parameters()] == list(PARAM_ORDER)
    for k in sd:
        assert sd[k].shape == want[k].shape == lc.param_shapes(lf, K)[k] and torch.equal(sd[k], want[k]), k
    assert [n for n, _ in m.named_children()] == ["conv1", "pool1", "conv2", "pool2", "conv3", "conv4", "conv5",
                                                  "pool3", "flat", "fc1", "dropout1", "fc2", "dropout2", "fc3"]


def test_header_symbols_are_exported():
    with open(os.path.join(ROOT, "include", "abd.h")) as f:
        names = sorted(set(re.findall(r"\b(abd_largecnn_\w+)\s*\(", f.read())))
    assert len(names) == 13, names
    lib = abd_amd.load_library()
    for n in names:
        assert hasattr(lib, n), n
        assert n in L.EXPORTS, n
    assert C.sizeof(L.LargeCnnArgs) == 176   # abd_largecnn_args on LP64


def test_create_limits_offsets_and_workspace_names():
    lib = abd_amd.load_library()
    h = C.c_void_p()
    for geo in ((11, 40, 10), (40, 11, 10), (0, 40, 10), (4097, 40, 10), (4096, 4096, 10), (32, 13, 0), (32, 13, 4097)):
        assert lib.abd_largecnn_create(*geo, C.byref(h)) == 1002, geo
    assert b"32 bits" in lib.abd_last_error() or b"num_classes" in lib.abd_last_error()
    assert lib.abd_largecnn_create(4096, 4096, 10, C.byref(h)) == 1002 and b"32 bits" in lib.abd_last_error()
    for geo in ((12, 12, 1), (12, 4096, 10), (32, 13, 4096)):   # the limits
        assert lib.abd_largecnn_create(*geo, C.byref(h)) == 0, geo
        lib.abd_largecnn_destroy(h)
    for (H, W), lf in SCRIPT_GEOMETRIES:
        assert lib.abd_largecnn_linear_features(H, W) == lf == lc.linear_features(H, W) == linear_features(H, W)
        assert lib.abd_largecnn_create(H, W, 10, C.byref(h)) == 0
        offs = (C.c_int64 * 17)()
        assert lib.abd_largecnn_param_offsets(h, offs) == 0
        sizes = [int(np.prod(s)) for s in lc.param_shapes(lf, 10).values()]
        assert list(offs) == [0] + list(np.cumsum(sizes))
        assert lib.abd_largecnn_param_count(h) == sum(sizes) == sum(p.numel() for p in largecnn(10, lf).parameters())
        lib.abd_largecnn_destroy(h)
    assert lib.abd_largecnn_linear_features(11, 40) == -1 and lib.abd_largecnn_linear_features(40, 11) == -1
    assert lib.abd_largecnn_create(100, 40, 10, C.byref(h)) == 0
    assert 6.4e6 < lib.abd_largecnn_param_count(h) < 6.6e6
    names = ["a1", "p1", "a2", "p2", "a3", "a4", "a5", "p3", "h1", "h2", "logits", "dlogits", "rowinfo", "z3",
             "keep1", "keep2", "da2"]
    got = [lib.abd_largecnn_workspace_offset(h, 4, n.encode()) for n in names]
    assert all(o >= 0 for o in got) and len(set(got)) == len(got)
    assert lib.abd_largecnn_workspace_offset(h, 4, b"nope") == -1
    # the documented size: the seven saved maps and the gradient maps dominate
    need = lib.abd_largecnn_workspace_bytes(h, 256)
    maps = 4 * 256 * (4000 * 96 + 1000 * 96 + 1000 * 256 + 250 * (256 + 384 + 384 + 256))
    assert maps <= need < 2.0e9
    # a batch whose pixel rows leave 32 bits is refused before any launch
    a = L.LargeCnnArgs()
    a.x = a.params = a.grads = 16   # never dereferenced: the calls return before any launch
    a.batch = 1 << 20
    a.labels = 16
    assert lib.abd_largecnn_train_step(h, C.byref(a), None, 0, None) == 1001 and b"32-bit" in lib.abd_last_error()
    a.batch = 2
    a.labels = None
    assert lib.abd_largecnn_train_step(h, C.byref(a), None, 0, None) == 1001 and b"labels" in lib.abd_last_error()
    a.labels = 16
    a.do_update = 1
    assert lib.abd_largecnn_train_step(h, C.byref(a), None, 0, None) == 1001 and b"Adam" in lib.abd_last_error()
    a.do_update = 0
    assert lib.abd_largecnn_train_step(h, C.byref(a), None, 0, None) == 1003
    assert lib.abd_largecnn_forward(h, C.byref(a), 1, None, 0, None) == 1003
    assert lib.abd_largecnn_backward(h, C.byref(a), None, None, 0, None) == 1001
    assert lib.abd_largecnn_backward(h, C.byref(a), 16, None, 0, None) == 1003
    assert lib.abd_largecnn_eval(h, None, 2, 16, None, None, 16, None, None, 0, None) == 1001
    assert lib.abd_largecnn_eval(h, 16, 2, 16, None, None, 16, None, None, 0, None) == 1003
    assert lib.abd_largecnn_eval(h, 16, 2, 16, None, None, 16, None, 24, 1 << 40, None) == 1001   # misaligned
    assert lib.abd_largecnn_set_large_min_blocks(h, 0) == 1001 and lib.abd_largecnn_set_large_min_blocks(None, 1) == 1001
    assert lib.abd_largecnn_set_large_min_blocks(h, 1) == 0
    lib.abd_largecnn_destroy(h)


class Shaped(nn.Module):
    """A reference-shaped instance from torch.nn layers; ``edit`` changes one thing after the build."""

    def __init__(self, K=10, lf=768, edit=None):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 96, kernel_size=(3, 3), stride=1, padding=1)
        self.pool1 = nn.MaxPool2d(kernel_size=(2, 2))
        self.conv2 = nn.Conv2d(96, 256, kernel_size=(3, 3), stride=1, padding=1)
        self.pool2 = nn.MaxPool2d(kernel_size=(2, 2))
        self.conv3 = nn.Conv2d(256, 384, kernel_size=(3, 3), stride=1, padding=1)
        self.conv4 = nn.Conv2d(384, 384, kernel_size=(3, 3), stride=1, padding=1)
        self.conv5 = nn.Conv2d(384, 256, kernel_size=(3, 3), stride=1, padding=1)
        self.pool3 = nn.MaxPool2d(kernel_size=(3, 3), stride=(2, 2))
        self.flat = nn.Flatten()
        self.fc1 = nn.Linear(lf, 256)
        self.dropout1 = nn.Dropout(0.5)
        self.fc2 = nn.Linear(256, 128)
        self.dropout2 = nn.Dropout(0.5)
        self.fc3 = nn.Linear(128, K)
        if edit:
            edit(self)


Shaped.__name__ = Shaped.__qualname__ = "largecnn"


def test_training_accepts_the_model_and_adoption():
    assert largecnn in T.ACCELERATED
    for m in (largecnn(10, 768), Shaped()):
        ps = list(m.parameters())
        assert T.fusable(m, torch.optim.Adam(ps), nn.CrossEntropyLoss())
        assert not T.fusable(m, torch.optim.Adam(ps, weight_decay=0.1), nn.CrossEntropyLoss())
        assert not T.fusable(m, torch.optim.Adam(ps, amsgrad=True), nn.CrossEntropyLoss())
        assert not T.fusable(m, torch.optim.Adam(ps[:-1]), nn.CrossEntropyLoss())
        assert not T.fusable(m, torch.optim.SGD(ps, lr=0.1), nn.CrossEntropyLoss())
        assert not T.fusable(m, torch.optim.Adam(ps), nn.NLLLoss())
        assert not T.fusable(m, torch.optim.Adam(ps), nn.CrossEntropyLoss(label_smoothing=0.1))
        with pytest.raises(L.AbdError):   # SGD
            T.train(m, [], "cpu", torch.optim.SGD(ps, lr=0.1), nn.CrossEntropyLoss())
        with pytest.raises(L.AbdError):
            T.clean_train(m, [], "cpu", torch.optim.SGD(ps, lr=0.1), nn.CrossEntropyLoss())


def test_adopt_shares_the_modules_and_parameters():
    s = Shaped()
    ps = list(s.parameters())
    a = adopt(s)
    assert type(a) is largecnn and a is adopt(s) and adopt(a) is a
    assert [id(p) for p in a.parameters()] == [id(p) for p in ps]
    assert [n for n, _ in a.named_parameters()] == list(PARAM_ORDER)
    for n, child in s.named_children():
        assert getattr(a, n) is child, n
    assert "_engine" not in s.__dict__ and not hasattr(s, "gemm_precision")     # the instance is not touched
    assert a._engine is None and a.training == s.training
    assert T.accelerated(s) is a and T.accelerated(a) is a
    foreign = nn.Linear(4, 2)
    assert T.accelerated(foreign) is foreign
    # a replaced layer is seen: the cache does not hand out the old adoption
    s.fc3 = nn.Linear(128, 10)
    b = adopt(s)
    assert b is not a and b.fc3 is s.fc3


@pytest.mark.parametrize("edit", [
    lambda m: setattr(m, "conv3", nn.Conv2d(256, 384, kernel_size=(5, 5), stride=1, padding=2)),
    lambda m: setattr(m, "conv2", nn.Conv2d(96, 256, kernel_size=(3, 3), stride=1, padding=0)),
    lambda m: setattr(m, "conv4", nn.Conv2d(384, 384, kernel_size=(3, 3), stride=1, padding=1, bias=False)),
    lambda m: setattr(m, "conv5", nn.Conv2d(384, 128, kernel_size=(3, 3), stride=1, padding=1)),
    lambda m: setattr(m, "pool3", nn.MaxPool2d(kernel_size=(3, 3))),
    lambda m: setattr(m, "pool1", nn.MaxPool2d(kernel_size=(2, 2), ceil_mode=True)),
    lambda m: setattr(m, "pool2", nn.AvgPool2d(kernel_size=(2, 2))),
    lambda m: delattr(m, "conv4"),
    lambda m: delattr(m, "pool2"),
    lambda m: setattr(m, "fc1", nn.Linear(700, 256)),
    lambda m: setattr(m, "fc2", nn.Linear(256, 64)),
    lambda m: setattr(m, "dropout1", nn.Dropout(0.4)),
    lambda m: setattr(m, "bn", nn.BatchNorm2d(96)),
    lambda m: m.double(),
])
def test_adopt_refuses_another_structure(edit):
    s = Shaped(edit=edit)
    with pytest.raises(L.AbdError):
        adopt(s)
    with pytest.raises(L.AbdError):
        T.train(s, [], "cpu", torch.optim.Adam(s.parameters()), nn.CrossEntropyLoss())
    with pytest.raises(L.AbdError):
        T.clean_test(s, "cpu", [], nn.CrossEntropyLoss())


def test_adopt_refuses_other_names():
    class Other(nn.Module):
        pass

    with pytest.raises(L.AbdError):
        adopt(Other())
    with pytest.raises(L.AbdError):
        adopt(nn.Linear(2, 2))


class _FakeDevice(torch.Tensor):
    """A CPU tensor that claims to live on the device: gets past require_device, so the refusal under test
    is the one that fires (nothing is launched before it)."""
    is_cuda = True


def test_cpu_tensors_bf16_and_geometry_are_refused():
    m = largecnn(10, 768)
    with pytest.raises(L.AbdError):
        m(torch.zeros(2, 1, 32, 13))
    with pytest.raises(L.AbdError):
        T.largecnn_train_step(m, torch.zeros(2, 1, 32, 13), torch.zeros(2, dtype=torch.int64), None, None, None)
    with pytest.raises(ValueError):
        m(torch.zeros(2, 32, 13).as_subclass(_FakeDevice))
    with pytest.raises(ValueError):   # (32, 40) gives 3072 features, the model has 768
        m(torch.zeros((2, 1, 32, 40)).as_subclass(_FakeDevice))
    with pytest.raises(ValueError):   # below 12 x 12
        m(torch.zeros((2, 1, 11, 13)).as_subclass(_FakeDevice))
    with pytest.raises(L.AbdError):
        m.set_gemm_precision("bf16")
    with pytest.raises(ValueError):
        m.set_gemm_precision("fp8")
    assert m.set_gemm_precision("f32") is m
    with pytest.raises(ValueError):
        m.set_dropout_source("nowhere")
    torch.manual_seed(0)
    m1, m2 = m.set_dropout_source("torch_cpu").step_masks(5, "cpu")
    assert m1.shape == (5, 256) and m2.shape == (5, 128) and m1.dtype == torch.uint8
    assert m.set_dropout_source("device").step_masks(5, "cpu") is None


def test_smallcnn_only_paths_refuse_the_model():
    """Data parallelism / SyncBN (ResidentTrainer, training.train_step), SGD fine-tuning, FlowMur, DABA and every
    defence entry point refuse largecnn -- this package's class and a reference-shaped instance -- with AbdError,
    also once an engine is bound, when the flat buffers exist."""
    from abd_amd import daba, defense as D, flowmur, pipeline as P

    class Eng:   # what a bound engine looks like to the duck-typed smallcnn paths
        device = torch.device("cpu")
        params = torch.zeros(4)
        running = torch.zeros(22)

    for make in (lambda: largecnn(10, 768), Shaped):
        for bound in (False, True):
            m = make()
            if bound:
                object.__setattr__(m, "_engine", Eng())
                object.__setattr__(m, "_bound", lambda eng: True)
            opt = torch.optim.Adam(m.parameters())
            x = torch.zeros((4, 1, 32, 13)).as_subclass(_FakeDevice)
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
                "flowmur_as_smallcnn": lambda: flowmur._as_abd_smallcnn(m),
                "flowmur_trigger": lambda: flowmur.TriggerOptimizer(m.eval(), 4000),
                "daba_entropy": lambda: daba.one_sotamax_entropy("largecnn", m, "nowhere.wav"),
                "daba_require": lambda: daba._require_cnn("largecnn", m),
            }
            for what, call in calls.items():
                with pytest.raises(L.AbdError):
                    call()
                    pytest.fail(f"{what} (bound={bound}) did not refuse {type(m).__module__}.largecnn")


def test_checkpoint_is_a_reference_pickle(tmp_path):
    torch.manual_seed(3)
    m = largecnn(10, 768)
    p = tmp_path / "ckpt.pt"
    T.save_reference_checkpoint(m, str(p))
    import zipfile
    with zipfile.ZipFile(p) as z:
        data = z.read([n for n in z.namelist() if n.endswith("data.pkl")][0])
    ops = [(o.name, a) for o, a, _ in pickletools.genops(io.BytesIO(data))]
    assert "utils.models largecnn" in [a for n, a in ops if n == "GLOBAL"]
    assert not any("abd_amd" in str(a) for _, a in ops if a is not None)
    state = T.reference_module_state(m)
    plain = nn.Module()
    plain.__dict__.update(state)
    assert list(plain.state_dict().keys()) == list(m.state_dict().keys())
    for k, v in m.state_dict().items():
        assert torch.equal(plain.state_dict()[k], v), k
    assert isinstance(plain.pool3, nn.MaxPool2d) and isinstance(plain.dropout2, nn.Dropout)
    assert "_engine" not in state and "gemm_precision" not in state and "_step" not in state


def test_getstate_drops_the_engine():
    m = largecnn(10, 768)
    m._engine = object()
    st = m.__getstate__()
    assert st["_engine"] is None
    n = largecnn.__new__(largecnn)
    n.__setstate__({k: v for k, v in st.items() if k not in ("_engine", "gemm_precision", "_step")})
    assert n._engine is None and n.gemm_precision == "f32" and n._step == 0 and n.dropout_source == "device"
