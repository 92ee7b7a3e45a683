"""GPU: largecnn on libabd against the float64 restatement of tests/largecnn_cases.py.

Bounds: 1e-4 relative to the largest magnitude of the compared tensor (the project's fp32 bound; the float32 CPU
run of the restatement stays within 1e-5, tests/test_largecnn_cpu.py), counters exact.  Measured distances are
printed before each assertion (profiles/largecnn/parity.md records them).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.utils.data as Data

import abd_amd
from abd_amd import _lib as L, training as T
from abd_amd.models_largecnn import largecnn, adopt, tile_info
import largecnn_cases as lc

pytestmark = pytest.mark.gpu
GUARD = 8 << 20
PAT = 0xA5
CASES = list(lc.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    # the cases are sized from the built kernels' tiles and thresholds
    assert [tile_info(k) for k in ("small_tile", "large_tile", "slice_rows", "colsum_rows", "large_min_blocks",
                                   "max_slices")] == [lc.SMALL_TILE, lc.LARGE_TILE, lc.SLICE_ROWS, lc.COLSUM_ROWS,
                                                      lc.LARGE_MIN_BLOCKS, lc.MAX_SLICES]
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref():
    """The float64 reference of a case, built once per module and shared read-only."""
    return lambda name: lc.run_case(name, torch.float64)


def build(name, dev):
    B, H, W, K, _ = lc.CASES[name]
    m = largecnn(K, lc.linear_features(H, W))
    m.load_state_dict({k: torch.tensor(v) for k, v in lc.make_state(name).items()})
    return m.to(dev)


class Reference(nn.Module):
    """A module of the reference's shape (utils/models.py:68-119), from torch.nn layers: what a script holds."""

    def __init__(self, num_classes, linear_features):
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
        self.fc1 = nn.Linear(linear_features, 256)
        self.dropout1 = nn.Dropout(0.5)
        self.fc2 = nn.Linear(256, 128)
        self.dropout2 = nn.Dropout(0.5)
        self.fc3 = nn.Linear(128, num_classes)

    def forward(self, x):
        x = self.pool2(self.conv2(self.pool1(self.conv1(x))))
        x = torch.relu(self.conv5(torch.relu(self.conv4(torch.relu(self.conv3(x))))))
        x = self.flat(self.pool3(x))
        x = self.dropout1(torch.relu(self.fc1(x)))
        x = self.dropout2(torch.relu(self.fc2(x)))
        return torch.log_softmax(self.fc3(x), dim=1)


# what a script holds is utils.models.largecnn: a class of that name in a module of its own, so that it pickles
import sys    # noqa: E402
import types  # noqa: E402
_SCRIPT_MODELS = types.ModuleType("largecnn_script_models")
Reference.__module__ = _SCRIPT_MODELS.__name__
Reference.__name__ = Reference.__qualname__ = "largecnn"
_SCRIPT_MODELS.largecnn = Reference
sys.modules[_SCRIPT_MODELS.__name__] = _SCRIPT_MODELS


def inputs(name, dev):
    x, y, ind, m1, m2 = lc.make_inputs(name)
    t = lambda a: torch.tensor(a, device=dev)   # noqa: E731
    return t(x), t(y), t(ind), (t(m1), t(m2))


def load_reference_checkpoint(path, dev):
    """torch.load a reference-format checkpoint (a pickle of ``utils.models.largecnn``) with that name bound to
    this package's class, as a script that imports it under that name would.  sys.modules is restored."""
    import sys
    import types
    um = types.ModuleType("utils.models")
    um.largecnn = largecnn
    pkg = types.ModuleType("utils")
    pkg.models = um
    old = {k: sys.modules.get(k) for k in ("utils", "utils.models")}
    sys.modules.update({"utils": pkg, "utils.models": um})
    try:
        return torch.load(path, map_location=dev, weights_only=False)   # a file this suite wrote
    finally:
        for k, v in old.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def metrics_buf(dev):
    return torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)


def counters(logits, y, ind):
    pred = logits.argmax(1)
    return (len(y), int((pred == y).sum()), int((ind == 1).sum()), int(((ind == 1) & (pred == y)).sum()), 1)


def check(what, got, want, tol=1e-4):
    e = lc.rel_err(got.detach().cpu(), want)
    print(f"{what}: {e:.3e}")
    assert e < tol, (what, e)


def close_loss(what, got, want):
    want = float(want)
    e = abs(got - want) / want if want > 0 else abs(got - want)
    print(f"{what}: {e:.3e}")
    assert e < 1e-4, (what, got, want)


def saved(m, B, name, n):
    eng = m._engine
    off = L.lib().abd_largecnn_workspace_offset(eng.h, B, name.encode())
    assert off >= 0
    return eng._ws[off:off + 4 * n].view(torch.float32).clone()


@pytest.mark.parametrize("name", CASES)
def test_eval_parity_and_counters(dev, ref, name):
    B, H, W, K, _ = lc.CASES[name]
    r = ref(name)
    x, y, ind, masks = inputs(name, dev)
    m = build(name, dev).eval()
    with torch.no_grad():
        ev = m(x)
    check(f"{name} eval log-probs", ev, r["eval_logits"])
    eng = m._engine
    mt = metrics_buf(dev)
    ev2 = torch.ops.abd.largecnn_eval_metrics(x, eng.params, K, y, ind, mt)
    assert torch.equal(ev2, ev)
    loss, *cnt = T.read_metrics(mt)
    close_loss(f"{name} eval loss", loss, r["eval_loss"])
    assert tuple(cnt) == counters(r["eval_logits"], y.cpu(), ind.cpu())


@pytest.mark.parametrize("name", CASES)
def test_train_forward_activations_gradients_and_determinism(dev, ref, name):
    B, H, W, K, _ = lc.CASES[name]
    r = ref(name)
    x, y, ind, masks = inputs(name, dev)
    m = build(name, dev).train()
    out = m.hip_forward(x, train=True, masks=masks)
    check(f"{name} train log-probs", out, r["acts"]["logits"])
    for an in lc.ACTIVATIONS:
        want = r["acts"][an]
        got = saved(m, B, an, want.numel())
        if want.dim() == 4 and an != "p3":   # p3 is kept in the reference's flatten order
            got = lc.channels_first(got, want.shape)
        check(f"{name} {an}", got, want)
    mt = metrics_buf(dev)
    lp = torch.empty((B, K), device=dev)
    T.largecnn_train_step(m, x, y, ind, None, mt, masks=masks, do_update=False, logits_out=lp)
    assert torch.equal(lp, out)
    loss, *cnt = T.read_metrics(mt)
    close_loss(f"{name} train loss", loss, r["loss"])
    assert tuple(cnt) == counters(r["acts"]["logits"], y.cpu(), ind.cpu())
    eng = m._engine
    g_step = eng.grads.clone()
    for n, g in zip(lc.PARAM_ORDER, eng.views(g_step)):
        check(f"{name} grad {n}", g, r["grads"][n], lc.bound(name, n))
    if K == 1:
        assert float(g_step.abs().max()) == 0.0
    H2, W2 = H // 2, W // 2
    da2 = saved(m, B, "da2", B * H2 * W2 * 256).view(B, H2, W2, 256)
    if K > 1:
        assert float(da2.abs().max()) > 0.0
    # the trailing row / column pool2 drops gets exactly zero gradient (odd: W2 = 7; jingleback: none dropped)
    assert float(da2[:, 2 * (H2 // 2):].abs().sum()) == 0.0 and float(da2[:, :, 2 * (W2 // 2):].abs().sum()) == 0.0
    # so does every position that is not its window's maximum: one survivor per window and channel at the most
    live = (da2[:, :2 * (H2 // 2), :2 * (W2 // 2)] != 0).view(B, H2 // 2, 2, W2 // 2, 2, 256).sum((2, 4))
    assert int(live.max()) <= 1
    # the same step twice: bit-equal
    T.largecnn_train_step(m, x, y, ind, None, None, masks=masks, do_update=False)
    assert torch.equal(eng.grads, g_step)


@pytest.mark.parametrize("name", ["odd", "flowmur", "ragged_batch", "jingleback"])
@pytest.mark.parametrize("min_blocks", [1, 2 ** 31 - 1], ids=["large_tile", "small_tile"])
def test_both_tiles_on_every_product(dev, ref, name, min_blocks):
    """launch_gemm picks the 128 x 128 tile from LARGE_MIN_BLOCKS blocks up, which at test sizes only jingleback's
    weight gradients reach.  With the threshold set on the engine's handle every product of the step -- the conv
    forward and data gradient (the pixel gather in the A loader, 16 rows per thread), the weight gradients (the
    gather in the B loader at 128 columns) and the head -- runs one tile, then the other: activations and all 16
    gradients against float64, each with ragged M."""
    B, H, W, K, _ = lc.CASES[name]
    r = ref(name)
    x, y, ind, masks = inputs(name, dev)
    m = build(name, dev).train()
    eng = m.engine(x)
    eng.call("set_large_min_blocks", min_blocks)
    out = torch.empty((B, K), device=dev)
    T.largecnn_train_step(m, x, y, ind, None, None, masks=masks, do_update=False, logits_out=out)
    check(f"{name} {min_blocks} train log-probs", out, r["acts"]["logits"])
    for an in ("a2", "a3", "a4", "a5", "h1", "h2"):
        want = r["acts"][an]
        got = saved(m, B, an, want.numel())
        check(f"{name} {min_blocks} {an}", lc.channels_first(got, want.shape) if want.dim() == 4 else got, want)
    for n, g in zip(lc.PARAM_ORDER, eng.views(eng.grads)):
        check(f"{name} {min_blocks} grad {n}", g, r["grads"][n], lc.bound(name, n))


@pytest.mark.parametrize("name", ["tiny", "odd", "flowmur", "ragged_batch", "k35"])
def test_autograd_path_bit_equal_to_train_step(dev, ref, name):
    """forward, torch's CrossEntropyLoss on the log-probabilities, abd_largecnn_backward: within the bound of
    float64 and bit-equal to abd_largecnn_train_step."""
    B, H, W, K, _ = lc.CASES[name]
    r = ref(name)
    x, y, ind, masks = inputs(name, dev)
    m2 = build(name, dev).train()
    m2.engine(x)
    m2.step_masks = lambda batch, device: masks
    nn.CrossEntropyLoss()(m2(x), y).backward()
    m3 = build(name, dev).train()
    T.largecnn_train_step(m3, x, y, ind, None, None, masks=masks, do_update=False)
    for n, p, s in zip(lc.PARAM_ORDER, m2._param_list(), m3._engine.views(m3._engine.grads)):
        check(f"{name} backward grad {n}", p.grad, r["grads"][n], lc.bound(name, n))
        assert torch.equal(p.grad.reshape(-1), s), n


def test_backward_must_follow_its_forward(dev):
    x, y, ind, masks = inputs("tiny", dev)
    m = build("tiny", dev).train()
    a, b = m(x), m(x)
    with pytest.raises(L.AbdError):
        a.sum().backward()
    b.sum().backward()
    c = m(x)
    T.largecnn_train_step(m, x, y, ind, None, None, do_update=False)   # the step overwrites the workspace
    with pytest.raises(L.AbdError):
        c.sum().backward()


@pytest.mark.parametrize("name", ["tiny", "ragged_batch"])
def test_fused_adam_equals_split_update(dev, name):
    x, y, ind, masks = inputs(name, dev)
    ms = [build(name, dev).train() for _ in range(2)]
    opts = [torch.optim.Adam(m.parameters(), lr=lc.LR) for m in ms]
    adams = []
    for m, o in zip(ms, opts):
        m.engine(x)
        adams.append(T.AdamBinding(m, o))
    T.largecnn_train_step(ms[0], x, y, ind, adams[0], None, masks=masks, do_update=True)
    T.largecnn_train_step(ms[1], x, y, ind, adams[1], None, masks=masks, do_update=False)
    T.apply_adam(ms[1], adams[1], dev)
    a, b = ms
    assert torch.equal(a._engine.params, b._engine.params)
    assert torch.equal(a._engine.exp_avg, b._engine.exp_avg)
    assert torch.equal(a._engine.exp_avg_sq, b._engine.exp_avg_sq)
    start = torch.cat([torch.tensor(lc.make_state(name)[n]).reshape(-1) for n in lc.PARAM_ORDER]).to(dev)
    moved = (a._engine.params - start).abs()
    assert float(moved.max()) <= lc.LR * (1 + 1e-3)
    for n, v in zip(lc.PARAM_ORDER, a._engine.views(moved)):
        assert float(v.max()) > 0.0, n


class DictSet(Data.Dataset):
    def __init__(self, x, y, ind):
        self.x, self.y, self.ind = x, y, ind

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return {"mfcc": self.x[i], "label": self.y[i], "poison_indicator": self.ind[i]}


def _loaders(name):
    xn, yn, indn, _, _ = lc.make_inputs(name)
    xc, yc, ic = torch.tensor(xn), torch.tensor(yn), torch.tensor(indn)
    ic[0] = 1
    bd = Data.DataLoader(DictSet(xc, yc, ic), batch_size=7, shuffle=False)     # batches of 7 and 4
    clean = Data.DataLoader(Data.TensorDataset(xc, yc), batch_size=7, shuffle=False)
    return xc, yc, ic, bd, clean


def test_training_loop_equals_manual_loop(dev):
    name = "ragged_batch"
    B, H, W, K, _ = lc.CASES[name]
    assert B == 11
    xc, yc, ic, bd, clean = _loaders(name)
    crit = nn.CrossEntropyLoss()
    a, b = build(name, dev), build(name, dev)
    oa = torch.optim.Adam(a.parameters(), lr=lc.LR)
    ob = torch.optim.Adam(b.parameters(), lr=lc.LR)
    torch.manual_seed(5)
    got = T.train(a, bd, dev, oa, crit)
    b.train()
    b._dropout_nonce = a._dropout_nonce   # the same dropout stream
    mt = metrics_buf(dev)
    adam = None
    for item in bd:
        x, y, ind = item["mfcc"].to(dev), item["label"].to(dev), item["poison_indicator"].to(dev)
        if adam is None:
            b.engine(x)
            adam = T.AdamBinding(b, ob)
        T.largecnn_train_step(b, x, y, ind, adam, mt)
    ls, tot, cor, pt, asr, nb = T.read_metrics(mt)
    assert got == (ls / nb, 100.0 * cor / tot, 100 * asr / pt)
    assert torch.equal(a._engine.params, b._engine.params)
    for p in a.parameters():
        assert float(oa.state[p]["step"]) == 2.0
        assert p.grad is not None and p.grad.shape == p.shape
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in a._param_list()]), a._engine.grads)
    got_t = T.test(a, dev, clean, bd, crit)
    eng = b._engine
    mc, mb = metrics_buf(dev), metrics_buf(dev)
    for lo, hi in ((0, 7), (7, B)):
        x, y, ind = xc[lo:hi].to(dev), yc[lo:hi].to(dev), ic[lo:hi].to(dev)
        torch.ops.abd.largecnn_eval_metrics(x, eng.params, K, y, None, mc)
        torch.ops.abd.largecnn_eval_metrics(x, eng.params, K, y, ind, mb)
    cl, ct, cc, _, _, nc = T.read_metrics(mc)
    bl, _, _, pt, ah, nbb = T.read_metrics(mb)
    assert got_t == (100 * cc / ct, 100 * ah / pt, cl / nc, bl / nbb)
    assert T.clean_test(a, dev, clean, crit) == (cl / nc, 100 * cc / ct)
    got_c = T.clean_train(a, clean, dev, oa, crit)
    mt = metrics_buf(dev)
    b.train()
    for xb, yb in clean:
        T.largecnn_train_step(b, xb.to(dev), yb.to(dev), None, adam, mt)
    ls, tot, cor, _, _, nb = T.read_metrics(mt)
    assert got_c == (ls / nb, 100.0 * cor / tot)
    assert torch.equal(a._engine.params, b._engine.params)
    with pytest.raises(L.AbdError):   # SGD is not the fused step's optimizer
        T.train(a, bd, dev, torch.optim.SGD(a.parameters(), lr=0.1), crit)


def test_adopted_instance_trains_like_the_native_class(dev, tmp_path):
    """A reference-shaped instance handed to train(): the script's own Parameter objects are re-homed, its
    optimizer's state is keyed by them, its own forward sees the trained weights, and the result is bit-equal to
    the native class from the same state and dropout stream."""
    name = "ragged_batch"
    B, H, W, K, _ = lc.CASES[name]
    xc, yc, ic, bd, clean = _loaders(name)
    crit = nn.CrossEntropyLoss()
    script = Reference(K, lc.linear_features(H, W))
    script.load_state_dict({k: torch.tensor(v) for k, v in lc.make_state(name).items()})
    script.to(dev)
    held = list(script.parameters())
    opt = torch.optim.Adam(script.parameters(), lr=lc.LR)
    native = build(name, dev)
    on = torch.optim.Adam(native.parameters(), lr=lc.LR)
    torch.manual_seed(5)
    got_n = T.train(native, bd, dev, on, crit)
    torch.manual_seed(5)
    adopt(script).set_dropout_source("device")
    adopt(script)._dropout_nonce = native._dropout_nonce
    got_s = T.train(script, bd, dev, opt, crit)
    assert got_s == got_n
    ad = adopt(script)
    assert ad is adopt(script) and not hasattr(script, "_engine")
    assert torch.equal(ad._engine.params, native._engine.params)
    assert [id(p) for p in script.parameters()] == [id(p) for p in held]
    assert set(opt.state.keys()) == set(held) and all(float(opt.state[p]["step"]) == 2.0 for p in held)
    for p, q in zip(script.parameters(), native.parameters()):
        assert torch.equal(p, q) and p.grad is not None
    assert T.test(script, dev, clean, bd, crit) == T.test(native, dev, clean, bd, crit)
    # the script's own eager forward runs on the trained weights
    script.eval()
    with torch.no_grad():
        own = script(xc[:4].to(dev))
        ours = ad.eval()(xc[:4].to(dev))
    check("adopted eager forward", ours, own.double().cpu())
    # EarlyStoppingModel saves such an instance as it saves any reference module: the module itself, although its
    # parameters are views of the flat buffer now
    stop = T.EarlyStoppingModel(path=str(tmp_path / "checkpoint.pt"))
    stop(1.0, script)
    back = torch.load(str(tmp_path / "checkpoint.pt"), map_location=dev, weights_only=False)
    assert type(back) is Reference and not isinstance(back, largecnn)
    sd, bsd = script.state_dict(), back.state_dict()
    assert list(bsd) == list(sd) and all(torch.equal(bsd[k], sd[k]) for k in sd)
    lo = ad._engine.params.data_ptr()
    assert all(not lo <= p.data_ptr() < lo + 4 * ad._engine.n for p in back.parameters())   # no alias of the live buffer
    back.eval()
    with torch.no_grad():
        again = back(xc[:4].to(dev))
    # equal weights (above, bit for bit); the vendor convolutions of two eager forwards need not round alike
    check("reloaded eager forward", again, own.double().cpu())
    script.train()
    T.train(script, bd, dev, opt, crit)                         # the saved script object trains on
    assert script.training and ad.training and ad._bound(ad._engine)
    T.clean_test(script, dev, clean, crit)
    assert not script.training and not ad.training


def test_guards_and_refusals(dev):
    name = "tiny"
    B, H, W, K, _ = lc.CASES[name]
    x, y, ind, masks = inputs(name, dev)
    m = build(name, dev).train()
    eng = m.engine(x)
    need = L.lib().abd_largecnn_workspace_bytes(eng.h, B)
    eng._ws = torch.full((need + GUARD,), PAT, dtype=torch.uint8, device=dev)[:need + GUARD]
    ws = eng._ws
    out = torch.full((B + 4, K), float("nan"), device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=lc.LR)
    adam = T.AdamBinding(m, opt)
    a = m._args(eng, x, B)
    a.labels, a.indicators = y.data_ptr(), ind.data_ptr()
    a.logits_out = out.data_ptr()
    a.exp_avg, a.exp_avg_sq = eng.exp_avg.data_ptr(), eng.exp_avg_sq.data_ptr()
    a.lr, a.beta1, a.beta2, a.eps, a.adam_step, a.do_update = adam.lr, 0.9, 0.999, 1e-8, 1, 1
    assert L.lib().abd_largecnn_train_step(eng.h, C.byref(a), ws.data_ptr(), need, L.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert int((ws[need:] != PAT).sum()) == 0
    assert torch.isnan(out[B:]).all() and torch.isfinite(out[:B]).all()
    assert L.lib().abd_largecnn_train_step(eng.h, C.byref(a), ws.data_ptr(), need - 1, None) == 1003
    assert L.lib().abd_largecnn_forward(eng.h, C.byref(a), 1, ws.data_ptr(), 16, None) == 1003
    with pytest.raises(L.AbdError):
        T.largecnn_train_step(m, x, None, None, None, None)   # no labels
    with pytest.raises(L.AbdError):
        m(x.cpu())
    with pytest.raises(ValueError):
        m(x[..., :-4].contiguous())   # 12 x 8: another linear_features


def test_device_dropout_masks(dev):
    """Without handed-in masks the keep-masks come from the hash: about half kept, reported through mask_out,
    reproducible for equal (seed, counter) and different for the next counter."""
    name = "flowmur"
    B, H, W, K, _ = lc.CASES[name]
    x, y, ind, _ = inputs(name, dev)
    m = build(name, dev).train()
    outs = []
    for counter in (0, 0, 1):
        mo = (torch.zeros((B, 256), dtype=torch.uint8, device=dev), torch.zeros((B, 128), dtype=torch.uint8, device=dev))
        m._step = counter
        lp = m.hip_forward(x, train=True, seed=77, masks_out=mo)
        outs.append((lp, mo))
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert not torch.equal(outs[0][1][0], outs[2][1][0])
    for mk in outs[0][1]:
        assert 0.35 < float(mk.float().mean()) < 0.65 and int(mk.max()) == 1
    again = m.hip_forward(x, train=True, masks=outs[0][1])
    assert torch.equal(again, outs[0][0])


def test_opcheck(dev):
    name = "tiny"
    B, H, W, K, _ = lc.CASES[name]
    x, y, ind, masks = inputs(name, dev)
    m = build(name, dev)
    eng = m.engine(x)
    eng.exp_avg = torch.zeros_like(eng.params)
    eng.exp_avg_sq = torch.zeros_like(eng.params)
    torch.library.opcheck(torch.ops.abd.largecnn_eval.default, (x, eng.params, K))
    mt = metrics_buf(dev)
    torch.library.opcheck(torch.ops.abd.largecnn_eval_metrics.default, (x, eng.params, K, y, ind, mt))
    args = (x, y, ind, eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq, mt, K, 1, 1e-4, 0.9, 0.999, 1e-8, 3, 0,
            masks[0], masks[1])
    torch.library.opcheck(torch.ops.abd.largecnn_train_step.default, args)


def test_bound_model_checkpoint_reloads(dev, tmp_path):
    """After engine() the parameters are views of the flat buffer: the reference-format checkpoint of such a
    model, and torch.save of the module itself, reload to the same state and the same log-probabilities."""
    name = "tiny"
    x, y, ind, masks = inputs(name, dev)
    m = build(name, dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=lc.LR)
    m.engine(x)
    T.largecnn_train_step(m, x, y, ind, T.AdamBinding(m, opt), None, masks=masks)   # bound, trained one step
    assert m._bound(m._engine)
    m.eval()
    with torch.no_grad():
        want = m(x)
    T.save_reference_checkpoint(m, str(tmp_path / "ref.pt"))
    torch.save(m, str(tmp_path / "whole.pt"))
    whole = torch.load(str(tmp_path / "whole.pt"), map_location=dev, weights_only=False)
    assert type(whole) is largecnn and whole._engine is None
    back = load_reference_checkpoint(str(tmp_path / "ref.pt"), dev)
    sd = m.state_dict()
    for b in (whole, back):
        assert type(b).__name__ == "largecnn" and b._engine is None
        bsd = b.state_dict()
        assert list(bsd) == list(sd) and all(torch.equal(bsd[k], sd[k]) for k in sd)
        lo = m._engine.params.data_ptr()
        hi = lo + 4 * m._engine.n
        assert all(p.is_contiguous() and not lo <= p.data_ptr() < hi for p in b.parameters())   # no alias of m
        b.eval()
        with torch.no_grad():
            assert torch.equal(b(x), want)
    assert m._bound(m._engine)   # saving left the model bound


SCRIPT = r'''
import json, sys
import torch, torch.nn as nn, torch.optim as optim, torch.utils.data as Data
from prepare_dataset import BDDataset
from utils.random_tools import fix_random
from utils.training_tools import train, test, EarlyStoppingModel
from abd_amd.models_largecnn import largecnn     # route one: this package's class

fix_random()
model = largecnn(10, 768)                        # flowmur.py's geometry: (32, 13) inputs
device = torch.device("cuda")
model.to(device)
criterion = nn.CrossEntropyLoss()
optimizer = optim.Adam(model.parameters(), lr=1e-4)
g = torch.Generator().manual_seed(1)
y = torch.randint(0, 10, (96,), generator=g)
x = torch.randn((96, 1, 32, 13), generator=g) + 0.5 * y[:, None, None, None].float()   # label-dependent level
ind = (torch.arange(96) % 10 == 0).long()
bd_train = Data.DataLoader(BDDataset(x, y, ind), batch_size=40, shuffle=True)
clean_test = Data.DataLoader(Data.TensorDataset(x, y), batch_size=40, shuffle=True)
bd_test = Data.DataLoader(BDDataset(x, y, ind), batch_size=40, shuffle=True)
stop = EarlyStoppingModel(patience=20, verbose=False, path="checkpoint.pt")
hist = []
for epoch in range(4):
    tr = train(model=model, train_loader=bd_train, device=device, optimizer=optimizer, criterion=criterion)
    te = test(model=model, device=device, clean_test_loader=clean_test, bd_test_loader=bd_test, criterion=criterion)
    stop(0.5 * (te[2] + te[3]), model=model)
    hist.append([*tr, *te])
model.eval()
with torch.no_grad():
    out = model(x[:8].to(device)).cpu()
torch.save({"out": out, "sd": {k: v.cpu() for k, v in model.state_dict().items()}}, "final.pt")
json.dump({"hist": hist, "cls": type(model).__module__}, open(sys.argv[1], "w"))
'''


def test_attack_script_shape_runs_through_the_dropin(dev, tmp_path):
    """An attack-script-shaped run (train / test / EarlyStoppingModel from utils.training_tools, the model from
    abd_amd.models_largecnn) under ``python -m abd_amd.run`` trains through libabd, and its checkpoint reloads."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (tmp_path / "flowmur_like.py").write_text(SCRIPT)
    out = tmp_path / "res.json"
    r = subprocess.run([sys.executable, "-m", "abd_amd.run", "flowmur_like.py", str(out)], cwd=tmp_path,
                       env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(out.read_text())
    assert res["cls"] == "abd_amd.models_largecnn"
    h = np.array(res["hist"])
    assert np.all(np.isfinite(h)) and h[-1, 0] < h[0, 0]          # the train loss falls
    final = torch.load(str(tmp_path / "final.pt"), weights_only=True)
    ck = load_reference_checkpoint(str(tmp_path / "checkpoint.pt"), dev)
    assert type(ck).__name__ == "largecnn"
    assert list(ck.state_dict()) == list(final["sd"])
    ck.eval()
    with torch.no_grad():
        yv = ck(torch.zeros((2, 1, 32, 13), device=dev))
    assert yv.shape == (2, 10) and torch.isfinite(yv).all() and torch.isfinite(final["out"]).all()
