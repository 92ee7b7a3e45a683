"""GPU: ResNet on libabd against the float64 restatement of tests/resnet_cases.py.

Bound: 1e-4 absolute on every tensor (resnet_cases.bound; the float32 CPU run of the restatement stays within
6.3e-5 on every case, tests/test_resnet_cpu.py), counters exact.  Measured distances are printed before each
assertion (profiles/resnet/parity.md records them).
"""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.utils.data as Data

import abd_amd
from abd_amd import _lib as L, training as T
from abd_amd.models_resnet import ResNet, ResidualBlock, adopt, tile_info
import resnet_cases as rc

pytestmark = pytest.mark.gpu
GUARD = 8 << 20
PAT = 0xA5
CASES = list(rc.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    # the cases are sized from the built kernels' tiles and thresholds
    assert [tile_info(k) for k in ("tile_rows", "k_step", "slice_rows", "max_slices", "stat_rows", "stat_blocks")] == [
        rc.TILE_ROWS, rc.K_STEP, rc.SLICE_ROWS, rc.MAX_SLICES, rc.STAT_ROWS, rc.STAT_BLOCKS]
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref():
    """The float64 reference of a case, built once per module and shared read-only."""
    return lambda name: rc.run_case(name, torch.float64)


def conv3x3(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False)


class RefBlock(nn.Module):
    def __init__(self, cin, cout, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(cin, cout, stride)
        self.bn1 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(cout, cout)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = downsample

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        out = out + (self.downsample(x) if self.downsample else x)
        return self.relu(out)


class Reference(nn.Module):
    """A module of the reference's shape (utils/models.py:289-332), from torch.nn layers: what a script holds."""

    def __init__(self, num_classes, linear_features):
        super().__init__()
        self.conv = conv3x3(1, 16)
        self.bn = nn.BatchNorm2d(16)
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = nn.Sequential(RefBlock(16, 16), RefBlock(16, 16))
        self.layer2 = nn.Sequential(
            RefBlock(16, 32, 2, nn.Sequential(conv3x3(16, 32, 2), nn.BatchNorm2d(32))), RefBlock(32, 32))
        self.layer3 = nn.Sequential(
            RefBlock(32, 64, 2, nn.Sequential(conv3x3(32, 64, 2), nn.BatchNorm2d(64))), RefBlock(64, 64))
        self.conv2d = nn.Conv2d(64, 64, kernel_size=(1, 1), stride=(2, 1))
        self.avg_pool = nn.AvgPool2d(4)
        self.fc = nn.Linear(linear_features, num_classes)

    def forward(self, x):
        out = self.layer3(self.layer2(self.layer1(self.relu(self.bn(self.conv(x))))))
        out = self.avg_pool(self.conv2d(out))
        return self.fc(out.view(out.size(0), -1))


Reference.__name__ = Reference.__qualname__ = "ResNet"   # what a script holds is utils.models.ResNet


def state(name):
    return {k: torch.tensor(v) for k, v in rc.make_state(name).items()}


def build(name, dev):
    B, H, W, K, _ = rc.CASES[name]
    m = ResNet(ResidualBlock, [2, 2, 2], K, rc.linear_features(H, W))
    m.load_state_dict(state(name))
    return m.to(dev)


def inputs(name, dev):
    x, y, ind = rc.make_inputs(name)
    t = lambda a: torch.tensor(a, device=dev)   # noqa: E731
    return t(x), t(y), t(ind)


def metrics_buf(dev):
    return torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)


def counters(logits, y, ind):
    pred = logits.argmax(1)
    return (len(y), int((pred == y).sum()), int((ind == 1).sum()), int(((ind == 1) & (pred == y)).sum()), 1)


def check(case, what, got, want):
    got, want = got.detach().double().cpu(), torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    e = float((got - want).abs().max()) if got.numel() else 0.0
    print(f"{case} {what}: {e:.3e}")
    assert e < rc.bound(case, what), (case, what, e)


def saved(m, B, name, n):
    eng = m._engine
    off = L.lib().abd_resnet_workspace_offset(eng.h, B, name.encode())
    assert off >= 0, name
    return eng._ws[off:off + 4 * n].view(torch.float32).clone()


def fused(m, x, y, ind, dev, update=True):
    """One fused step; returns (logits, metrics words)."""
    opt = torch.optim.Adam(m.parameters(), lr=rc.LR, betas=rc.BETAS, eps=rc.EPS)
    m.engine(x)
    adam = T.AdamBinding(m, opt)
    mt = metrics_buf(dev)
    out = torch.empty((x.shape[0], m.fc.out_features), device=dev)
    T.resnet_train_step(m, x, y, ind, adam, mt, do_update=update, logits_out=out)
    return out, T.read_metrics(mt)


@pytest.mark.parametrize("name", CASES)
def test_eval_parity_and_counters(dev, ref, name):
    x, y, ind = inputs(name, dev)
    m = build(name, dev).eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        out = m(x)
    check(name, "eval_logits", out, ref(name)["eval_logits"])
    mt = metrics_buf(dev)
    eng = m.engine(x)
    torch.ops.abd.resnet_eval_metrics(x, eng.params, eng.running, eng.K, y, ind, mt)
    loss, *cnt = T.read_metrics(mt)
    assert tuple(cnt) == counters(out, y, ind)
    assert abs(loss - float(ref(name)["eval_loss"])) < 1e-4
    after = m.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in before)   # eval updates nothing


@pytest.mark.parametrize("name", CASES)
def test_train_step_maps_gradients_running_and_adam(dev, ref, name):
    """Every saved map, the batch statistics, every gradient, all 30 running tensors and num_batches_tracked
    after one fused step; the Adam update is torch.optim.Adam's on the restatement's parameters with the device's
    gradients (the first step moves a parameter by lr g / (|g| + eps), which for |g| near eps turns a gradient
    difference far inside the bound into a full +-lr, so the oracle's own gradients cannot serve there)."""
    B, H, W, K, _ = rc.CASES[name]
    r = ref(name)
    x, y, ind = inputs(name, dev)
    m = build(name, dev).train()
    out, (loss, *cnt) = fused(m, x, y, ind, dev, update=False)
    check(name, "train_logits", out, r["acts"]["logits"])
    assert tuple(cnt) == counters(out, y, ind)
    assert abs(loss - float(r["loss"])) < 1e-4
    for u in range(len(rc.UNITS)):
        shp = rc.unit_shape(u, B, H, W)
        n = shp[0] * shp[1] * shp[2] * shp[3]
        for k in ("z", "a"):
            check(name, f"{k}{u}", rc.channels_first(saved(m, B, f"{k}{u}", n), shp), r["acts"][f"{k}{u}"])
        st = saved(m, B, f"s{u}", 2 * shp[1])
        check(name, f"mean{u}", st[:shp[1]], r["acts"][f"mean{u}"])
        check(name, f"invstd{u}", st[shp[1]:], (r["acts"][f"var{u}"] + rc.BN_EPS).rsqrt())
    c2 = r["acts"]["c2"]
    check(name, "c2", rc.channels_first(saved(m, B, "c2", c2.numel()), tuple(c2.shape)), c2)
    check(name, "pool", saved(m, B, "pool", r["acts"]["pool"].numel()).view(r["acts"]["pool"].shape), r["acts"]["pool"])
    eng = m._engine
    grads = {n_: g.clone() for n_, g in zip(rc.PARAM_ORDER, eng.views(eng.grads))}
    for n_ in rc.PARAM_ORDER:
        check(name, f"grad {n_}", grads[n_].view(r["grads"][n_].shape), r["grads"][n_])
        if K == 1:
            assert not grads[n_].any()
    sd = m.state_dict()
    for k, v in r["running"].items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v), k
        else:
            check(name, f"running {k}", sd[k], v)
    # the same step with the update, from equal state: bit-equal logits and gradients, torch's Adam on them
    m2 = build(name, dev).train()
    out2, _ = fused(m2, x, y, ind, dev, update=True)
    assert torch.equal(out2, out)
    assert torch.equal(m2._engine.grads, eng.grads)
    p64 = [torch.tensor(rc.make_state(name)[n_], dtype=torch.float64, requires_grad=True) for n_ in rc.PARAM_ORDER]
    for p, n_ in zip(p64, rc.PARAM_ORDER):
        p.grad = grads[n_].double().cpu().view(p.shape)
    torch.optim.Adam(p64, lr=rc.LR, betas=rc.BETAS, eps=rc.EPS).step()
    for p, q, n_ in zip(p64, m2._param_list(), rc.PARAM_ORDER):
        check(name, f"adam {n_}", q, p.detach())
    # eval after the step runs on the updated parameters and running statistics
    m2.eval()
    with torch.no_grad():
        ev = m2(x)
        sd2 = {k: v.double().cpu() if v.is_floating_point() else v.cpu() for k, v in m2.state_dict().items()}
        want = rc.restate({n_: sd2[n_] for n_ in rc.PARAM_ORDER}, {k: sd2[k] for k in rc.BUFFER_ORDER},
                          x.double().cpu(), False)["logits"]
    check(name, "eval_after_step", ev, want)
    assert float((ev - torch.as_tensor(r["eval_logits"]).to(ev)).abs().max()) > 1e-3 or K == 1


@pytest.mark.parametrize("name", CASES)
def test_autograd_path_bit_equal_and_two_steps_bit_equal(dev, name):
    x, y, ind = inputs(name, dev)
    a, b, c = (build(name, dev).train() for _ in range(3))
    out_a, _ = fused(a, x, y, ind, dev, update=False)
    out_b, _ = fused(b, x, y, ind, dev, update=False)
    assert torch.equal(out_a, out_b) and torch.equal(a._engine.grads, b._engine.grads)
    assert torch.equal(a._engine.running, b._engine.running)
    logits = c(x)
    nn.CrossEntropyLoss()(logits, y).backward()
    assert torch.equal(logits.detach(), out_a)
    for p, g in zip(c._param_list(), a._engine.views(a._engine.grads)):
        assert torch.equal(p.grad.reshape(-1), g)
    assert torch.equal(c._engine.running, a._engine.running) and torch.equal(c._engine.nbt, a._engine.nbt)


def test_backward_must_follow_its_forward(dev):
    x, y, ind = inputs("tiny", dev)
    m = build("tiny", dev).train()
    l1 = m(x)
    fused(m, x, y, ind, dev, update=False)   # overwrites the workspace
    with pytest.raises(L.AbdError):
        l1.sum().backward()


def _loaders(name):
    B, H, W, K, _ = rc.CASES[name]
    g = torch.Generator().manual_seed(11)
    n = 3 * B
    xc = torch.randn(n, 1, H, W, generator=g)
    yc = torch.randint(0, K, (n,), generator=g)
    ic = (torch.rand(n, generator=g) < 0.4).long()
    ic[0] = 1

    class Dict(Data.Dataset):
        def __len__(self):
            return n

        def __getitem__(self, i):
            return {"mfcc": xc[i], "label": yc[i], "poison_indicator": ic[i]}

    return xc, Data.DataLoader(Dict(), batch_size=B), Data.DataLoader(Data.TensorDataset(xc, yc), batch_size=B)


def test_training_loops_native_and_adopted(dev):
    """train / test / clean_train / clean_test on a three-batch in-memory loader: the same returns and the same
    final state_dict for this package's class and for a reference-shaped instance, whose own Parameter objects
    and BatchNorm buffers are re-homed and whose optimizer state holds the flat Adam views."""
    name = "tiny"
    B, H, W, K, _ = rc.CASES[name]
    xc, bd, clean = _loaders(name)
    crit = nn.CrossEntropyLoss()
    script = Reference(K, rc.linear_features(H, W))
    script.load_state_dict(state(name))
    script.to(dev)
    held = list(script.parameters())
    opt = torch.optim.Adam(script.parameters(), lr=rc.LR)
    native = build(name, dev)
    on = torch.optim.Adam(native.parameters(), lr=rc.LR)
    rets_n = [T.train(native, bd, dev, on, crit), T.test(native, dev, clean, bd, crit),
              T.clean_train(native, clean, dev, on, crit), T.clean_test(native, dev, clean, crit)]
    rets_s = [T.train(script, bd, dev, opt, crit), T.test(script, dev, clean, bd, crit),
              T.clean_train(script, clean, dev, opt, crit), T.clean_test(script, dev, clean, crit)]
    assert rets_s == rets_n
    ad = adopt(script)
    assert ad is adopt(script) and not hasattr(script, "_engine") and ad._bound(ad._engine)
    assert [id(p) for p in script.parameters()] == [id(p) for p in held]
    assert set(opt.state.keys()) == set(held) and all(float(opt.state[p]["step"]) == 6.0 for p in held)
    lo, n = ad._engine.exp_avg.data_ptr(), ad._engine.n
    assert all(lo <= opt.state[p]["exp_avg"].data_ptr() < lo + 4 * n for p in held)
    sn, ss = native.state_dict(), script.state_dict()
    assert list(sn) == list(ss)
    assert all(torch.equal(sn[k], ss[k]) for k in sn)
    assert int(ss["layer2.0.downsample.1.num_batches_tracked"]) == 3 + 7 + 6
    assert not torch.equal(ss["bn.running_mean"].cpu(), state(name)["bn.running_mean"])
    assert all(p.grad is not None for p in held)
    # the script's own eager forward runs on the trained weights and statistics
    script.eval()
    with torch.no_grad():
        own = script(xc[:4].to(dev))
        ours = ad.eval()(xc[:4].to(dev))
    check(name, "adopted eager forward", ours, own.double().cpu())
    # a state_dict round trip into a fresh model
    fresh = ResNet(ResidualBlock, [2, 2, 2], K, rc.linear_features(H, W))
    fresh.load_state_dict({k: v.cpu() for k, v in ss.items()})
    fresh.to(dev).eval()
    with torch.no_grad():
        assert torch.equal(fresh(xc[:4].to(dev)), ours)


def test_guards_and_refusals(dev):
    name = "tiny"
    B, H, W, K, _ = rc.CASES[name]
    x, y, ind = inputs(name, dev)
    m = build(name, dev).train()
    eng = m.engine(x)
    need = L.lib().abd_resnet_workspace_bytes(eng.h, B)
    eng._ws = torch.full((need + GUARD,), PAT, dtype=torch.uint8, device=dev)[:need + GUARD]
    ws = eng._ws
    out = torch.full((B + 4, K), float("nan"), device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=rc.LR)
    adam = T.AdamBinding(m, opt)
    a = m._args(eng, x, B)
    a.labels, a.indicators = y.data_ptr(), ind.data_ptr()
    a.logits_out = out.data_ptr()
    a.exp_avg, a.exp_avg_sq = eng.exp_avg.data_ptr(), eng.exp_avg_sq.data_ptr()
    a.lr, a.beta1, a.beta2, a.eps, a.adam_step, a.do_update = adam.lr, 0.9, 0.999, 1e-8, 1, 1
    assert L.lib().abd_resnet_train_step(eng.h, C.byref(a), ws.data_ptr(), need, L.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert int((ws[need:] != PAT).sum()) == 0
    assert torch.isnan(out[B:]).all() and torch.isfinite(out[:B]).all()
    assert L.lib().abd_resnet_train_step(eng.h, C.byref(a), ws.data_ptr(), need - 1, None) == 1003
    assert L.lib().abd_resnet_forward(eng.h, C.byref(a), 1, ws.data_ptr(), 16, None) == 1003
    with pytest.raises(L.AbdError):
        T.resnet_train_step(m, x, None, None, None, None)   # no labels
    with pytest.raises(L.AbdError):
        m(x.cpu())
    with pytest.raises(ValueError):
        m(torch.zeros(B, 1, 64, 13, device=dev))   # another linear_features
    with pytest.raises(L.AbdError):
        T.train(m, [], dev, torch.optim.SGD(m.parameters(), lr=0.1), nn.CrossEntropyLoss())
