"""GPU: smalllstm on libabd against the float64 restatement of tests/smalllstm_cases.py.

Bound: 1e-4 absolute on every tensor, except the five saved 1 / sqrt(var + eps) entries of smalllstm_cases.BOUNDS,
where the float32 CPU run of the restatement is itself up to 4.5e-3 from float64 and the bound is four times that
distance (everywhere else the float32 CPU run stays within 8.9e-5, tests/test_smalllstm_cpu.py); counters exact.
Every distance is printed as it is measured; a test measures all of its tensors and then asserts that none missed
its bound (profiles/smalllstm/parity.md records the figures).
"""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.data as Data

import abd_amd
from abd_amd import _lib as L, training as T
from abd_amd.models_smalllstm import smalllstm, adopt, tile_info
import smalllstm_cases as sc

pytestmark = pytest.mark.gpu
GUARD = 8 << 20
PAT = 0xA5
CASES = list(sc.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    # the cases are sized from the built kernels' tiles and thresholds
    assert [tile_info(k) for k in ("tile_rows", "k_step", "slice_rows", "max_slices", "stat_rows", "stat_blocks",
                                   "rec_rows")] == [sc.TILE_ROWS, sc.K_STEP, sc.SLICE_ROWS, sc.MAX_SLICES,
                                                    sc.STAT_ROWS, sc.STAT_BLOCKS, sc.REC_ROWS]
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref():
    """The float64 reference of a case, built once per module and shared read-only."""
    return lambda name: sc.run_case(name, torch.float64)


class Reference(nn.Module):
    """A module of the reference's shape (utils/models.py:121-178), from torch.nn layers: what a script holds."""

    def __init__(self, num_classes, rnn_features):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 64, kernel_size=(2, 2))
        self.bn1 = nn.BatchNorm2d(64)
        self.pool1 = nn.MaxPool2d(kernel_size=(1, 3))
        self.conv2 = nn.Conv2d(64, 64, kernel_size=(2, 2))
        self.bn2 = nn.BatchNorm2d(64)
        self.pool2 = nn.MaxPool2d(kernel_size=(2, 2), padding=(1, 1))
        self.conv3 = nn.Conv2d(64, 32, kernel_size=(2, 2))
        self.bn3 = nn.BatchNorm2d(32)
        self.pool3 = nn.MaxPool2d(kernel_size=(2, 2), padding=(0, 1))
        self.drop1 = nn.Dropout(0.4)
        self.flat = nn.Flatten()
        self.rnn = nn.LSTM(rnn_features, 128, 2, batch_first=True, bidirectional=False)
        self.fc1 = nn.Linear(224, 128)
        self.drop2 = nn.Dropout(0.5)
        self.fc2 = nn.Linear(128, num_classes)
        self.softmax = nn.Softmax()

    def forward(self, x):
        x = self.pool1(self.bn1(F.relu(self.conv1(x))))
        x = self.pool2(self.bn2(F.relu(self.conv2(x))))
        x = self.drop1(self.pool3(self.bn3(F.relu(self.conv3(x)))))
        n, c, h, w = x.shape
        x = x.permute(0, 2, 3, 1).reshape(n, h, w * c)
        z = torch.zeros(2, n, 128, device=x.device)
        hs, _ = self.rnn(x, (z, z))
        return F.log_softmax(self.fc2(hs[:, -1, :]), dim=1)


Reference.__name__ = Reference.__qualname__ = "smalllstm"   # what a script holds is utils.models.smalllstm


def state(name):
    return {k: torch.tensor(v) for k, v in sc.make_state(name).items()}


def build(name, dev):
    B, H, W, K, _ = sc.CASES[name]
    m = smalllstm(K, sc.rnn_features(H, W))
    m.load_state_dict(state(name))
    return m.to(dev)


def inputs(name, dev):
    t = lambda a: torch.tensor(a, device=dev)   # noqa: E731
    return tuple(t(a) for a in sc.make_inputs(name))


def metrics_buf(dev):
    return torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)


def counters(logits, y, ind):
    pred = logits.argmax(1)
    return (len(y), int((pred == y).sum()), int((ind == 1).sum()), int(((ind == 1) & (pred == y)).sum()), 1)


_MISSES: list = []


def check(case, what, got, want):
    """Prints the distance and notes a miss of the bound; all_within_bounds asserts, after the test has measured
    every tensor, that there was none."""
    got, want = got.detach().double().cpu(), torch.as_tensor(want, dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    e = float((got - want).abs().max()) if got.numel() else 0.0
    print(f"{case} {what}: {e:.3e}")
    if not e < sc.bound(case, what):
        _MISSES.append((case, what, e, sc.bound(case, what)))


@pytest.fixture(autouse=True)
def all_within_bounds():
    _MISSES.clear()
    yield
    misses = list(_MISSES)
    _MISSES.clear()
    assert not misses, misses


def saved(m, B, name, n):
    eng = m._engine
    off = L.lib().abd_smalllstm_workspace_offset(eng.h, B, name.encode())
    assert off >= 0, name
    return eng._ws[off:off + 4 * n].view(torch.float32).clone()


def fused(m, x, y, ind, dev, update=True, mask=None, mask_out=None, seed=None):
    """One fused step; returns (log-probabilities, metrics words)."""
    opt = torch.optim.Adam(m.parameters(), lr=sc.LR, betas=sc.BETAS, eps=sc.EPS)
    m.engine(x)
    adam = T.AdamBinding(m, opt)
    mt = metrics_buf(dev)
    out = torch.empty((x.shape[0], m.fc2.out_features), device=dev)
    T.smalllstm_train_step(m, x, y, ind, adam, mt, mask=mask, mask_out=mask_out, do_update=update, seed=seed,
                           logits_out=out)
    return out, T.read_metrics(mt)


@pytest.mark.parametrize("name", CASES)
def test_eval_parity_and_counters(dev, ref, name):
    x, y, ind, _ = inputs(name, dev)
    m = build(name, dev).eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        out = m(x)
    check(name, "eval_logits", out, ref(name)["eval_logits"])
    mt = metrics_buf(dev)
    eng = m.engine(x)
    torch.ops.abd.smalllstm_eval_metrics(x, eng.params, eng.running, eng.K, y, ind, mt)
    loss, *cnt = T.read_metrics(mt)
    assert tuple(cnt) == counters(out, y, ind)
    assert abs(loss - float(ref(name)["eval_loss"])) < 1e-4
    after = m.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in before)   # eval updates nothing


@pytest.mark.parametrize("name", CASES)
def test_train_step_maps_gradients_running_and_adam(dev, ref, name):
    """Every saved map, the batch statistics, both layers' h and c at every step, every gradient (fc1's exactly
    zero), the running statistics and num_batches_tracked after one fused step under the case's mask; the Adam
    update is torch.optim.Adam's on the restatement's parameters with the device's gradients (the first step moves
    a parameter by lr g / (|g| + eps), which for |g| near eps turns a gradient difference far inside the bound into
    a full +-lr, so the oracle's own gradients cannot serve there)."""
    B, H, W, K, _ = sc.CASES[name]
    r = ref(name)
    x, y, ind, mask = inputs(name, dev)
    m = build(name, dev).train()
    mo = torch.zeros_like(mask)
    out, (loss, *cnt) = fused(m, x, y, ind, dev, update=False, mask=mask, mask_out=mo)
    assert torch.equal(mo, mask)
    check(name, "train_logits", out, r["acts"]["logits"])
    assert tuple(cnt) == counters(out, y, ind)
    assert abs(loss - float(r["loss"])) < 1e-4
    for i in (1, 2, 3):
        for k in ("z", "a", "p"):
            want = r["acts"][f"{k}{i}"]
            check(name, f"{k}{i}", sc.channels_first(saved(m, B, f"{k}{i}", want.numel()), tuple(want.shape)), want)
        Cc = r["acts"][f"mean{i}"].numel()
        st = saved(m, B, f"s{i}", 2 * Cc)
        check(name, f"mean{i}", st[:Cc], r["acts"][f"mean{i}"])
        check(name, f"invstd{i}", st[Cc:], (r["acts"][f"var{i}"] + sc.BN_EPS).rsqrt())
    check(name, "seq", saved(m, B, "seq", r["acts"]["seq"].numel()).view(r["acts"]["seq"].shape), r["acts"]["seq"])
    for l in range(sc.LAYERS):
        for k in ("h", "c"):
            want = r["acts"][f"{k}{l}"]
            check(name, f"{k}{l}", saved(m, B, f"{k}{l}", want.numel()).view(want.shape), want)
    eng = m._engine
    grads = {n_: g.clone() for n_, g in zip(sc.PARAM_ORDER, eng.views(eng.grads))}
    for n_ in sc.PARAM_ORDER:
        check(name, f"grad {n_}", grads[n_].view(r["grads"][n_].shape), r["grads"][n_])
        if K == 1 or n_.startswith("fc1."):
            assert not grads[n_].any(), n_
    sd = m.state_dict()
    for k, v in r["running"].items():
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v), k
        else:
            check(name, f"running {k}", sd[k], v)
    # the same step with the update, from equal state: bit-equal log-probabilities and gradients, torch's Adam on them
    m2 = build(name, dev).train()
    out2, _ = fused(m2, x, y, ind, dev, update=True, mask=mask)
    assert torch.equal(out2, out)
    assert torch.equal(m2._engine.grads, eng.grads)
    st0 = sc.make_state(name)
    p64 = [torch.tensor(st0[n_], dtype=torch.float64, requires_grad=True) for n_ in sc.PARAM_ORDER]
    for p, n_ in zip(p64, sc.PARAM_ORDER):
        p.grad = grads[n_].double().cpu().view(p.shape)
    torch.optim.Adam(p64, lr=sc.LR, betas=sc.BETAS, eps=sc.EPS).step()
    for p, q, n_ in zip(p64, m2._param_list(), sc.PARAM_ORDER):
        check(name, f"adam {n_}", q, p.detach())
        if n_.startswith("fc1."):
            assert torch.equal(q.cpu(), torch.tensor(st0[n_])), n_   # bit-unchanged
    # eval after the step runs on the updated parameters and running statistics
    m2.eval()
    with torch.no_grad():
        ev = m2(x)
        sd2 = {k: v.double().cpu() if v.is_floating_point() else v.cpu() for k, v in m2.state_dict().items()}
        want = sc.restate({n_: sd2[n_] for n_ in sc.PARAM_ORDER}, {k: sd2[k] for k in sc.BUFFER_ORDER},
                          x.double().cpu(), False)["logits"]
    check(name, "eval_after_step", ev, want)
    assert float((ev - torch.as_tensor(r["eval_logits"]).to(ev)).abs().max()) > 1e-3 or K == 1


@pytest.mark.parametrize("name", CASES)
def test_determinism_autograd_path_and_mask_replay(dev, name):
    x, y, ind, _ = inputs(name, dev)
    a, b, c, d = (build(name, dev).train() for _ in range(4))
    for m in (a, b, c, d):
        m._dropout_nonce = 5   # one hash stream for all four
    mo = torch.zeros(a.mask_shape(x), dtype=torch.uint8, device=dev)
    out_a, _ = fused(a, x, y, ind, dev, update=False, mask_out=mo, seed=77)
    out_b, _ = fused(b, x, y, ind, dev, update=False, seed=77)
    assert torch.equal(out_a, out_b) and torch.equal(a._engine.grads, b._engine.grads)
    assert torch.equal(a._engine.running, b._engine.running)
    # the mask the hash step used, handed back in, reproduces it
    out_d, _ = fused(d, x, y, ind, dev, update=False, mask=mo, seed=1)
    assert torch.equal(out_d, out_a) and torch.equal(d._engine.grads, a._engine.grads)
    # model(x), CrossEntropyLoss, backward: the same launches
    torch.manual_seed(3)
    e = build(name, dev).train()
    e._dropout_nonce = 5
    torch.manual_seed(3)
    logp = c(x)
    nn.CrossEntropyLoss()(logp, y).backward()
    out_e, _ = fused(e, x, y, ind, dev, update=False)   # the default seed, as c's forward took it
    assert torch.equal(logp.detach(), out_e)
    for p, g in zip(c._param_list(), e._engine.views(e._engine.grads)):
        assert torch.equal(p.grad.reshape(-1), g)
    assert torch.equal(c._engine.running, e._engine.running) and torch.equal(c._engine.nbt, e._engine.nbt)


def test_backward_must_follow_its_forward(dev):
    x, y, ind, _ = inputs("tiny", dev)
    m = build("tiny", dev).train()
    l1 = m(x)
    fused(m, x, y, ind, dev, update=False)   # overwrites the workspace
    with pytest.raises(L.AbdError):
        l1.sum().backward()


def _loaders(name):
    B, H, W, K, _ = sc.CASES[name]
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
    name = "flowmur"
    B, H, W, K, _ = sc.CASES[name]
    xc, bd, clean = _loaders(name)
    crit = nn.CrossEntropyLoss()
    script = Reference(K, sc.rnn_features(H, W))
    script.load_state_dict(state(name))
    script.to(dev)
    held = list(script.parameters())
    opt = torch.optim.Adam(script.parameters(), lr=sc.LR)
    native = build(name, dev)
    on = torch.optim.Adam(native.parameters(), lr=sc.LR)
    torch.manual_seed(5)
    rets_n = [T.train(native, bd, dev, on, crit), T.test(native, dev, clean, bd, crit),
              T.clean_train(native, clean, dev, on, crit), T.clean_test(native, dev, clean, crit)]
    torch.manual_seed(5)
    rets_s = [T.train(script, bd, dev, opt, crit), T.test(script, dev, clean, bd, crit),
              T.clean_train(script, clean, dev, opt, crit), T.clean_test(script, dev, clean, crit)]
    assert rets_s == rets_n
    ad = adopt(script)
    assert ad is adopt(script) and not hasattr(script, "_engine") and ad._bound(ad._engine)
    assert [id(p) for p in script.parameters()] == [id(p) for p in held]
    assert all(w is p for w, p in zip(script.rnn._flat_weights, script.rnn.parameters()))
    assert set(opt.state.keys()) == set(held) and all(float(opt.state[p]["step"]) == 6.0 for p in held)
    lo, n = ad._engine.exp_avg.data_ptr(), ad._engine.n
    assert all(lo <= opt.state[p]["exp_avg"].data_ptr() < lo + 4 * n for p in held)
    sn, ss = native.state_dict(), script.state_dict()
    assert list(sn) == list(ss)
    assert all(torch.equal(sn[k], ss[k]) for k in sn)
    assert int(ss["bn3.num_batches_tracked"]) == 3 + 2 + 6
    assert not torch.equal(ss["bn1.running_mean"].cpu(), state(name)["bn1.running_mean"])
    assert all(p.grad is not None for p in held)
    assert torch.equal(ss["fc1.weight"].cpu(), state(name)["fc1.weight"])   # Adam on a zero gradient moves nothing
    # the script's own eager forward runs on the trained weights and statistics
    script.eval()
    with torch.no_grad():
        own = script(xc[:4].to(dev))
        ours = ad.eval()(xc[:4].to(dev))
    check(name, "adopted eager forward", ours, own.double().cpu())
    # a state_dict round trip into a fresh model
    fresh = smalllstm(K, sc.rnn_features(H, W))
    fresh.load_state_dict({k: v.cpu() for k, v in ss.items()})
    fresh.to(dev).eval()
    with torch.no_grad():
        assert torch.equal(fresh(xc[:4].to(dev)), ours)


def test_guards_and_refusals(dev):
    name = "tiny"
    B, H, W, K, _ = sc.CASES[name]
    x, y, ind, _ = inputs(name, dev)
    m = build(name, dev).train()
    eng = m.engine(x)
    need = L.lib().abd_smalllstm_workspace_bytes(eng.h, B)
    eng._ws = torch.full((need + GUARD,), PAT, dtype=torch.uint8, device=dev)[:need + GUARD]
    ws = eng._ws
    out = torch.full((B + 4, K), float("nan"), device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=sc.LR)
    adam = T.AdamBinding(m, opt)
    a = m._args(eng, x, B)
    a.labels, a.indicators = y.data_ptr(), ind.data_ptr()
    a.logits_out = out.data_ptr()
    a.exp_avg, a.exp_avg_sq = eng.exp_avg.data_ptr(), eng.exp_avg_sq.data_ptr()
    a.lr, a.beta1, a.beta2, a.eps, a.adam_step, a.do_update = adam.lr, 0.9, 0.999, 1e-8, 1, 1
    assert L.lib().abd_smalllstm_train_step(eng.h, C.byref(a), ws.data_ptr(), need, L.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert int((ws[need:] != PAT).sum()) == 0
    assert torch.isnan(out[B:]).all() and torch.isfinite(out[:B]).all()
    assert L.lib().abd_smalllstm_train_step(eng.h, C.byref(a), ws.data_ptr(), need - 1, None) == 1003
    assert L.lib().abd_smalllstm_forward(eng.h, C.byref(a), 1, ws.data_ptr(), 16, None) == 1003
    # a train-mode forward without the running statistics leaves num_batches_tracked alone too
    nbt, run = eng.nbt.clone(), eng.running.clone()
    a.running = None
    assert L.lib().abd_smalllstm_forward(eng.h, C.byref(a), 1, ws.data_ptr(), need, L.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert torch.equal(eng.nbt, nbt) and torch.equal(eng.running, run)
    with pytest.raises(L.AbdError):
        T.smalllstm_train_step(m, x, None, None, None, None)   # no labels
    with pytest.raises(L.AbdError):
        m(x.cpu())
    with pytest.raises(ValueError):
        m(torch.zeros(B, 1, 32, 40, device=dev))   # another rnn_features
    with pytest.raises(L.AbdError):
        T.train(m, [], dev, torch.optim.SGD(m.parameters(), lr=0.1), nn.CrossEntropyLoss())
