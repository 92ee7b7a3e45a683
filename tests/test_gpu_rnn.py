"""GPU: RNN on libabd against the float64 restatement of tests/rnn_cases.py.

Bounds: 1e-4 relative to the largest magnitude of the compared tensor (the project's fp32 bound; the float32 CPU
run of the restatement stays within 1e-5, tests/test_rnn_cpu.py), counters exact.  Measured distances are
printed before each assertion (profiles/rnn/parity.md records them).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.utils.data as Data

import abd_amd
from abd_amd import _lib as L, training as T
from abd_amd.models_rnn import RNN, tile_info
import rnn_cases as rc

pytestmark = pytest.mark.gpu
GUARD = 8 << 20
PAT = 0xA5
CASES = list(rc.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    # the cases are sized from the built kernels' tiles and thresholds
    assert [tile_info(k) for k in ("rec_rows", "small_tile", "large_tile", "slice_rows", "colsum_rows",
                                   "large_min_blocks")] == [rc.REC_ROWS, rc.SMALL_TILE, rc.LARGE_TILE, rc.SLICE_ROWS,
                                                            rc.COLSUM_ROWS, rc.LARGE_MIN_BLOCKS]
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ref():
    """The float64 reference of a case, built once per module and shared read-only."""
    return lambda name, states=False: rc.run_case(name, torch.float64, states=states)


def build(name, dev):
    B, Tn, Fd, K, _ = rc.CASES[name]
    m = RNN(K, Fd)
    m.load_state_dict({k: torch.tensor(v) for k, v in rc.make_state(name).items()})
    return m.to(dev)


def inputs(name, dev):
    x, y, ind = rc.make_inputs(name)
    return torch.tensor(x, device=dev), torch.tensor(y, device=dev), torch.tensor(ind, device=dev)


def metrics_buf(dev):
    return torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)


def counters(logits, y, ind):
    pred = logits.argmax(1)
    return (len(y), int((pred == y).sum()), int((ind == 1).sum()), int(((ind == 1) & (pred == y)).sum()), 1)


def check(what, got, want, tol=1e-4):
    e = rc.rel_err(got.detach().cpu(), want)
    print(f"{what}: {e:.3e}")
    assert e < tol, (what, e)


def close_loss(what, got, want):
    want = float(want)
    e = abs(got - want) / want if want > 0 else abs(got - want)
    print(f"{what}: {e:.3e}")
    assert e < 1e-4, (what, got, want)


def saved(m, B, name, shape):
    eng = m._engine
    off = L.lib().abd_rnn_workspace_offset(eng.h, B, name.encode())
    assert off >= 0
    n = int(np.prod(shape))
    return eng._ws[off:off + 4 * n].view(torch.float32).view(shape).clone()


@pytest.mark.parametrize("name", CASES)
def test_forward_parity_and_counters(dev, ref, name):
    """Logits and counters of the eval ops and of the train step; with no BatchNorm and no dropout the two
    forwards are the same computation and must agree bit for bit."""
    B, Tn, Fd, K, _ = rc.CASES[name]
    r = ref(name)
    x, y, ind = inputs(name, dev)
    m = build(name, dev).eval()
    with torch.no_grad():
        ev = m(x)
    check(f"{name} eval logits", ev, r["logits"])
    eng = m._engine
    mt = metrics_buf(dev)
    ev2 = torch.ops.abd.rnn_eval_metrics(x, eng.params, K, y, ind, mt)
    assert torch.equal(ev2, ev)
    loss, *cnt = T.read_metrics(mt)
    close_loss(f"{name} eval loss", loss, r["loss"])
    assert tuple(cnt) == counters(r["logits"], y.cpu(), ind.cpu())
    m.train()
    mt = metrics_buf(dev)
    out = torch.empty((B, K), device=dev)
    T.rnn_train_step(m, x, y, ind, None, mt, do_update=False, logits_out=out)
    assert torch.equal(out, ev)
    loss2, *cnt2 = T.read_metrics(mt)
    assert loss2 == loss and cnt2 == cnt
    # a non-float32 input is cast as the reference casts it
    with torch.no_grad():
        assert torch.equal(m.eval()(x.double()), ev)


@pytest.mark.parametrize("name", CASES)
def test_gradients_saved_states_and_determinism(dev, ref, name):
    B, Tn, Fd, K, _ = rc.CASES[name]
    r = ref(name, states=True)
    x, y, ind = inputs(name, dev)
    m = build(name, dev).train()
    m.hip_forward(x)
    for layer, (h, c, g) in enumerate(r["states"], 1):
        check(f"{name} h{layer}", saved(m, B, f"h{layer}", (B, Tn, rc.H)), h)
        check(f"{name} c{layer}", saved(m, B, f"c{layer}", (B, Tn, rc.H)), c)
        check(f"{name} gates{layer}", saved(m, B, f"gates{layer}", (B, Tn, 4 * rc.H)), g)
    T.rnn_train_step(m, x, y, ind, None, None, do_update=False)
    eng = m._engine
    g_step = eng.grads.clone()
    for n, g in zip(rc.PARAM_ORDER, eng.views(g_step)):
        check(f"{name} grad {n}", g, r["grads"][n], rc.bound(name, n))
    if Tn == 1:
        for k in range(rc.LAYERS):   # h_{-1} = 0: no recurrent weight gradient at all
            assert float(eng.views(g_step)[4 * k + 1].abs().max()) == 0.0
    if K == 1:
        assert float(g_step.abs().max()) == 0.0
    # the same step twice: bit-equal
    T.rnn_train_step(m, x, y, ind, None, None, do_update=False)
    assert torch.equal(eng.grads, g_step)


def _autograd_and_step(dev, name):
    x, y, ind = inputs(name, dev)
    m2 = build(name, dev).train()
    nn.CrossEntropyLoss()(m2(x), y).backward()
    m3 = build(name, dev).train()
    T.rnn_train_step(m3, x, y, ind, None, None, do_update=False)
    return [p.grad.reshape(-1) for p in m2._param_list()], m3._engine.views(m3._engine.grads)


@pytest.mark.parametrize("name", ["tiny", "one_step", "ragged_tiles", "wide", "big_batch"])
def test_backward_entry_and_autograd_path(dev, ref, name):
    """abd_rnn_forward, torch's CrossEntropyLoss, abd_rnn_backward: within the bound of float64, and bit-equal
    to abd_rnn_train_step (the step's d(logits) follows torch's log_softmax / nll_loss arithmetic)."""
    auto, step = _autograd_and_step(dev, name)
    r = ref(name)
    for n, a, s in zip(rc.PARAM_ORDER, auto, step):
        check(f"{name} backward grad {n}", a, r["grads"][n], rc.bound(name, n))
        assert torch.equal(a, s), n


def test_backward_must_follow_its_forward(dev):
    x, y, ind = inputs("tiny", dev)
    m = build("tiny", dev).train()
    a, b = m(x), m(x)
    with pytest.raises(L.AbdError):
        a.sum().backward()
    b.sum().backward()
    with pytest.raises(L.AbdError):   # backward consumed the saved gates
        m.hip_backward(x, torch.ones_like(b), m._engine.token)


@pytest.mark.parametrize("name", ["tiny", "ragged_tiles"])
def test_fused_adam_equals_split_update(dev, ref, name):
    x, y, ind = inputs(name, dev)
    ms = [build(name, dev).train() for _ in range(2)]
    opts = [torch.optim.Adam(m.parameters(), lr=rc.LR) for m in ms]
    adams = []
    for m, o in zip(ms, opts):
        m.engine(x)
        adams.append(T.AdamBinding(m, o))
    T.rnn_train_step(ms[0], x, y, ind, adams[0], None, do_update=True)
    T.rnn_train_step(ms[1], x, y, ind, adams[1], None, do_update=False)
    T.apply_adam(ms[1], adams[1], dev)
    a, b = ms
    assert torch.equal(a._engine.params, b._engine.params)
    assert torch.equal(a._engine.exp_avg, b._engine.exp_avg)
    assert torch.equal(a._engine.exp_avg_sq, b._engine.exp_avg_sq)
    # the update moved every tensor, by at most lr per element on the first step (|m / sqrt(v)| <= 1)
    start = torch.cat([torch.tensor(rc.make_state(name)[n]).reshape(-1) for n in rc.PARAM_ORDER]).to(dev)
    moved = (a._engine.params - start).abs()
    assert float(moved.max()) <= rc.LR * (1 + 1e-3)
    for n, v in zip(rc.PARAM_ORDER, a._engine.views(moved)):
        assert float(v.max()) > 0.0, n


class DictSet(Data.Dataset):
    def __init__(self, x, y, ind):
        self.x, self.y, self.ind = x, y, ind

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return {"mfcc": self.x[i], "label": self.y[i], "poison_indicator": self.ind[i]}


def test_training_loop_equals_manual_loop(dev):
    name = "ragged_tiles"
    B, Tn, Fd, K, _ = rc.CASES[name]
    xn, yn, indn = rc.make_inputs(name)
    xc, yc, ic = torch.tensor(xn), torch.tensor(yn), torch.tensor(indn)
    bd = Data.DataLoader(DictSet(xc, yc, ic), batch_size=40, shuffle=False)     # batches of 40 and 25
    clean = Data.DataLoader(Data.TensorDataset(xc, yc), batch_size=40, shuffle=False)
    crit = nn.CrossEntropyLoss()
    a, b = build(name, dev), build(name, dev)
    oa = torch.optim.Adam(a.parameters(), lr=rc.LR)
    ob = torch.optim.Adam(b.parameters(), lr=rc.LR)
    got = T.train(a, bd, dev, oa, crit)
    b.train()
    mt = metrics_buf(dev)
    adam = None
    for item in bd:
        x, y, ind = item["mfcc"].to(dev), item["label"].to(dev), item["poison_indicator"].to(dev)
        if adam is None:
            b.engine(x)
            adam = T.AdamBinding(b, ob)
        T.rnn_train_step(b, x, y, ind, adam, mt)
    ls, tot, cor, pt, asr, nb = T.read_metrics(mt)
    assert got == (ls / nb, 100.0 * cor / tot, 100 * asr / pt)
    assert torch.equal(a._engine.params, b._engine.params)
    for p in a.parameters():
        assert float(oa.state[p]["step"]) == 2.0
        assert p.grad is not None and p.grad.shape == p.shape
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in a._param_list()]), a._engine.grads)
    # test() / clean_test() / clean_train() against the ops
    got_t = T.test(a, dev, clean, bd, crit)
    eng = b._engine
    mc, mb = metrics_buf(dev), metrics_buf(dev)
    for lo, hi in ((0, 40), (40, B)):
        x, y, ind = xc[lo:hi].to(dev), yc[lo:hi].to(dev), ic[lo:hi].to(dev)
        torch.ops.abd.rnn_eval_metrics(x, eng.params, K, y, None, mc)
        torch.ops.abd.rnn_eval_metrics(x, eng.params, K, y, ind, mb)
    cl, ct, cc, _, _, nc = T.read_metrics(mc)
    bl, _, _, pt, ah, nbb = T.read_metrics(mb)
    assert got_t == (100 * cc / ct, 100 * ah / pt, cl / nc, bl / nbb)
    assert T.clean_test(a, dev, clean, crit) == (cl / nc, 100 * cc / ct)
    got_c = T.clean_train(a, clean, dev, oa, crit)
    mt = metrics_buf(dev)
    for xb, yb in clean:
        T.rnn_train_step(b, xb.to(dev), yb.to(dev), None, adam, mt)
    ls, tot, cor, _, _, nb = T.read_metrics(mt)
    assert got_c == (ls / nb, 100.0 * cor / tot)
    assert torch.equal(a._engine.params, b._engine.params)
    with pytest.raises(L.AbdError):   # SGD is not the fused step's optimizer
        T.train(a, bd, dev, torch.optim.SGD(a.parameters(), lr=0.1), crit)


def test_guards_and_refusals(dev):
    name = "tiny"
    B, Tn, Fd, K, _ = rc.CASES[name]
    x, y, ind = inputs(name, dev)
    m = build(name, dev).train()
    eng = m.engine(x)
    need = L.lib().abd_rnn_workspace_bytes(eng.h, B)
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
    # the workspace handed over is exactly `need` bytes, followed by the guard
    assert L.lib().abd_rnn_train_step(eng.h, C.byref(a), ws.data_ptr(), need, L.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    assert int((ws[need:] != PAT).sum()) == 0
    assert torch.isnan(out[B:]).all() and torch.isfinite(out[:B]).all()
    assert L.lib().abd_rnn_train_step(eng.h, C.byref(a), ws.data_ptr(), need - 1, None) == 1003
    assert L.lib().abd_rnn_forward(eng.h, C.byref(a), ws.data_ptr(), 16, None) == 1003
    with pytest.raises(L.AbdError):
        T.rnn_train_step(m, x, None, None, None, None)   # no labels
    with pytest.raises(L.AbdError):
        m(x.cpu())
    with pytest.raises(ValueError):
        m(x[..., :-1].contiguous())


def test_opcheck(dev):
    name = "tiny"
    B, Tn, Fd, K, _ = rc.CASES[name]
    x, y, ind = inputs(name, dev)
    m = build(name, dev)
    eng = m.engine(x)
    eng.exp_avg = torch.zeros_like(eng.params)
    eng.exp_avg_sq = torch.zeros_like(eng.params)
    torch.library.opcheck(torch.ops.abd.rnn_eval.default, (x, eng.params, K))
    mt = metrics_buf(dev)
    torch.library.opcheck(torch.ops.abd.rnn_eval_metrics.default, (x, eng.params, K, y, ind, mt))
    args = (x, y, ind, eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq, mt, K, 1, 1e-4, 0.9, 0.999, 1e-8)
    torch.library.opcheck(torch.ops.abd.rnn_train_step.default, args)


def test_bound_model_checkpoint_reloads(dev, tmp_path):
    """After engine() the parameters are views of the flat buffer: the reference-format checkpoint of such a
    model, and torch.save of the module itself, reload to the same state and the same logits."""
    from conftest import load_dropin_checkpoint
    name = "tiny"
    x, y, ind = inputs(name, dev)
    m = build(name, dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=rc.LR)
    m.engine(x)
    T.rnn_train_step(m, x, y, ind, T.AdamBinding(m, opt), None)   # bound, trained one step
    assert m._bound(m._engine)
    m.eval()
    with torch.no_grad():
        want = m(x)
    T.save_reference_checkpoint(m, str(tmp_path / "ref.pt"))
    torch.save(m, str(tmp_path / "whole.pt"))
    back = [load_dropin_checkpoint(str(tmp_path / "ref.pt"), map_location=dev),
            torch.load(str(tmp_path / "whole.pt"), map_location=dev, weights_only=False)]
    sd = m.state_dict()
    for b in back:
        assert type(b).__name__ == "RNN" and b._engine is None
        assert (b.hidden_size, b.num_layers) == (768, 3)
        bsd = b.state_dict()
        assert list(bsd) == list(sd) and all(torch.equal(bsd[k], sd[k]) for k in sd)
        lo = m._engine.params.data_ptr()
        hi = lo + 4 * m._engine.n
        assert all(p.is_contiguous() and not lo <= p.data_ptr() < hi for p in b.parameters())   # no alias of m
        b.eval()
        with torch.no_grad():
            assert torch.equal(b(x), want)
    assert m._bound(m._engine)   # saving left the model bound


DROPIN_SCRIPT = r'''
import json, sys
import torch, torch.nn as nn, torch.optim as optim, torch.utils.data as Data
from prepare_dataset import BDDataset
from utils.random_tools import fix_random
from utils.training_tools import train, test, EarlyStoppingModel
from utils.models import RNN                     # ultrasonic.py: --model RNN

fix_random()
model = RNN(10, 13)                              # num_classes, time_len = n_mfcc
device = torch.device("cuda")
model.to(device)
criterion = nn.CrossEntropyLoss()
optimizer = optim.Adam(model.parameters(), lr=1e-4)
g = torch.Generator().manual_seed(1)
y = torch.randint(0, 10, (96,), generator=g)
x = torch.randn((96, 1, 8, 13), generator=g) + 0.5 * y[:, None, None, None].float()   # label-dependent level
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
json.dump({"hist": hist, "cls": type(model).__module__, "file": sys.modules["utils.models"].__file__,
           "ref_loaded": "utils._reference_models" in sys.modules}, open(sys.argv[1], "w"))
'''


def test_attack_script_shape_runs_through_the_dropin(dev, tmp_path):
    """An attack-script-shaped run (``--model RNN``: model from utils.models, train / test / EarlyStoppingModel
    from utils.training_tools) under ``python -m abd_amd.run`` trains through libabd, and its checkpoint reloads."""
    import json
    import os
    import subprocess
    import sys
    from conftest import load_dropin_checkpoint
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (tmp_path / "ultrasonic_like.py").write_text(DROPIN_SCRIPT)
    out = tmp_path / "res.json"
    r = subprocess.run([sys.executable, "-m", "abd_amd.run", "ultrasonic_like.py", str(out)], cwd=tmp_path,
                       env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(out.read_text())
    assert res["cls"] == "abd_amd.models_rnn" and "dropin" in res["file"] and not res["ref_loaded"]
    h = np.array(res["hist"])
    assert np.all(np.isfinite(h)) and h[-1, 0] < h[0, 0]          # the train loss falls
    final = torch.load(str(tmp_path / "final.pt"), weights_only=True)
    ck = load_dropin_checkpoint(str(tmp_path / "checkpoint.pt"), map_location=dev)
    assert type(ck).__name__ == "RNN"
    assert list(ck.state_dict()) == list(final["sd"])
    ck.eval()
    with torch.no_grad():
        yv = ck(torch.zeros((2, 1, 8, 13), device=dev))
    assert yv.shape == (2, 10) and torch.isfinite(yv).all() and torch.isfinite(final["out"]).all()
