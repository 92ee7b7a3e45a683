"""GPU: lstmwithattention on libabd against the float64 restatement of tests/lstm_attention_cases.py.

Bounds: 1e-4 relative to the largest magnitude of the compared tensor (the project's fp32 bound; the
float32 CPU run of the restatement stays within 1e-5, tests/test_lstm_attention_cpu.py), counters exact.
Measured distances are printed before each assertion (profiles/lstm_attention/parity.md records them).
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.utils.data as Data

import abd_amd
from abd_amd import _lib as L, training as T
from abd_amd.models_lstm import lstmwithattention, tile_rows
import lstm_attention_cases as lc

pytestmark = pytest.mark.gpu
TOL = 1e-4
GUARD = 8 << 20
PAT = 0xA5
CASES = list(lc.CASES)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    assert tile_rows() == lc.TILE   # the ragged_tiles case is sized from the kernel's tile
    return torch.device("cuda", 0)


def build(name, dev):
    B, Tn, Fd, K, _ = lc.geometry(name)
    m = lstmwithattention(K, Fd, Tn)
    m.load_state_dict({k: torch.tensor(v) for k, v in lc.make_state(name).items()})
    return m.to(dev)


def inputs(name, dev):
    x, y, ind, mask = lc.make_inputs(name)
    return (torch.tensor(x, device=dev), torch.tensor(y, device=dev), torch.tensor(ind, device=dev),
            torch.tensor(mask, device=dev))


def metrics_buf(dev):
    return torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)


def counters(logits, y, ind):
    pred = logits.argmax(1)
    return (len(y), int((pred == y).sum()), int((ind == 1).sum()), int(((ind == 1) & (pred == y)).sum()), 1)


def check(what, got, ref, tol=TOL):
    e = lc.rel_err(got.detach().cpu(), ref)
    print(f"{what}: {e:.3e}")
    assert e < tol, (what, e)


def saved(m, B, name, shape):
    eng = m._engine
    off = L.lib().abd_lstmattn_workspace_offset(eng.h, B, name.encode())
    assert off >= 0
    n = int(np.prod(shape))
    return eng._ws[off:off + 4 * n].view(torch.float32).view(shape).clone()


@pytest.mark.parametrize("name", CASES)
def test_forward_parity_counters_and_running_statistics(dev, name):
    B, Tn, Fd, K, _ = lc.CASES[name]
    ref = lc.run_case(name)
    x, y, ind, mask = inputs(name, dev)
    m = build(name, dev).eval()
    with torch.no_grad():
        ev = m(x)
    check(f"{name} eval logits", ev, ref["eval_logits"])
    eng = m._engine
    mt = metrics_buf(dev)
    ev2 = torch.ops.abd.lstmattn_eval_metrics(x, eng.params, eng.running, K, y, ind, mt)
    assert torch.equal(ev2, ev)
    loss, *cnt = T.read_metrics(mt)
    print(f"{name} eval loss: {abs(loss - float(ref['eval_loss'])) / float(ref['eval_loss']):.3e}")
    assert abs(loss - float(ref["eval_loss"])) < TOL * float(ref["eval_loss"])
    assert tuple(cnt) == counters(ref["eval_logits"], y.cpu(), ind.cpu())
    # train mode, host mask
    m.train()
    mt = metrics_buf(dev)
    out = torch.empty((B, K), device=dev)
    T.lstm_train_step(m, x, y, ind, None, mt, mask=mask, do_update=False, logits_out=out)
    check(f"{name} train logits", out, ref["train_logits"])
    loss, *cnt = T.read_metrics(mt)
    print(f"{name} train loss: {abs(loss - float(ref['loss'])) / float(ref['loss']):.3e}")
    assert abs(loss - float(ref["loss"])) < TOL * float(ref["loss"])
    assert tuple(cnt) == counters(ref["train_logits"], y.cpu(), ind.cpu())
    sd = m.state_dict()
    for n in lc.BUFFERS:
        if n.endswith("num_batches_tracked"):
            assert int(sd[n]) == int(ref["running"][n]), n
        else:
            check(f"{name} {n}", sd[n], ref["running"][n])
    # device-generated mask, read back and replayed on the host
    mo = torch.full((B, 64), 7, dtype=torch.uint8, device=dev)
    T.lstm_train_step(m, x, y, ind, None, None, mask_out=mo, do_update=False, logits_out=out, seed=5)
    assert int(mo.max()) <= 1
    r = lc.Restated(lc.make_state(name))
    with torch.no_grad():
        want = r(torch.tensor(lc.make_inputs(name)[0], dtype=torch.float64), True, mo.cpu())
    check(f"{name} train logits (device mask)", out, want)


@pytest.mark.parametrize("name", CASES)
def test_gradients_and_saved_states(dev, name):
    B, Tn, Fd, K, _ = lc.CASES[name]
    ref = lc.run_case(name)
    x, y, ind, mask = inputs(name, dev)
    m = build(name, dev).train()
    T.lstm_train_step(m, x, y, ind, None, None, mask=mask, do_update=False)
    eng = m._engine
    g_step = eng.grads.clone()
    for n, g in zip(lc.PARAM_ORDER, eng.views(g_step)):
        check(f"{name} grad {n}", g, ref["grads"][n])
    # saved h / c of both layers and directions: the reverse direction's placement
    for layer in (1, 2):
        yv = saved(m, B, f"y{layer}", (B, Tn, 128))
        check(f"{name} h{layer} forward", yv[..., :64], ref[f"h{layer}"][0])
        check(f"{name} h{layer} reverse", yv[..., 64:], ref[f"h{layer}"][1])
        cv = saved(m, B, f"c{layer}", (2, B, Tn, 64))
        check(f"{name} c{layer}", cv, ref[f"c{layer}"])
    # the same step twice: bit-equal
    T.lstm_train_step(m, x, y, ind, None, None, mask=mask, do_update=False)
    assert torch.equal(eng.grads, g_step)


def _autograd_and_step(dev, name):
    """Gradients of the autograd path (abd_lstmattn_forward, torch's CrossEntropyLoss, abd_lstmattn_backward)
    and of the fused step under the same CPU-drawn mask, with the restatement's for that mask."""
    B, Tn, Fd, K, _ = lc.geometry(name)
    x, y, ind, _ = inputs(name, dev)
    m2 = build(name, dev).train()
    m2.set_dropout_source("torch_cpu")
    torch.manual_seed(31)
    cpu_mask = torch.empty((B, 64)).bernoulli_(0.5).to(torch.uint8)
    torch.manual_seed(31)
    loss = nn.CrossEntropyLoss()(m2(x), y)
    loss.backward()
    m3 = build(name, dev).train()
    T.lstm_train_step(m3, x, y, ind, None, None, mask=cpu_mask.to(dev), do_update=False)
    r = lc.Restated(lc.make_state(name))
    xl = torch.tensor(lc.make_inputs(name)[0], dtype=torch.float64)
    nn.functional.cross_entropy(r(xl, True, cpu_mask), y.cpu()).backward()
    return [p.grad.reshape(-1) for p in m2._param_list()], m3._engine.views(m3._engine.grads), r.grads()


@pytest.mark.parametrize("name", CASES)
def test_backward_entry_parity(dev, name):
    auto, _, want = _autograd_and_step(dev, name)
    for n, g in zip(lc.PARAM_ORDER, auto):
        check(f"{name} backward grad {n}", g, want[n])


@pytest.mark.parametrize("name", CASES)
def test_autograd_path_bit_equal_to_train_step(dev, name):
    """torch's CrossEntropyLoss backward and the step's own d(logits) kernel use the same arithmetic (torch's
    log_softmax / nll_loss backward formulas, the same exp and log routines, the same reduction order for
    K <= 64), so the two paths agree bit for bit."""
    auto, step, _ = _autograd_and_step(dev, name)
    worst = max(lc.rel_err(a, s) for a, s in zip(auto, step))
    print(f"{name} autograd vs train_step: worst relative difference {worst:.3e}")
    for n, a, s in zip(lc.PARAM_ORDER, auto, step):
        assert torch.equal(a, s), n


@pytest.mark.parametrize("name", ["tiny", "ragged_tiles"])
def test_fused_adam_equals_split_update(dev, name):
    x, y, ind, mask = inputs(name, dev)
    ms = [build(name, dev).train() for _ in range(3)]
    opts = [torch.optim.Adam(m.parameters(), lr=lc.LR) for m in ms]
    adams = []
    for m, o in zip(ms, opts):
        m.engine(x)
        adams.append(T.AdamBinding(m, o))
    T.lstm_train_step(ms[0], x, y, ind, adams[0], None, mask=mask, do_update=True)
    T.lstm_train_step(ms[1], x, y, ind, adams[1], None, mask=mask, do_update=False)
    T.apply_adam(ms[1], adams[1], dev)
    T.lstm_train_step(ms[2], x, y, ind, adams[2], None, mask=mask, do_update=True)
    for a, b in ((ms[0], ms[1]), (ms[0], ms[2])):
        assert torch.equal(a._engine.params, b._engine.params)
        assert torch.equal(a._engine.exp_avg, b._engine.exp_avg)
        assert torch.equal(a._engine.exp_avg_sq, b._engine.exp_avg_sq)
    assert not torch.equal(ms[0]._engine.params, torch.cat([torch.tensor(lc.make_state(name)[n]).reshape(-1)
                                                            for n in lc.PARAM_ORDER]).to(dev))


class DictSet(Data.Dataset):
    def __init__(self, x, y, ind):
        self.x, self.y, self.ind = x, y, ind

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return {"mfcc": self.x[i], "label": self.y[i], "poison_indicator": self.ind[i]}


def test_training_loop_equals_manual_loop(dev):
    name = "ragged_tiles"
    B, Tn, Fd, K, _ = lc.CASES[name]
    xn, yn, indn, _ = lc.make_inputs(name)
    xc, yc, ic = torch.tensor(xn), torch.tensor(yn), torch.tensor(indn)
    bd = Data.DataLoader(DictSet(xc, yc, ic), batch_size=10, shuffle=False)     # batches of 10 and 7
    clean = Data.DataLoader(Data.TensorDataset(xc, yc), batch_size=10, shuffle=False)
    crit = nn.CrossEntropyLoss()
    a, b = build(name, dev), build(name, dev)
    for m in (a, b):
        m.set_dropout_source("torch_cpu")
    oa = torch.optim.Adam(a.parameters(), lr=lc.LR)
    ob = torch.optim.Adam(b.parameters(), lr=lc.LR)
    torch.manual_seed(7)
    got = T.train(a, bd, dev, oa, crit)
    # manual loop over the entry points
    torch.manual_seed(7)
    b.train()
    mt = metrics_buf(dev)
    adam = None
    first_loss = None
    for item in bd:   # iterating the loader draws its base seed from the CPU generator, as train() does
        x, y, ind = item["mfcc"].to(dev), item["label"].to(dev), item["poison_indicator"].to(dev)
        if adam is None:
            b.engine(x)
            adam = T.AdamBinding(b, ob)
        T.lstm_train_step(b, x, y, ind, adam, mt)
        if first_loss is None:
            first_loss = T.read_metrics(mt)[0]
    ls, tot, cor, pt, asr, nb = T.read_metrics(mt)
    assert got == (ls / nb, 100.0 * cor / tot, 100 * asr / pt)
    assert torch.equal(a._engine.params, b._engine.params)
    # first batch against the restatement, with the mask the CPU generator gave
    torch.manual_seed(7)
    iter(bd)   # the loader's base-seed draw
    m0 = torch.empty((10, 64)).bernoulli_(0.5).to(torch.uint8)
    r = lc.Restated(lc.make_state(name))
    want = float(nn.functional.cross_entropy(r(xc[:10].double(), True, m0), yc[:10]))
    print(f"first batch loss: {abs(first_loss - want) / want:.3e}")
    assert abs(first_loss - want) < TOL * want
    # optimizer state synced, p.grad exposed
    for p in a.parameters():
        assert float(oa.state[p]["step"]) == 2.0
        assert oa.state[p]["exp_avg"].data_ptr() >= a._engine.exp_avg.data_ptr()
        assert p.grad is not None and p.grad.shape == p.shape
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in a._param_list()]), a._engine.grads)
    # test() / clean_test() / clean_train() against the ops
    got_t = T.test(a, dev, clean, bd, crit)
    b.eval()
    eng = b._engine
    mc, mb = metrics_buf(dev), metrics_buf(dev)
    for lo, hi in ((0, 10), (10, B)):
        x, y, ind = xc[lo:hi].to(dev), yc[lo:hi].to(dev), ic[lo:hi].to(dev)
        torch.ops.abd.lstmattn_eval_metrics(x, eng.params, eng.running, K, y, None, mc)
        torch.ops.abd.lstmattn_eval_metrics(x, eng.params, eng.running, K, y, ind, mb)
    cl, ct, cc, _, _, nc = T.read_metrics(mc)
    bl, _, _, pt, ah, nbb = T.read_metrics(mb)
    assert got_t == (100 * cc / ct, 100 * ah / pt, cl / nc, bl / nbb)
    assert T.clean_test(a, dev, clean, crit) == (cl / nc, 100 * cc / ct)
    torch.manual_seed(9)
    got_c = T.clean_train(a, clean, dev, oa, crit)
    torch.manual_seed(9)
    b.train()
    mt = metrics_buf(dev)
    for xb, yb in clean:
        T.lstm_train_step(b, xb.to(dev), yb.to(dev), None, adam, mt)
    ls, tot, cor, _, _, nb = T.read_metrics(mt)
    assert got_c == (ls / nb, 100.0 * cor / tot)
    assert torch.equal(a._engine.params, b._engine.params)


def test_guards_and_refusals(dev):
    name = "tiny"
    B, Tn, Fd, K, _ = lc.CASES[name]
    x, y, ind, mask = inputs(name, dev)
    m = build(name, dev).train()
    eng = m.engine(x)
    need = L.lib().abd_lstmattn_workspace_bytes(eng.h, B)
    eng._ws = torch.full((need + GUARD,), PAT, dtype=torch.uint8, device=dev)
    out = torch.full((B + 4, K), float("nan"), device=dev)
    mo = torch.full((B + 4, 64), PAT, dtype=torch.uint8, device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=lc.LR)
    T.lstm_train_step(m, x, y, ind, T.AdamBinding(m, opt), metrics_buf(dev), mask_out=mo, logits_out=out)
    torch.cuda.synchronize()
    assert int((eng._ws[need:] != PAT).sum()) == 0
    assert torch.isnan(out[B:]).all() and torch.isfinite(out[:B]).all()
    assert int((mo[B:] != PAT).sum()) == 0
    # a workspace that is too small
    a = m._args(eng, x, B)
    a.labels = y.data_ptr()
    assert L.lib().abd_lstmattn_train_step(eng.h, C.byref(a), eng._ws.data_ptr(), need - 1, None) == 1003
    assert L.lib().abd_lstmattn_forward(eng.h, C.byref(a), 1, eng._ws.data_ptr(), 16, None) == 1003
    # no labels
    with pytest.raises(L.AbdError):
        T.lstm_train_step(m, x, None, None, None, None)
    with pytest.raises(L.AbdError):
        m.set_gemm_precision("bf16")
    with pytest.raises(L.AbdError):
        m(x.cpu())
    with pytest.raises(ValueError):
        m(x[:, :, :-1].contiguous())


def test_opcheck(dev):
    name = "tiny"
    B, Tn, Fd, K, _ = lc.CASES[name]
    x, y, ind, mask = inputs(name, dev)
    m = build(name, dev)
    eng = m.engine(x)
    eng.exp_avg = torch.zeros_like(eng.params)
    eng.exp_avg_sq = torch.zeros_like(eng.params)
    torch.library.opcheck(torch.ops.abd.lstmattn_eval.default, (x, eng.params, eng.running, K))
    mt = metrics_buf(dev)
    torch.library.opcheck(torch.ops.abd.lstmattn_eval_metrics.default, (x, eng.params, eng.running, K, y, ind, mt))
    args = (x, y, ind, eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq, eng.running, eng.nbt, mt, K, 1,
            1e-4, 0.9, 0.999, 1e-8, 7, 0, mask)
    torch.library.opcheck(torch.ops.abd.lstmattn_train_step.default, args)


def test_bound_model_checkpoint_reloads(dev, tmp_path):
    """After engine() the parameters are views of the flat buffer: the reference-format checkpoint of such a
    model, and torch.save of the module itself, reload to the same state and the same eval logits."""
    from conftest import load_dropin_checkpoint
    name = "tiny"
    x, y, ind, mask = inputs(name, dev)
    m = build(name, dev).train()
    opt = torch.optim.Adam(m.parameters(), lr=lc.LR)
    m.engine(x)
    T.lstm_train_step(m, x, y, ind, T.AdamBinding(m, opt), None, mask=mask)   # bound, trained one step
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
        assert type(b).__name__ == "lstmwithattention" and b._engine is None
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
from utils.models import lstmwithattention      # ultrasonic.py:147-148: --model lstmwithattention

fix_random()
model = lstmwithattention(10, 13, 32)            # classes, time_len = n_mfcc, seq_len
device = torch.device("cuda")
model.to(device)
criterion = nn.CrossEntropyLoss()
optimizer = optim.Adam(model.parameters(), lr=1e-3)
g = torch.Generator().manual_seed(1)
y = torch.randint(0, 10, (96,), generator=g)
x = 20 * torch.randn((96, 1, 32, 13), generator=g) + 6 * y[:, None, None, None].float()   # label-dependent level
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
    """An attack-script-shaped run (``--model lstmwithattention``: model from utils.models, train / test /
    EarlyStoppingModel from utils.training_tools) under ``python -m abd_amd.run`` trains through libabd, and
    its checkpoint reloads."""
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
    assert res["cls"] == "abd_amd.models_lstm" and "dropin" in res["file"] and not res["ref_loaded"]
    h = np.array(res["hist"])
    assert np.all(np.isfinite(h)) and h[-1, 0] < h[0, 0]          # the train loss falls
    final = torch.load(str(tmp_path / "final.pt"), weights_only=True)
    ck = load_dropin_checkpoint(str(tmp_path / "checkpoint.pt"), map_location=dev)
    assert type(ck).__name__ == "lstmwithattention"
    assert list(ck.state_dict()) == list(final["sd"])
    ck.eval()
    with torch.no_grad():
        y = ck(torch.zeros((2, 1, 32, 13), device=dev))
    assert y.shape == (2, 10) and torch.isfinite(y).all() and torch.isfinite(final["out"]).all()
