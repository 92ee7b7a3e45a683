"""GPU: lstmwithattention across the shape range abd_lstmattn_create accepts (lc.ENVELOPE), against the float64
restatement of tests/lstm_attention_cases.py.

Each case is the smallest shape that reaches a loop bound or a cap of csrc/lstm_attn.hip that the four cases of
tests/test_gpu_lstm_attention.py leave alone (T = 1, T < 5, T > 256, T = 1024, F = 1 / 33 / 128, K = 1 / 70 / 200,
B = 600).  Bounds: 1e-4 relative to the largest magnitude of the compared tensor, except where
lc.ENVELOPE_BOUNDS records ten times a measured float32-CPU distance; counters exact.  The conditions these
rest on are asserted on the CPU (tests/test_lstm_attention_cpu.py).  Measured distances are printed before each
assertion (profiles/lstm_attention/parity.md, "Accepted shape range").
"""
import ctypes as C

import pytest
import torch
import torch.nn as nn

from abd_amd import _lib as L, ops, training as T   # noqa: F401  (ops registers torch.ops.abd)
import lstm_attention_cases as lc
import test_gpu_lstm_attention as g

pytestmark = pytest.mark.gpu
TOL = g.TOL
ENVELOPE = list(lc.ENVELOPE)
dev = g.dev


def loss_check(what, got, ref):
    ref = float(ref)
    if ref == 0.0:
        print(f"{what}: {abs(got):.3e} (reference 0)")
        assert got == 0.0, what
        return
    print(f"{what}: {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) < TOL * ref, what


@pytest.mark.parametrize("name", ENVELOPE)
def test_forward_counters_and_running_statistics(dev, name):
    B, Tn, Fd, K, _ = lc.ENVELOPE[name]
    ref = lc.run_case(name)
    x, y, ind, mask = g.inputs(name, dev)
    m = g.build(name, dev).eval()
    eng = m.engine(x)
    mt = g.metrics_buf(dev)
    ev = torch.ops.abd.lstmattn_eval_metrics(x, eng.params, eng.running, K, y, ind, mt)
    g.check(f"{name} eval logits", ev, ref["eval_logits"])
    loss, *cnt = T.read_metrics(mt)
    loss_check(f"{name} eval loss", loss, ref["eval_loss"])
    assert tuple(cnt) == g.counters(ref["eval_logits"], y.cpu(), ind.cpu())
    m.train()
    mt = g.metrics_buf(dev)
    out = torch.empty((B, K), device=dev)
    T.lstm_train_step(m, x, y, ind, None, mt, mask=mask, do_update=False, logits_out=out)
    g.check(f"{name} train logits", out, ref["train_logits"])
    loss, *cnt = T.read_metrics(mt)
    loss_check(f"{name} train loss", loss, ref["loss"])
    assert tuple(cnt) == g.counters(ref["train_logits"], y.cpu(), ind.cpu())
    if K == 1:
        assert cnt[1] == B   # one class: every prediction is right
    sd = m.state_dict()
    for n in lc.BUFFERS:
        if n.endswith("num_batches_tracked"):
            assert int(sd[n]) == int(ref["running"][n]), n
        else:
            g.check(f"{name} {n}", sd[n], ref["running"][n])


@pytest.mark.parametrize("name", ENVELOPE)
def test_gradients_and_saved_states(dev, name):
    B, Tn, Fd, K, _ = lc.ENVELOPE[name]
    ref = lc.run_case(name)
    x, y, ind, mask = g.inputs(name, dev)
    m = g.build(name, dev).train()
    m.engine(x).grads.fill_(float("nan"))   # every gradient element has to be written
    T.lstm_train_step(m, x, y, ind, None, None, mask=mask, do_update=False)
    eng = m._engine
    for n, gr in zip(lc.PARAM_ORDER, eng.views(eng.grads)):
        if K == 1:
            worst = float(gr.abs().max())
            print(f"{name} grad {n}: {worst:.3e} (reference 0)")
            assert worst == 0.0, n
        else:
            g.check(f"{name} grad {n}", gr, ref["grads"][n], lc.grad_bound(name, n, TOL))
    for layer in (1, 2):
        yv = g.saved(m, B, f"y{layer}", (B, Tn, 128))
        g.check(f"{name} h{layer} forward", yv[..., :64], ref[f"h{layer}"][0])
        g.check(f"{name} h{layer} reverse", yv[..., 64:], ref[f"h{layer}"][1])
        cv = g.saved(m, B, f"c{layer}", (2, B, Tn, 64))
        g.check(f"{name} c{layer}", cv, ref[f"c{layer}"])


@pytest.mark.parametrize("name", ["big_batch", "strided_head"])
def test_same_step_twice_is_bit_equal(dev, name):
    """The split-K slices (ksplit 64 on big_batch) and the two-stage column sums are summed in a fixed order."""
    x, y, ind, mask = g.inputs(name, dev)
    m = g.build(name, dev).train()
    T.lstm_train_step(m, x, y, ind, None, None, mask=mask, do_update=False)
    first = m._engine.grads.clone()
    m._engine.grads.zero_()
    T.lstm_train_step(m, x, y, ind, None, None, mask=mask, do_update=False)
    assert torch.isfinite(first).all() and torch.equal(m._engine.grads, first)


@pytest.mark.parametrize("name", ["wide_classes", "ragged_feature"])
def test_autograd_path_beyond_one_wave_of_classes(dev, name):
    """model(x) + CrossEntropyLoss + backward() for K > 64, where torch's reduction order over the classes is no
    longer the step's: within the bound of the restatement; the difference to the fused step is reported only."""
    auto, step, want = g._autograd_and_step(dev, name)
    worst = max(lc.rel_err(a, s) for a, s in zip(auto, step))
    print(f"{name} autograd vs train_step: worst relative difference {worst:.3e}")
    for n, a in zip(lc.PARAM_ORDER, auto):
        g.check(f"{name} backward grad {n}", a, want[n], lc.grad_bound(name, n, TOL))


def test_argmax_ties_take_the_first_index(dev):
    """K = 200, the maximum at classes 69, 70 and 133: 69 and 133 are the same lane of ce_kernel (133 = 69 + 64),
    70 the next one.  output.weight is zero, so the logits are the bias bit for bit; torch's argmax is 69."""
    name = "wide_classes"
    B, Tn, Fd, K, _ = lc.ENVELOPE[name]
    x, _, _, mask = g.inputs(name, dev)
    st = lc.make_state(name)
    st["output.weight"][:] = 0.0
    bias = -1.0 - 0.25 * (torch.arange(K) % 7).float()
    bias[[69, 70, 133]] = 2.0
    st["output.bias"] = bias.numpy()
    m = g.build(name, dev)
    m.load_state_dict({k: torch.tensor(v) for k, v in st.items()})
    assert int(bias.argmax()) == 69
    ind = torch.ones(B, dtype=torch.int64, device=dev)
    for label, hits in ((69, B), (70, 0), (133, 0)):
        y = torch.full((B,), label, dtype=torch.int64, device=dev)
        m.eval()
        eng = m.engine(x)
        mt = g.metrics_buf(dev)
        ev = torch.ops.abd.lstmattn_eval_metrics(x, eng.params, eng.running, K, y, ind, mt)
        assert torch.equal(ev.cpu(), bias.expand(B, K))
        assert T.read_metrics(mt)[1:] == (B, hits, B, hits, 1), ("eval", label)
        m.train()
        mt = g.metrics_buf(dev)
        out = torch.empty((B, K), device=dev)
        T.lstm_train_step(m, x, y, ind, None, mt, mask=mask, do_update=False, logits_out=out)
        assert torch.equal(out.cpu(), bias.expand(B, K))
        assert T.read_metrics(mt)[1:] == (B, hits, B, hits, 1), ("train", label)


@pytest.mark.parametrize("name", ["big_batch", "cap_seq", "wide_classes"])
def test_workspace_and_output_bounds(dev, name):
    B, Tn, Fd, K, _ = lc.ENVELOPE[name]
    x, y, ind, mask = g.inputs(name, dev)
    m = g.build(name, dev).train()
    eng = m.engine(x)
    need = L.lib().abd_lstmattn_workspace_bytes(eng.h, B)
    eng._ws = torch.full((need + g.GUARD,), g.PAT, dtype=torch.uint8, device=dev)
    out = torch.full((B + 4, K), float("nan"), device=dev)
    mo = torch.full((B + 4, 64), g.PAT, dtype=torch.uint8, device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=lc.LR)
    before = eng.params.clone()
    T.lstm_train_step(m, x, y, ind, T.AdamBinding(m, opt), g.metrics_buf(dev), mask_out=mo, logits_out=out)
    torch.cuda.synchronize()
    assert int((eng._ws[need:] != g.PAT).sum()) == 0
    assert torch.isnan(out[B:]).all() and torch.isfinite(out[:B]).all()
    assert int((mo[B:] != g.PAT).sum()) == 0 and int(mo[:B].max()) <= 1
    assert torch.isfinite(eng.params).all() and not torch.equal(eng.params, before)
    a = m._args(eng, x, B)
    a.labels = y.data_ptr()
    assert L.lib().abd_lstmattn_train_step(eng.h, C.byref(a), eng._ws.data_ptr(), need - 1, None) == 1003
    assert L.lib().abd_lstmattn_forward(eng.h, C.byref(a), 1, eng._ws.data_ptr(), need - 1, None) == 1003


def test_device_mask_on_a_big_batch(dev):
    name = "big_batch"
    B, Tn, Fd, K, _ = lc.ENVELOPE[name]
    x, y, ind, _ = g.inputs(name, dev)
    m = g.build(name, dev).train()
    mo = torch.full((B, 64), 7, dtype=torch.uint8, device=dev)
    out = torch.empty((B, K), device=dev)
    T.lstm_train_step(m, x, y, ind, None, None, mask_out=mo, do_update=False, logits_out=out, seed=5)
    assert int(mo.max()) <= 1
    rate = float(mo.float().mean())
    print(f"{name} keep rate over {B * 64} draws: {rate:.4f}")
    assert abs(rate - 0.5) < 0.013   # five standard deviations of a fair coin: 5 * 0.5 / sqrt(38400)
    r = lc.Restated(lc.make_state(name))
    with torch.no_grad():
        want = r(torch.tensor(lc.make_inputs(name)[0], dtype=torch.float64), True, mo.cpu())
    g.check(f"{name} train logits (device mask)", out, want)


def test_create_and_train_refusals(dev):
    lib = L.lib()
    h = C.c_void_p()
    for geo in ((0, 13, 10), (1025, 13, 10), (32, 0, 10), (32, 129, 10), (32, 13, 0), (32, 13, 4097)):
        assert lib.abd_lstmattn_create(*geo, C.byref(h)) == 1002, geo
    assert lib.abd_lstmattn_create(1, 1, 3, C.byref(h)) == 0
    x = torch.zeros((1, 1, 1, 1), device=dev)
    a = L.LstmAttnArgs()
    a.x = a.labels = a.params = a.grads = a.running = x.data_ptr()   # refused before anything is launched
    a.batch = 1
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    assert lib.abd_lstmattn_train_step(h, C.byref(a), ws.data_ptr(), ws.numel(), None) == 1001
    assert lib.abd_lstmattn_forward(h, C.byref(a), 1, ws.data_ptr(), ws.numel(), None) == 1001
    lib.abd_lstmattn_destroy(h)
    with pytest.raises(L.AbdError):
        nn.Module.train(g.lstmwithattention(3, 1, 1).to(dev))(x)
