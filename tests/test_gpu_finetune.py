"""GPU: the regularised fine-tuning step (csrc/finetune.hip, torch.ops.abd.sgd / segment_norms / perturb /
smallcnn_finetune_reg_step, abd_amd.defense.finetune_reg_epoch / finetune_epoch).

1. segment norms against float64 numpy (2^-22: a double accumulation rounded once to fp32, plus a sqrt)
2. perturb / SGD against float64 evaluated from the device's own fp32 inputs (1e-6 normalised, the bound
   test_gpu_smallcnn.py sets for the Adam arithmetic) and against torch.optim.SGD on CPU copies
3. the composite step against the same step composed from the entry points that existed before it
   (training.train_step(do_update=False), hip_forward(train=True)) plus the new elementwise ops: bit
   equality when the no-update train step is itself bit-reproducible, else its run-to-run spread + 1e-6
4. the composite's log-probs and loss against the float64 restatement (finetune_cases.RegTrainer, pinned
   to the reference's own function by tests/golden/finetune_golden.npz) at the suite's RTOL = 1e-4
5. the Python layer
Set ABD_PARITY_OUT to a file name to have the observed figures of 3 and 4 appended to it.
"""
import os

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D, models as M, training as T
from finetune_cases import RegTrainer, case_inputs, draw_masks, segment_norms
from golden_inputs import rng
from oracle import smallcnn as oc

pytestmark = pytest.mark.gpu
RTOL = 1e-4
ELEM_TOL = 1e-6
NORM_TOL = 2.0 ** -22
R, ALPHA, LR, MU = 0.05, 0.7, 0.01, 0.9


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    from abd_amd import ops  # noqa: F401
    return torch.device("cuda", 0)


def note(line):
    print(line)
    out = os.environ.get("ABD_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def nrel(a, b):
    a = np.asarray(a.cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def build(st, K, dev, prec="f32split", nonce=None):
    m = M.smallcnn(K, st["fc1.weight"].shape[1])
    m.load_state_dict({k: torch.tensor(v) for k, v in st.items()})
    m = m.to(dev).set_gemm_precision(prec).train()
    if nonce is not None:
        m._dropout_nonce = nonce
    return m


def dev_masks(masks, dev):
    """[(m1, m2)] x 3 numpy -> ((3, B, flat), (3, B, 128)) uint8 device tensors."""
    return (torch.tensor(np.stack([m[0] for m in masks]), device=dev),
            torch.tensor(np.stack([m[1] for m in masks]), device=dev))


# ------------------------------------------------------------------ 1. segment norms
def magnitudes(r, n):
    """fp32 values over several decades, so the squares' sum is not dominated by rounding luck."""
    return (r.standard_normal(n) * np.exp(r.uniform(-6, 3, n))).astype(np.float32)


def test_segment_norms_synthetic(dev):
    lens = [1, 3, 64, 2049, 70001]
    offs = np.concatenate([[1], 1 + np.cumsum(lens)]).astype(np.int64)      # element offset 1: nothing 16-byte aligned
    host = magnitudes(rng(11), int(offs[-1]) + 7)
    buf = torch.tensor(host, device=dev)
    assert buf.data_ptr() % 16 == 0
    n1 = torch.ops.abd.segment_norms(buf, offs.tolist())
    n2 = torch.ops.abd.segment_norms(buf, offs.tolist())
    assert torch.equal(n1, n2)
    ref = segment_norms(host, offs)
    err = np.abs(n1.cpu().numpy().astype(np.float64) / ref - 1).max()
    print(f"segment norms: max rel err {err:.2e} (bound {NORM_TOL:.2e})")
    assert err <= NORM_TOL
    # the same segments through pointers at every 4-byte phase of a 16-byte line
    for shift in (1, 2, 3):
        view = torch.tensor(np.concatenate([np.zeros(shift, np.float32), host]), device=dev)[shift:]
        assert view.data_ptr() % 16 == 4 * shift
        v = torch.ops.abd.segment_norms(view, offs.tolist())
        assert np.abs(v.cpu().numpy().astype(np.float64) / ref - 1).max() <= NORM_TOL, shift


def test_segment_norms_model_tensors(dev):
    import ctypes as C
    h = C.c_void_p()
    assert L.lib().abd_smallcnn_create(32, 40, 35, 0, C.byref(h)) == 0
    off = (C.c_int64 * 17)()
    L.lib().abd_smallcnn_param_offsets(h, off)
    L.lib().abd_smallcnn_destroy(h)
    offs = list(off)
    assert offs[16] - offs[15] == 35 and len(offs) == 17                    # fc2.bias: 35 elements
    host = magnitudes(rng(12), offs[-1])
    buf = torch.tensor(host, device=dev)
    n1 = torch.ops.abd.segment_norms(buf, offs)
    assert torch.equal(n1, torch.ops.abd.segment_norms(buf, offs))
    ref = segment_norms(host, offs)
    assert np.abs(n1.cpu().numpy().astype(np.float64) / ref - 1).max() <= NORM_TOL


# ------------------------------------------------------------------ 2. perturb and SGD
def test_perturb(dev):
    lens = [1, 3, 64, 2049, 70001, 5]
    offs = np.concatenate([[1], 1 + np.cumsum(lens)]).astype(np.int64)
    n = int(offs[-1]) + 3
    r = rng(13)
    p = r.standard_normal(n).astype(np.float32)
    g = magnitudes(r, n)
    g[offs[2]:offs[3]] = 0.0                                               # an all-zero gradient tensor
    pd, gd = torch.tensor(p, device=dev), torch.tensor(g, device=dev)
    norms = torch.ops.abd.segment_norms(gd, offs.tolist())
    out = torch.ops.abd.perturb(pd, gd, norms, offs.tolist(), R).cpu().numpy()
    assert np.array_equal(out[:1], p[:1]) and np.array_equal(out[offs[-1]:], p[offs[-1]:])   # outside: copied
    nd = norms.cpu().numpy().astype(np.float64)
    assert nd[2] == 0.0
    for s in range(len(lens)):
        sl = slice(int(offs[s]), int(offs[s + 1]))
        if s == 2:
            assert np.isnan(out[sl]).all()                                  # 0 / 0, as grad / grad.norm() gives
            continue
        ref = p[sl].astype(np.float64) + R * (g[sl].astype(np.float64) / nd[s])
        assert np.isfinite(out[sl]).all()
        assert nrel(out[sl], ref) < ELEM_TOL, s
    # the scalar path (the three buffers at different phases of a 16-byte line) gives the same bits
    g2 = torch.tensor(np.concatenate([[0.0], g]).astype(np.float32), device=dev)[1:]
    assert g2.data_ptr() % 16 == 4
    out2 = torch.ops.abd.perturb(pd, g2, norms, offs.tolist(), R).cpu().numpy()
    assert np.array_equal(out2, out, equal_nan=True)


@pytest.mark.parametrize("n,shift", [(70001 + 2049, 0), (4099, 1)])
def test_sgd_three_steps_vs_torch(dev, n, shift):
    """Three abd::sgd steps from a zero buffer with the two-gradient blend, against torch.optim.SGD(momentum) on
    CPU copies fed the fp32 blend, and against float64 evaluated from the device's own fp32 inputs.
    shift = 1: views one element into their storage (no 16-byte alignment: the scalar kernel)."""
    r = rng(14 + shift)

    def on_dev(a):
        return torch.tensor(np.concatenate([np.zeros(shift, np.float32), a]), device=dev)[shift:]

    p0 = r.standard_normal(n).astype(np.float32)
    p = on_dev(p0)
    buf = on_dev(np.zeros(n, np.float32))
    gout = on_dev(np.zeros(n, np.float32))
    pc = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.SGD([pc], lr=LR, momentum=MU)
    p64, b64 = p0.astype(np.float64), np.zeros(n)
    for step in range(3):
        g1, g2 = magnitudes(r, n) * 1e-2, magnitudes(r, n) * 1e-2
        p_before, b_before = p.cpu().numpy().astype(np.float64), buf.cpu().numpy().astype(np.float64)
        torch.ops.abd.sgd(p, on_dev(g1), buf, gout, LR, MU, on_dev(g2), ALPHA)
        d64 = (1 - ALPHA) * g1.astype(np.float64) + ALPHA * g2.astype(np.float64)
        assert nrel(gout, d64) < ELEM_TOL
        nb = MU * b_before + d64                                            # one step from the device's own state
        assert nrel(buf, nb) < ELEM_TOL and nrel(p, p_before - LR * nb) < ELEM_TOL
        pc.grad = (1 - ALPHA) * torch.tensor(g1) + ALPHA * torch.tensor(g2)  # ft_reg.py:109 in fp32
        opt.step()
        b64 = MU * b64 + d64
        p64 = p64 - LR * b64
    assert nrel(buf, opt.state[pc]["momentum_buffer"]) < ELEM_TOL and nrel(p, pc.detach()) < ELEM_TOL
    assert nrel(buf, b64) < ELEM_TOL and nrel(p, p64) < ELEM_TOL
    # plain SGD: no buffer, no blend, no gradient output
    q = on_dev(p0)
    g = magnitudes(r, n)
    torch.ops.abd.sgd(q, on_dev(g), None, None, LR)
    assert nrel(q, p0.astype(np.float64) - LR * g.astype(np.float64)) < ELEM_TOL
    # grad_out may alias the second gradient (the composite leaves the blend in grads)
    ga, gb = on_dev(g), on_dev(p0)
    q2, b2 = on_dev(p0), on_dev(np.zeros(n, np.float32))
    L.check(L.lib().abd_sgd_f32(q2.data_ptr(), ga.data_ptr(), gb.data_ptr(), ALPHA, b2.data_ptr(), MU, LR,
                                gb.data_ptr(), n, L.stream_ptr(dev)), "abd_sgd_f32")
    assert nrel(gb, (1 - ALPHA) * g.astype(np.float64) + ALPHA * p0.astype(np.float64)) < ELEM_TOL
    assert torch.equal(gb, b2)                                              # first step: buf = d


# ------------------------------------------------------------------ 3. composite against composition
def no_update_step(m, x, y, masks, lp=None):
    T.train_step(m, x, y, None, None, None, mask1=masks[0], mask2=masks[1], do_update=False, logprobs_out=lp)
    return m._engine.grads.clone()


def composed_step(m, x, y, m1, m2, buf, K):
    """One batch of train_finetuning_reg from the entry points that predate the composite, one by one."""
    eng = m._engine
    offs = list(eng.offsets)
    B = x.shape[0]
    lp = torch.empty((3, B, K), device=x.device)
    p0, run0, nbt0 = eng.params.clone(), eng.running.clone(), eng.nbt.clone()
    g1 = no_update_step(m, x, y, (m1[0], m2[0]), lp[0])
    norms = torch.ops.abd.segment_norms(g1, offs)
    moved = torch.ops.abd.perturb(eng.params, g1, norms, offs, R)
    eng.params.copy_(moved)
    g2 = no_update_step(m, x, y, (m1[1], m2[1]), lp[1])
    eng.params.copy_(p0)
    eng.running.copy_(run0)          # forwards 1 and 2 ran on the reference's discarded copy
    eng.nbt.copy_(nbt0)
    gout = torch.empty_like(g1)
    torch.ops.abd.sgd(eng.params, g1, buf, gout, LR, MU, g2, ALPHA)
    lp[2] = m.hip_forward(x, train=True, mask1=m1[2], mask2=m2[2])
    lp3 = lp[2].cpu().numpy().astype(np.float64)
    yh = y.cpu().numpy()
    loss = float(-oc.log_softmax(lp3)[np.arange(B), yh].mean())
    return dict(params=eng.params.clone(), buf=buf.clone(), grads=gout, running=eng.running.clone(),
                nbt=eng.nbt.clone(), lp=lp, loss=loss, correct=int((lp3.argmax(1) == yh).sum()), p0=p0, moved=moved)


CASES = [(32, 13, 10, 48, "f32split"), (32, 13, 10, 48, "f32"), (32, 40, 35, 33, "f32split"), (32, 40, 35, 33, "f32"),
         (32, 13, 10, 1, "f32split"), (32, 13, 10, 1, "f32"), (32, 40, 35, 33, "bf16")]


@pytest.mark.parametrize("H,W,K,B,prec", CASES)
def test_composite_equals_composition(dev, H, W, K, B, prec):
    st, x, y = case_inputs(H, W, K, B, seed=20 + B + K)
    flat = st["fc1.weight"].shape[1]
    m1, m2 = dev_masks(draw_masks(rng(30 + B), B, flat), dev)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    ma, mb = build(st, K, dev, prec), build(st, K, dev, prec)
    ea, eb = ma.engine(xd), mb.engine(xd)
    buf0 = torch.tensor(magnitudes(rng(31), ea.n) * 1e-3, device=dev)       # a momentum buffer in mid-recurrence
    # the tolerance: the existing no-update train step's own run-to-run spread on identical inputs
    keep = (eb.running.clone(), eb.nbt.clone())
    ga = no_update_step(mb, xd, yd, (m1[0], m2[0]))
    gb = no_update_step(mb, xd, yd, (m1[0], m2[0]))
    eb.running.copy_(keep[0])
    eb.nbt.copy_(keep[1])
    spread = nrel(ga, gb)
    exp = composed_step(mb, xd, yd, m1, m2, buf0.clone(), K)
    bufa = buf0.clone()
    loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
    correct = torch.zeros(1, dtype=torch.int64, device=dev)
    lp = torch.ops.abd.smallcnn_finetune_reg_step(xd, yd, ea.params, ea.grads, bufa, ea.running, ea.nbt, loss_sum, correct,
                                                  K, R, ALPHA, LR, MU, 5, 0, None, None, m1, m2, prec)
    torch.cuda.synchronize()
    got = dict(params=ea.params, buf=bufa, grads=ea.grads, running=ea.running, lp=lp)
    errs = {k: nrel(got[k], exp[k]) for k in got}
    bit = {k: bool(torch.equal(got[k], exp[k])) for k in got}
    loss_err = abs(float(loss_sum) - exp["loss"]) / abs(exp["loss"])
    note(f"| {H}x{W} K={K} B={B} {prec} | {spread:.2e} | " + " | ".join(f"{errs[k]:.2e}{'=' if bit[k] else ''}" for k in got)
         + f" | {loss_err:.1e} |")
    if spread == 0.0:
        assert all(bit.values()), bit
    else:
        assert max(errs.values()) <= spread + ELEM_TOL, errs
    assert torch.equal(ea.nbt, exp["nbt"]) and ea.nbt.tolist() == [1, 1, 1]
    # the loss is a float64 mean of at most 48 terms on both sides, summed in different orders
    assert loss_err <= 1e-12 + (0 if spread == 0.0 else RTOL * (spread + ELEM_TOL))
    assert int(correct) == exp["correct"]
    # the displaced parameters are gone: params left its start by lr * buf and nothing else
    assert nrel(exp["moved"], exp["p0"]) > 1e-4
    step = (exp["p0"].double() - ea.params.double()).cpu().numpy()
    np.testing.assert_allclose(step, LR * bufa.double().cpu().numpy(), rtol=0,
                               atol=2.0 ** -23 * float(exp["p0"].abs().max()))


# ------------------------------------------------------------------ 4. against float64
def test_composite_matches_float64_restatement(dev):
    H, W, K, B = 32, 13, 10, 48
    st, x, y = case_inputs(H, W, K, B, seed=20 + B + K)
    flat = st["fc1.weight"].shape[1]
    m = build(st, K, dev)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    eng = m.engine(xd)
    buf = torch.zeros_like(eng.params)
    mo1 = torch.empty((3, B, flat), dtype=torch.uint8, device=dev)
    mo2 = torch.empty((3, B, 128), dtype=torch.uint8, device=dev)
    loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
    correct = torch.zeros(1, dtype=torch.int64, device=dev)
    lp = torch.ops.abd.smallcnn_finetune_reg_step(xd, yd, eng.params, eng.grads, buf, eng.running, eng.nbt, loss_sum,
                                                  correct, K, R, ALPHA, LR, MU, 99, 6, mo1, mo2)
    k1, k2 = mo1.cpu().numpy(), mo2.cpu().numpy()
    assert abs(k1.mean() - 0.6) < 0.02 and abs(k2.mean() - 0.5) < 0.05
    assert not np.array_equal(k1[0], k1[1]) and not np.array_equal(k1[1], k1[2])   # counters 6, 7, 8
    tr = RegTrainer(st, LR, MU, R, ALPHA)                                   # float32 dropout scale, as the device
    outs, loss, _ = tr.step(x, y, [(k1[k], k2[k]) for k in range(3)])
    got = lp.cpu().numpy()
    for k in range(3):
        err = np.abs(got[k] - outs[k]).max() / np.abs(outs[k]).max()
        note(f"| float64 restatement, forward {k + 1} log-probs | {err:.2e} |")
        np.testing.assert_allclose(got[k], outs[k], rtol=RTOL, atol=RTOL * np.abs(outs[k]).max())
    note(f"| float64 restatement, loss_sum | {abs(float(loss_sum) / loss - 1):.2e} |")
    assert abs(float(loss_sum) - loss) <= RTOL * abs(loss)


# ------------------------------------------------------------------ 5. the Python layer
def test_finetune_reg_epoch_equals_op_per_batch(dev):
    H, W, K, B = 32, 13, 10, 16
    st, x, y = case_inputs(H, W, K, 2 * B, seed=41)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    ma = build(st, K, dev)
    ea = ma.engine(xd)
    mb = build(st, K, dev, nonce=ma._dropout_nonce)
    eb = mb.engine(xd)
    opt = torch.optim.SGD(ma.parameters(), lr=LR, momentum=MU)
    seed = M.dropout_seed(dev, mb)
    bufb = torch.zeros_like(eb.params)
    perm = rng(42).permutation(2 * B)
    idx = torch.tensor(perm, device=dev)
    counter = 0
    for ep, order in enumerate((None, perm)):
        loss, acc, final = D.finetune_reg_epoch(ma, xd, yd, opt, R, ALPHA, batch_size=B, order=order)
        ls = torch.zeros(1, dtype=torch.float64, device=dev)
        co = torch.zeros(1, dtype=torch.int64, device=dev)
        for i in range(2):
            rows = slice(i * B, (i + 1) * B)
            xb, yb = (xd[rows], yd[rows]) if order is None else (xd[idx[rows]], yd[idx[rows]])
            torch.ops.abd.smallcnn_finetune_reg_step(xb.contiguous(), yb.contiguous(), eb.params, eb.grads, bufb,
                                                      eb.running, eb.nbt, ls, co, K, R, ALPHA, LR, MU, seed, counter,
                                                      None, None)
            counter += 3
        assert loss == pytest.approx(float(ls) / 2, rel=1e-6) and acc == pytest.approx(int(co) / (2 * B))
        assert nrel(ea.params, eb.params) < 1e-5 and nrel(ea.momentum_buf, bufb) < 1e-5
        assert nrel(ea.running, eb.running) < 1e-5 and torch.equal(ea.nbt, eb.nbt)
        assert all(f.data_ptr() == g.data_ptr() and f.shape == p.shape and p.grad is f
                   for f, g, p in zip(final, ea.views(ea.grads), ma._param_list()))
        assert nrel(ea.grads, eb.grads) < 1e-4
    assert ea.nbt.tolist() == [4, 4, 4] and ma._step == 12
    # the optimizer's momentum buffers are views of the flat buffer ...
    for p, off in zip(ma._param_list(), ea.offsets):
        mbuf = opt.state[p]["momentum_buffer"]
        assert mbuf.data_ptr() == ea.momentum_buf.data_ptr() + 4 * off and mbuf.shape == p.shape
    # ... so a plain torch step on the exposed gradients continues the recurrence
    p_before, b_before, g = ea.params.double().cpu(), ea.momentum_buf.double().cpu(), ea.grads.double().cpu()
    opt.step()
    nb = MU * b_before + g
    assert nrel(ea.momentum_buf, nb) < ELEM_TOL and nrel(ea.params, p_before - LR * nb) < ELEM_TOL


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_finetune_epoch_loss_and_accuracy_definitions(dev, kind):
    """train_finetuning: loss = sum of the batch-mean losses of each step's pre-update forward / batches (a
    short last batch weighs as much as a full one), acc = correct / samples; against a twin model stepped
    through training.train_step and read back batch by batch."""
    H, W, K, B, N = 32, 13, 10, 16, 40
    st, x, y = case_inputs(H, W, K, N, seed=43)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    ma = build(st, K, dev)
    ea = ma.engine(xd[:B])
    mb = build(st, K, dev, nonce=ma._dropout_nonce)
    eb = mb.engine(xd[:B])

    def make_opt(m):
        return torch.optim.SGD(m.parameters(), lr=LR, momentum=MU) if kind == "sgd" else \
            torch.optim.Adam(m.parameters(), lr=1e-3)

    loss, acc = D.finetune_epoch(ma, xd, yd, make_opt(ma), batch_size=B)
    optb = make_opt(mb)
    bind = T.SgdBinding(mb, optb) if kind == "sgd" else T.AdamBinding(mb, optb)
    means, hits = [], 0
    for s, e in D.batch_bounds(N, B):
        lp = torch.empty((e - s, K), device=dev)
        if kind == "sgd":
            T.train_step(mb, xd[s:e], yd[s:e], None, None, None, do_update=False, logprobs_out=lp)
            torch.ops.abd.sgd(eb.params, eb.grads, bind.buf, None, LR, MU)
        else:
            T.train_step(mb, xd[s:e], yd[s:e], None, bind, None, logprobs_out=lp)
        l64 = lp.cpu().numpy().astype(np.float64)
        yh = y[s:e]
        means.append(-oc.log_softmax(l64)[np.arange(e - s), yh].mean())
        hits += int((l64.argmax(1) == yh).sum())
    assert len(means) == 3
    assert loss == pytest.approx(sum(means) / 3, rel=1e-5) and acc == pytest.approx(hits / N)
    assert abs(sum(means) / 3 - (16 * means[0] + 16 * means[1] + 8 * means[2]) / 40) > 1e-6   # not the mean over rows
    assert nrel(ea.params, eb.params) < 1e-5 and nrel(ea.params, torch.cat(
        [torch.tensor(st[k]).reshape(-1) for k in M.PARAM_ORDER])) > 1e-6
    assert all(p.grad is not None and p.grad.data_ptr() == g.data_ptr()
               for p, g in zip(ma._param_list(), ea.views(ea.grads)))


def test_opcheck_new_ops(dev):
    H, W, K, B = 32, 13, 10, 8
    st, x, y = case_inputs(H, W, K, B, seed=44)
    m = build(st, K, dev)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    eng = m.engine(xd)
    n = eng.params.numel()
    buf, gout, g2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.randn(n, device=dev)
    torch.library.opcheck(torch.ops.abd.sgd.default, (eng.params, eng.grads, buf, gout, LR, MU, g2, ALPHA))
    torch.library.opcheck(torch.ops.abd.sgd.default, (eng.params, eng.grads, None, None, LR))
    offs = list(eng.offsets)
    norms = torch.ops.abd.segment_norms(g2, offs)
    torch.library.opcheck(torch.ops.abd.segment_norms.default, (g2, offs))
    torch.library.opcheck(torch.ops.abd.perturb.default, (eng.params, g2, norms, offs, R))
    flat = st["fc1.weight"].shape[1]
    ls = torch.zeros(1, dtype=torch.float64, device=dev)
    co = torch.zeros(1, dtype=torch.int64, device=dev)
    mo1 = torch.empty((3, B, flat), dtype=torch.uint8, device=dev)
    mo2 = torch.empty((3, B, 128), dtype=torch.uint8, device=dev)
    args = (xd, yd, eng.params, eng.grads, buf, eng.running, eng.nbt, ls, co, K, R, ALPHA, LR, MU, 3, 0)
    torch.library.opcheck(torch.ops.abd.smallcnn_finetune_reg_step.default, args + (None, None))
    torch.library.opcheck(torch.ops.abd.smallcnn_finetune_reg_step.default, args + (mo1, mo2),
                          dict(mask1_in=mo1.clone(), mask2_in=mo2.clone()))


def test_cpu_tensors_raise(dev):
    H, W, K, B = 32, 13, 10, 4
    st, x, y = case_inputs(H, W, K, B, seed=45)
    m = build(st, K, dev)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    opt = torch.optim.SGD(m.parameters(), lr=LR, momentum=MU)
    for bad in ((xd.cpu(), yd), (xd, yd.cpu())):
        with pytest.raises(L.AbdError):
            D.finetune_reg_epoch(m, bad[0], bad[1], opt, R, ALPHA)
        with pytest.raises(L.AbdError):
            D.finetune_epoch(m, bad[0], bad[1], opt)
    eng = m.engine(xd)
    with pytest.raises(L.AbdError):
        torch.ops.abd.sgd(eng.params, eng.grads.cpu(), None, None, LR)
    with pytest.raises(L.AbdError):
        D.finetune_epoch(m, xd, yd, torch.optim.SGD(m.parameters(), lr=LR, momentum=MU, nesterov=True))
