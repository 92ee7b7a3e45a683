"""GPU: the TSBD defense on the device (csrc/tsbd.hip, torch.ops.abd.row_abs_sums / smallcnn_unlearn_step /
reinit_weights, abd_amd.defense.unlearn_epoch / neuron_weight_change / reinit_models / reinit_sweep).

1. the unlearning step against the same step composed from the entry points that existed before it
   (training.train_step(do_update=False), negation, torch.ops.abd.adam): bit equality over 3 steps
2. its log-probs and loss against the float64 restatement (tsbd_cases.Unlearner, pinned to the reference's
   own function by tests/golden/tsbd_golden.npz) at the suite's RTOL = 1e-4
3. row abs sums: |a - b| bit-equal to torch on the CPU, row sums within 1 fp32 ulp of the float64 sum
4. re-initialisation: threshold, zeroed count and every output element equal to tsbd_cases.zero_reinit on
   the device's own fp32 values
5. the sweep against training.test on re-initialised models, and the epoch semantics
Set ABD_PARITY_OUT to a file name to have the observed figures of 2 appended to it.
"""
import os

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D, models as M, training as T
from golden_inputs import rng
from tsbd_cases import Unlearner, apply_reinit, case_inputs, draw_masks, zero_reinit

pytestmark = pytest.mark.gpu
RTOL = 1e-4
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
SHAPES = [(32, 13, 10, 1), (32, 13, 10, 16), (100, 40, 35, 8)]


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


def build(st, K, dev, prec="f32split", nonce=None):
    m = M.smallcnn(K, st["fc1.weight"].shape[1])
    m.load_state_dict({k: torch.tensor(v) for k, v in st.items()})
    m = m.to(dev).set_gemm_precision(prec).train()
    if nonce is not None:
        m._dropout_nonce = nonce
    return m


def ulps(got, ref32):
    """Distance in fp32 representation steps between two arrays of non-negative floats."""
    a = np.ascontiguousarray(got, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(ref32, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def record_of(eng, name="conv3.weight"):
    i = M.PARAM_ORDER.index(name)
    rows = {"conv1.weight": 64, "conv2.weight": 64, "conv3.weight": 32}[name]
    return [eng.offsets[i], rows, (eng.offsets[i + 1] - eng.offsets[i]) // rows]


# ------------------------------------------------------------------ 1. unlearning step against composition
@pytest.mark.parametrize("prec", ["f32split", "f32", "bf16"])
@pytest.mark.parametrize("H,W,K,B", SHAPES)
def test_unlearn_step_equals_composition(dev, H, W, K, B, prec):
    st, x, y = case_inputs(H, W, K, B, seed=50 + B + K)
    flat = st["fc1.weight"].shape[1]
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    ma, mb = build(st, K, dev, prec), build(st, K, dev, prec)
    ea, eb = ma.engine(xd), mb.engine(xd)
    ma_m, ma_v = torch.zeros_like(ea.params), torch.zeros_like(ea.params)
    mb_m, mb_v = torch.zeros_like(eb.params), torch.zeros_like(eb.params)
    meta, metb = (torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev) for _ in range(2))
    rec = record_of(ea)
    sums = torch.empty(rec[1], device=dev)
    r = rng(60 + B)
    p0 = ea.params.clone()
    for step in (1, 2, 3):
        k1, k2 = draw_masks(r, B, flat)
        m1, m2 = torch.tensor(k1, device=dev), torch.tensor(k2, device=dev)
        # the composition: gradient of +loss, negated, Adam
        T.train_step(mb, xd, yd, None, None, metb, mask1=m1, mask2=m2, do_update=False)
        g_pos = eb.grads.clone()
        eb.grads.neg_()
        torch.ops.abd.adam(eb.params, eb.grads, mb_m, mb_v, step, LR, B1, B2, EPS)
        lp = torch.ops.abd.smallcnn_unlearn_step(xd, yd, ea.params, ea.grads, ma_m, ma_v, ea.running, ea.nbt, meta, sums,
                                                 None, None, K, step, LR, B1, B2, EPS, 5, step, rec, m1, m2, prec)
        torch.cuda.synchronize()
        for what, got, exp in (("params", ea.params, eb.params), ("exp_avg", ma_m, mb_m), ("exp_avg_sq", ma_v, mb_v),
                               ("running", ea.running, eb.running), ("nbt", ea.nbt, eb.nbt), ("metrics", meta, metb),
                               ("grads", ea.grads, -g_pos)):
            assert torch.equal(got, exp), (what, step)
        assert ea.nbt.tolist() == [step] * 3 and lp.shape == (B, K)
        # the record layer's |grad| row sums: double accumulation, one rounding
        g = ea.grads[rec[0]:rec[0] + rec[1] * rec[2]].cpu().numpy().reshape(rec[1], rec[2])
        ref = np.abs(g.astype(np.float64)).sum(-1).astype(np.float32)
        assert ulps(sums.cpu().numpy(), ref).max() <= 1
    assert not torch.equal(ea.params, p0)
    loss_sum, total, _, _, _, nb = T.read_metrics(meta)
    assert total == 3 * B and nb == 3 and loss_sum > 0


# ------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("H,W,K,B", SHAPES)
def test_unlearn_step_matches_float64_restatement(dev, H, W, K, B):
    st, x, y = case_inputs(H, W, K, B, seed=70 + B + K)
    flat = st["fc1.weight"].shape[1]
    m = build(st, K, dev)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    eng = m.engine(xd)
    ea, ev = torch.zeros_like(eng.params), torch.zeros_like(eng.params)
    metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
    mo1 = torch.empty((B, flat), dtype=torch.uint8, device=dev)
    mo2 = torch.empty((B, 128), dtype=torch.uint8, device=dev)
    rec = record_of(eng)
    sums = torch.empty(rec[1], device=dev)
    lp = torch.ops.abd.smallcnn_unlearn_step(xd, yd, eng.params, eng.grads, ea, ev, eng.running, eng.nbt, metrics, sums,
                                             mo1, mo2, K, 1, LR, B1, B2, EPS, 99, 6, rec)
    k1, k2 = mo1.cpu().numpy(), mo2.cpu().numpy()
    if B >= 8:
        assert abs(k1.mean() - 0.6) < 0.1 and abs(k2.mean() - 0.5) < 0.1
    un = Unlearner(st, LR)                                       # float32 dropout scale, as the device
    out, loss, hits, norm = un.step(x, y, (k1, k2))
    got = lp.cpu().numpy()
    err = np.abs(got - out).max() / np.abs(out).max()
    loss_sum, total, correct, _, _, _ = T.read_metrics(metrics)
    nerr = np.abs(sums.cpu().numpy() - norm).max() / np.abs(norm).max()
    note(f"| {H}x{W} K={K} B={B} | {err:.2e} | {abs(loss_sum / loss - 1):.2e} | {nerr:.2e} |")
    np.testing.assert_allclose(got, out, rtol=RTOL, atol=RTOL * np.abs(out).max())
    assert abs(loss_sum - loss) <= RTOL * abs(loss) and total == B
    # the device negated the gradient: its sign agrees with the restatement's where the gradient is not tiny
    g = eng.grads.cpu().numpy()
    gr = np.concatenate([un.grads[k].reshape(-1) for k in M.PARAM_ORDER])
    big = np.abs(gr) > 1e-3 * np.abs(gr).max()
    assert big.any() and np.array_equal(np.sign(g[big]), np.sign(gr[big]))


# ------------------------------------------------------------------ 3. row abs sums
def magnitudes(r, n):
    return (r.standard_normal(n) * np.exp(r.uniform(-6, 3, n))).astype(np.float32)


def table_rows(table):
    """[(flat start, length)] of every row of a flat-triple table, in row order."""
    return [(o + i * n, n) for o, rows, n in zip(table[0::3], table[1::3], table[2::3]) for i in range(rows)]


def check_row_abs_sums(dev, a, b, table):
    ad = torch.tensor(a, device=dev)
    bd = torch.tensor(b, device=dev) if b is not None else None
    absdiff, sums = torch.ops.abd.row_abs_sums(ad, bd, table)
    again = torch.ops.abd.row_abs_sums(ad, bd, table)
    assert torch.equal(absdiff, again[0]) and torch.equal(sums, again[1])
    exp = (torch.tensor(a) - torch.tensor(b)).abs() if b is not None else torch.tensor(a).abs()   # torch on the CPU
    rows = table_rows(table)
    packed = torch.cat([exp[s:s + n] for s, n in rows])
    assert torch.equal(absdiff.cpu(), packed)
    ref = np.array([packed[at:at + n].numpy().astype(np.float64).sum()
                    for at, n in zip(np.cumsum([0] + [n for _, n in rows[:-1]]), [n for _, n in rows])])
    d = ulps(sums.cpu().numpy(), ref.astype(np.float32))
    print(f"row sums: {len(rows)} rows, max {d.max()} ulp")
    assert d.max() <= 1
    none, sums2 = torch.ops.abd.row_abs_sums(ad, bd, table, False)
    assert none.numel() == 0 and torch.equal(sums2, sums)


def test_row_abs_sums_model_tables(dev):
    m = M.smallcnn(10, 224)
    n = D.param_offsets(m)[-1]
    r = rng(80)
    a, b = magnitudes(r, n), magnitudes(r, n)
    b[::5] = a[::5]                                                   # exact zeros among the differences
    check_row_abs_sums(dev, a, b, D.row_table(m, "conv"))
    check_row_abs_sums(dev, a, b, D.row_table(m, "bn"))
    check_row_abs_sums(dev, a, None, D.row_table(m, "conv"))


def test_row_abs_sums_odd_table(dev):
    # first segment at element 3 (no 16-byte alignment), row lengths 7 and 300 (no power of two), 70 rows of
    # 256 (more than one block), a 1-row segment and rows of length 1
    table = [3, 5, 7, 41, 70, 256, 18000, 1, 300, 18301, 9, 1, 18311, 2, 65]
    r = rng(81)
    n = 18311 + 130 + 5
    check_row_abs_sums(dev, magnitudes(r, n), magnitudes(r, n), table)
    check_row_abs_sums(dev, magnitudes(r, n), None, table)
    view = torch.tensor(magnitudes(r, n + 1), device=dev)[1:]         # the buffer itself at a 4-byte phase
    assert view.data_ptr() % 16 == 4
    absdiff, sums = torch.ops.abd.row_abs_sums(view, None, table)
    h = view.cpu()
    rows = table_rows(table)
    assert torch.equal(absdiff.cpu(), torch.cat([h[s:s + n_].abs() for s, n_ in rows]))
    with pytest.raises(L.AbdError):
        torch.ops.abd.row_abs_sums(view, None, [0, 4, 0])
    with pytest.raises(L.AbdError):
        torch.ops.abd.row_abs_sums(view, None, [n, 2, 4])             # past the buffer


# ------------------------------------------------------------------ 4. re-initialisation
@pytest.fixture(scope="module")
def unlearned(dev):
    """A 32x13 model after three unlearning steps, with its original state and NWC (computed once)."""
    H, W, K, B = 32, 13, 10, 16
    st, x, y = case_inputs(H, W, K, 3 * B, seed=90)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    base = build(st, K, dev)
    base.engine(xd)
    m = build(st, K, dev)
    opt = torch.optim.Adam(m.parameters(), lr=LR)
    D.unlearn_epoch(m, xd, yd, opt, batch_size=B, whole_epoch=True)
    out = dict(st=st, base=base, model=m, xd=xd, yd=yd, K=K)
    for lt in ("conv", "bn"):
        names, scores, absdiff = D.neuron_weight_change(m, st, lt)
        out[lt] = dict(names=names, scores=scores, absdiff=absdiff, ranked=D.rank_neurons((names, scores)))
    return out


def expected_reinit(base, lt, absdiff, ranked, top_num, wratio):
    """(thr, out, zeroed) of tsbd_cases.zero_reinit on the device's own fp32 absdiff values."""
    table = D.row_table(base, lt)
    names = D.neuron_names(base, lt)
    host = absdiff.cpu().numpy()
    rows = table_rows(table)
    packed_at = np.cumsum([0] + [n for _, n in rows[:-1]])
    by_name = {nm: host[at:at + n] for nm, at, (_, n) in zip(names, packed_at, rows)}
    start = {nm: s for nm, (s, _) in zip(names, rows)}
    thr, masks = zero_reinit(by_name, ranked, top_num, wratio)
    assert thr.dtype == np.float32
    out = D._flat_params(base, "cpu").numpy().copy()
    zeroed = 0
    for nm, mask in masks.items():
        out[start[nm] + np.nonzero(mask)[0]] = 0.0
        zeroed += int(mask.sum())
    return thr, out, zeroed


def check_reinit(base, lt, absdiff, ranked, top_num, wratio):
    """One variant (the first top_num neurons of the ranking) against the restatement; returns the zeroed count."""
    got, thr, zeroed = D.reinit_models(base, ranked[:top_num], absdiff, [1.0], wratio)
    ethr, eout, ezero = expected_reinit(base, lt, absdiff, ranked, top_num, wratio)
    assert float(thr[0]) == float(ethr) and int(zeroed[0]) == ezero
    assert np.array_equal(got[0].cpu().numpy(), eout)
    return ezero


def test_reinit_on_unlearned_model(dev, unlearned):
    u, c = unlearned, unlearned["conv"]
    base = u["base"]
    assert float(c["absdiff"].max()) > 1e-4                          # the model did move
    many, thr, zeroed = D.reinit_models(base, c["ranked"], c["absdiff"], D.REINIT_RATIO, 0.7)
    assert many.shape == (11, base._engine.n) and thr.shape == (11,) and zeroed.dtype == torch.int64
    for v, ratio in enumerate(D.REINIT_RATIO):
        ethr, eout, ezero = expected_reinit(base, "conv", c["absdiff"], c["ranked"], int(160 * ratio), 0.7)
        assert float(thr[v]) == float(ethr) and int(zeroed[v]) == ezero, ratio
        assert np.array_equal(many[v].cpu().numpy(), eout), ratio
        # 11 variants in one call against one call each
        one = D.reinit_models(base, c["ranked"], c["absdiff"], [ratio], 0.7)
        assert torch.equal(one[0][0], many[v]) and torch.equal(one[1][0], thr[v]) and torch.equal(one[2][0], zeroed[v])
    assert torch.equal(D._flat_params(base, dev), base._engine.params)   # the model itself is untouched
    assert zeroed.tolist() == sorted(zeroed.tolist()) and int(zeroed[0]) >= 2       # more neurons, more weights


def test_reinit_ties_at_the_threshold(dev, unlearned):
    u, c = unlearned, unlearned["conv"]
    q = torch.round(c["absdiff"] * 1024.0) / 1024.0                  # multiples of 2^-10
    assert q.unique().numel() < 64
    for top_num in (16, 80):
        ezero = check_reinit(u["base"], "conv", q, c["ranked"], top_num, 0.7)
        m = sum(256 if layer != "conv1.weight" else 4 for layer, _, _ in c["ranked"][:top_num])
        assert ezero > int(m * 0.7)                                   # ``>=`` zeroes more than k weights


def test_reinit_extreme_ranks_and_single_rows(dev, unlearned):
    u, c = unlearned, unlearned["conv"]
    base, ranked = u["base"], c["ranked"]
    m16 = sum(256 if layer != "conv1.weight" else 4 for layer, _, _ in ranked[:16])
    assert check_reinit(base, "conv", c["absdiff"], ranked, 16, 1.5 / m16) >= 1          # k == 1
    assert check_reinit(base, "conv", c["absdiff"], ranked, 16, 1.0) == m16              # k == m
    row4 = [r for r in ranked if r[0] == "conv1.weight"][:1]
    row256 = [r for r in ranked if r[0] == "conv3.weight"][:1]
    assert check_reinit(base, "conv", c["absdiff"], row4, 1, 0.7) >= 2                   # m = 4, k = 2
    assert check_reinit(base, "conv", c["absdiff"], row256, 1, 0.7) >= 179               # m = 256
    assert check_reinit(base, "conv", c["absdiff"], ranked, 160, 0.7) >= int(24832 * 0.7)   # every conv row
    assert check_reinit(base, "conv", c["absdiff"], ranked, 160, 1.0) == 24832


def test_reinit_bn_table(dev, unlearned):
    u, b = unlearned, unlearned["bn"]
    assert b["absdiff"].numel() == 160 and len(b["ranked"]) == 160 and b["ranked"][0][0].startswith("bn")
    for top_num, wratio in ((16, 0.7), (160, 0.7), (160, 1.0), (3, 0.4)):
        check_reinit(u["base"], "bn", b["absdiff"], b["ranked"], top_num, wratio)


def test_reinit_invalid_arguments(dev, unlearned):
    u, c = unlearned, unlearned["conv"]
    base = u["base"]
    params = base._engine.params
    table = D.row_table(base, "conv")
    sel = torch.zeros((1, 160), dtype=torch.uint8)
    with pytest.raises(L.AbdError, match="selects no row"):
        torch.ops.abd.reinit_weights(params, c["absdiff"], table, sel, [1])
    sel[0, 0] = 1                                                    # conv1.weight.0: m = 4
    for k in (0, -1, 5):
        with pytest.raises(L.AbdError, match="outside"):
            torch.ops.abd.reinit_weights(params, c["absdiff"], table, sel, [k])
    out, thr, zeroed = torch.ops.abd.reinit_weights(params, c["absdiff"], table, sel, [4])
    assert int(zeroed[0]) == 4 and torch.count_nonzero(out[0][:4]) == 0 and torch.equal(out[0][4:], params[4:])
    with pytest.raises(ValueError):
        D.reinit_models(base, c["ranked"], c["absdiff"], [0.001], 0.7)               # top_num == 0, as min([])
    with pytest.raises(L.AbdError):
        torch.ops.abd.reinit_weights(params, c["absdiff"], table, sel.repeat(17, 1), [1] * 17)


# ------------------------------------------------------------------ 5. sweep and epoch semantics
def test_reinit_sweep_equals_test_on_reinitialised_models(dev, unlearned):
    u, c = unlearned, unlearned["conv"]
    st, base, K = u["st"], u["base"], u["K"]
    _, cx, cy = case_inputs(32, 13, K, 64, seed=91)
    _, bx, by = case_inputs(32, 13, K, 64, seed=92)
    bind = (rng(93).random(64) < 0.7).astype(np.int64)
    bind[0] = 1
    by[bind == 1] = 2
    dv = [torch.tensor(a, device=dev) for a in (cx, cy, bx, by, bind)]
    ratios = [0.01, 0.5]
    got = D.reinit_sweep(base, *dv, c["ranked"], c["absdiff"], ratios=ratios, wratio=0.7, batch_size=32)
    host = c["absdiff"].cpu().numpy()
    names = c["names"]
    rows = table_rows(D.row_table(base, "conv"))
    packed_at = np.cumsum([0] + [n for _, n in rows[:-1]])
    by_name = {nm: host[at:at + n] for nm, at, (_, n) in zip(names, packed_at, rows)}
    clean = [(torch.tensor(cx[s:s + 32]), torch.tensor(cy[s:s + 32])) for s in (0, 32)]
    bd = [dict(mfcc=torch.tensor(bx[s:s + 32]), label=torch.tensor(by[s:s + 32]),
               poison_indicator=torch.tensor(bind[s:s + 32])) for s in (0, 32)]
    for v, ratio in enumerate(ratios):
        _, masks = zero_reinit(by_name, c["ranked"], int(160 * ratio), 0.7)
        twin = build(apply_reinit(st, masks), K, dev)
        exp = T.test(twin, dev, clean, bd, torch.nn.CrossEntropyLoss())
        print(f"ratio {ratio}: sweep {got[v]}, training.test {exp}")
        assert got[v][0] == exp[0] and got[v][1] == exp[1]
        assert got[v][2] == pytest.approx(exp[2], rel=1e-6) and got[v][3] == pytest.approx(exp[3], rel=1e-6)
    assert got[0] != got[1]
    # one variant as a model of its own, ready for finetune_epoch
    params, _, _ = D.reinit_models(base, c["ranked"], c["absdiff"], [0.5], 0.7)
    m = D.model_with_params(base, params[0])
    assert m._engine is None and torch.equal(D._flat_params(m, dev), params[0])
    loss, acc = D.finetune_epoch(m, dv[0], dv[1], torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9), batch_size=32)
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0 and not torch.equal(D._flat_params(m, dev), params[0])


def test_unlearn_epoch_semantics(dev):
    H, W, K, B, N = 32, 13, 10, 16, 40
    st, x, y = case_inputs(H, W, K, N, seed=94)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    ma = build(st, K, dev)
    ea = ma.engine(xd[:B])
    mb = build(st, K, dev, nonce=ma._dropout_nonce)
    eb = mb.engine(xd[:B])
    opt = torch.optim.Adam(ma.parameters(), lr=LR)
    loss, acc, avg, var = D.unlearn_epoch(ma, xd, yd, opt, batch_size=B)
    # the twin: the first batch only, through the op
    mm, mv = torch.zeros_like(eb.params), torch.zeros_like(eb.params)
    metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
    rec = record_of(eb)
    sums = torch.empty(32, device=dev)
    torch.ops.abd.smallcnn_unlearn_step(xd[:B], yd[:B], eb.params, eb.grads, mm, mv, eb.running, eb.nbt, metrics, sums,
                                        None, None, K, 1, LR, B1, B2, EPS, M.dropout_seed(dev, mb), 0, rec)
    first_loss, total, hits, _, _, _ = T.read_metrics(metrics)
    assert total == B
    assert loss == pytest.approx(first_loss / 3) and acc == pytest.approx(hits / N)      # 3 batches, 40 rows
    assert torch.equal(ea.params, eb.params) and torch.equal(avg, sums)
    assert var.shape == (32,) and bool(torch.isnan(var).all())
    assert ea.nbt.tolist() == [1, 1, 1] and ma._step == 1
    assert all(int(opt.state[p]["step"]) == 1 for p in ma.parameters())
    assert all(p.grad is not None and p.grad.data_ptr() == g.data_ptr() for p, g in zip(ma._param_list(), ea.views(ea.grads)))
    assert torch.equal(opt.state[ma.conv3.weight]["exp_avg"].reshape(-1), mm[rec[0]:rec[0] + 32 * 256])
    # whole_epoch=True visits every batch (16, 16 and 8 rows), same divisors
    loss2, acc2, avg2, var2 = D.unlearn_epoch(ma, xd, yd, opt, batch_size=B, whole_epoch=True)
    assert ea.nbt.tolist() == [4, 4, 4] and ma._step == 4
    assert all(int(opt.state[p]["step"]) == 4 for p in ma.parameters())
    assert bool(torch.isfinite(var2).all()) and avg2.shape == (32,) and loss2 > loss and 0.0 <= acc2 <= 1.0
    # a permutation and no record layer (correlation_analysis.py's variant)
    perm = rng(95).permutation(N)
    loss3, acc3, none_a, none_v = D.unlearn_epoch(ma, xd, yd, opt, record_layer=None, batch_size=B, order=perm)
    assert none_a is None and none_v is None and ea.nbt.tolist() == [5, 5, 5] and np.isfinite(loss3)
    with pytest.raises(L.AbdError):
        D.unlearn_epoch(ma, xd, yd, torch.optim.SGD(ma.parameters(), lr=0.01))
    with pytest.raises(L.AbdError):
        D.unlearn_epoch(ma, xd.cpu(), yd, opt)
