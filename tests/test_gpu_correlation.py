"""GPU: the unlearning correlation analysis on the device (csrc/nwc_corr.hip, torch.ops.abd.smallcnn_unlearn_run /
nwc_pair, abd_amd.defense.unlearn_run / correlation_analysis).

1. the unlearning run against n separate torch.ops.abd.smallcnn_unlearn_step calls: bit equality of the
   parameters, Adam moments, gradients, BN buffers and every per-step metrics row, in the three GEMM precisions
2. nwc_pair: |a - orig| and the fp32 row sums bit-equal to torch.ops.abd.row_abs_sums, the double sums within
   row_len * 2^-53 * sum of numpy's sequential float64 sum (all terms are non-negative), the statistics against
   the same formulas in numpy float64 on the device's own double sums
3. correlation_analysis end to end on the fixture of tests/golden/correlation_golden.npz
4. torch.library.opcheck on both ops
Set ABD_PARITY_OUT to a file name to have the observed figures of 3 appended to it.

Measured on MI355X (f32split, the fixture: 3 Adam(1e-3) steps, 16 rows; profiles/correlation/parity.md):
largest relative difference of a neuron's score to the float64 restatement 1.62e-5 (5.4e-7 of the largest
score), |delta r| 4.29e-9; the bounds asserted are 10x those.  fp32 gradient rounding passes through Adam's normalised update undamped (a first step moves
every weight by lr * sign(g), so a gradient whose sign flips under rounding moves its weight by 2 lr), hence
no bound could be fixed before measuring.
"""
import os

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D, models as M, training as T
from correlation_cases import FIXTURE, analyse, fixture_inputs
from golden_inputs import rng, unpack_mask
from tsbd_cases import case_inputs, draw_masks

pytestmark = pytest.mark.gpu
RTOL = 1e-4
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
U = 2.0 ** -53
SCORE_BOUND = 1.62e-4     # 10 x the measured 1.62e-5 (cap: 1e-2)
R_BOUND = 4.3e-8          # 10 x the measured 4.29e-9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "correlation_golden.npz")


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


class Side:
    """One model's engine buffers plus Adam moments for the raw ops."""

    def __init__(self, st, K, dev, prec, xd):
        self.m = build(st, K, dev, prec)
        self.e = self.m.engine(xd)
        self.mm, self.mv = torch.zeros_like(self.e.params), torch.zeros_like(self.e.params)

    def state(self):
        e = self.e
        return (("params", e.params), ("grads", e.grads), ("exp_avg", self.mm), ("exp_avg_sq", self.mv),
                ("running", e.running), ("nbt", e.nbt))


# ------------------------------------------------------------------ 1. the run against separate steps
@pytest.mark.parametrize("prec", ["f32split", "f32", "bf16"])
@pytest.mark.parametrize("H,W,K,B", [(32, 13, 10, 1), (32, 13, 10, 5), (100, 40, 35, 8)])
def test_unlearn_run_equals_separate_steps(dev, H, W, K, B, prec):
    n = 3
    st, x, y = case_inputs(H, W, K, B, seed=150 + B + K)
    flat = st["fc1.weight"].shape[1]
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    a, b = Side(st, K, dev, prec, xd), Side(st, K, dev, prec, xd)
    r = rng(160 + B)
    drawn = [draw_masks(r, B, flat) for _ in range(n)]
    m1 = torch.tensor(np.stack([d[0] for d in drawn]), device=dev)
    m2 = torch.tensor(np.stack([d[1] for d in drawn]), device=dev)
    meta, metb = (torch.zeros((n, L.METRICS_WORDS), dtype=torch.int64, device=dev) for _ in range(2))
    p0 = a.e.params.clone()
    lpa = torch.ops.abd.smallcnn_unlearn_run(xd, yd, a.e.params, a.e.grads, a.mm, a.mv, a.e.running, a.e.nbt, meta, None,
                                             None, K, n, 1, LR, B1, B2, EPS, 5, 1, m1, m2, prec)
    for i in range(n):
        lpb = torch.ops.abd.smallcnn_unlearn_step(xd, yd, b.e.params, b.e.grads, b.mm, b.mv, b.e.running, b.e.nbt, metb[i],
                                                  None, None, None, K, 1 + i, LR, B1, B2, EPS, 5, 1 + i, None, m1[i], m2[i],
                                                  prec)
    torch.cuda.synchronize()
    for (what, got), (_, exp) in zip(a.state(), b.state()):
        assert torch.equal(got, exp), what
    assert torch.equal(meta, metb) and torch.equal(lpa, lpb)
    assert a.e.nbt.tolist() == [n] * 3 and not torch.equal(a.e.params, p0)
    for i in range(n):                                            # row i holds step i alone
        loss_sum, total, _, _, _, nb = T.read_metrics(meta[i])
        assert total == B and nb == 1 and loss_sum > 0
    assert len({int(v) for v in meta[:, 0]}) == n                 # three different losses


def test_unlearn_run_generated_masks_advance_the_counter(dev):
    H, W, K, B, n = 32, 13, 10, 5, 3
    st, x, y = case_inputs(H, W, K, B, seed=170)
    flat = st["fc1.weight"].shape[1]
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    a, b = Side(st, K, dev, "f32split", xd), Side(st, K, dev, "f32split", xd)
    meta, metb = (torch.zeros((n, L.METRICS_WORDS), dtype=torch.int64, device=dev) for _ in range(2))
    oa1, ob1 = (torch.zeros((n, B, flat), dtype=torch.uint8, device=dev) for _ in range(2))
    oa2, ob2 = (torch.zeros((n, B, 128), dtype=torch.uint8, device=dev) for _ in range(2))
    seed, counter, first = 99, 7, 4
    torch.ops.abd.smallcnn_unlearn_run(xd, yd, a.e.params, a.e.grads, a.mm, a.mv, a.e.running, a.e.nbt, meta, oa1, oa2, K, n,
                                       first, LR, B1, B2, EPS, seed, counter)
    for i in range(n):
        torch.ops.abd.smallcnn_unlearn_step(xd, yd, b.e.params, b.e.grads, b.mm, b.mv, b.e.running, b.e.nbt, metb[i], None,
                                            ob1[i], ob2[i], K, first + i, LR, B1, B2, EPS, seed, counter + i)
    torch.cuda.synchronize()
    assert torch.equal(oa1, ob1) and torch.equal(oa2, ob2) and torch.equal(meta, metb)
    for (what, got), (_, exp) in zip(a.state(), b.state()):
        assert torch.equal(got, exp), what
    # the counter did advance: every step drew other masks
    assert not torch.equal(oa1[0], oa1[1]) and not torch.equal(oa1[1], oa1[2]) and not torch.equal(oa2[0], oa2[2])
    with pytest.raises(L.AbdError):
        torch.ops.abd.smallcnn_unlearn_run(xd, yd, a.e.params, a.e.grads, a.mm, a.mv, a.e.running, a.e.nbt, meta, None, None,
                                           K, 0, 1, LR, B1, B2, EPS, seed, counter)
    with pytest.raises(L.AbdError):                               # one mask set for three steps
        torch.ops.abd.smallcnn_unlearn_run(xd, yd, a.e.params, a.e.grads, a.mm, a.mv, a.e.running, a.e.nbt, meta, None, None,
                                           K, n, 1, LR, B1, B2, EPS, seed, counter, oa1[0], oa2[0])


# ------------------------------------------------------------------ 2. nwc_pair
def table_rows(table):
    """[(flat start, length)] of every row of a flat-triple table, in row order."""
    return [(o + i * n, n) for o, rows, n in zip(table[0::3], table[1::3], table[2::3]) for i in range(rows)]


def pair_inputs(r, n, table):
    """orig and two changed copies whose per-row changes share a per-row scale: correlated, not collinear."""
    orig = r.standard_normal(n).astype(np.float32)
    a, b = orig.copy(), orig.copy()
    for s, ln in table_rows(table):
        scale, other = np.exp(r.uniform(-4, 0)), np.exp(r.uniform(-4, 0))
        a[s:s + ln] += (scale * r.standard_normal(ln)).astype(np.float32)
        b[s:s + ln] += ((0.6 * scale + 0.4 * other) * r.standard_normal(ln)).astype(np.float32)
    return orig, a, b


def host_stats(x, y):
    """abd_nwc_pair_f32's formulas in numpy float64."""
    n = len(x)
    mx, my = x.mean(), y.mean()
    dx, dy = x - mx, y - my
    sxx, syy, sxy = (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.float64(sxy) / np.sqrt(np.float64(sxx * syy)) if n >= 2 and sxx * syy != 0 else np.nan
        slope = np.float64(sxy) / np.float64(sxx) if sxx != 0 else np.nan
    return np.array([n, mx, my, sxx, syy, sxy, r, slope, my - slope * mx])


def check_pair(dev, orig, a, b, table, two_points=False):
    od, ad, bd = (torch.tensor(v, device=dev) for v in (orig, a, b))
    ab_a, ab_b, s32_a, s32_b, s64, stats = torch.ops.abd.nwc_pair(od, ad, bd, table)
    again = torch.ops.abd.nwc_pair(od, ad, bd, table)
    assert all(torch.equal(p, q) or (p.dtype == torch.float64 and torch.equal(p.view(torch.int64), q.view(torch.int64)))
               for p, q in zip((ab_a, ab_b, s32_a, s32_b, s64, stats), again))
    rows = table_rows(table)
    assert s64.shape == (2, len(rows)) and stats.shape == (9,) and s64.dtype == stats.dtype == torch.float64
    for params, absdiff, s32, col in ((ad, ab_a, s32_a, 0), (bd, ab_b, s32_b, 1)):
        ref_abs, ref_sums = torch.ops.abd.row_abs_sums(params, od, table)
        assert torch.equal(absdiff, ref_abs) and torch.equal(s32, ref_sums)
        host, got = absdiff.cpu().numpy().astype(np.float64), s64[col].cpu().numpy()
        at = 0
        for i, (_, ln) in enumerate(rows):
            seq = np.cumsum(host[at:at + ln])[-1]                 # numpy's sequential float64 sum
            assert abs(got[i] - seq) <= ln * U * seq, (i, ln)
            at += ln
        assert np.array_equal(got.astype(np.float32), s32.cpu().numpy())     # the same sum, rounded once
    none = torch.ops.abd.nwc_pair(od, ad, bd, table, False)
    assert none[0].numel() == none[1].numel() == 0 and torch.equal(none[2], s32_a) and torch.equal(none[3], s32_b)
    x, y = s64[0].cpu().numpy(), s64[1].cpu().numpy()
    got, exp = stats.cpu().numpy(), host_stats(x, y)
    n = len(rows)
    assert got[0] == n
    np.testing.assert_allclose(got[1:3], exp[1:3], rtol=2 * n * U)            # means of non-negative values
    np.testing.assert_allclose(got[3:5], exp[3:5], rtol=8 * n * U)            # sums of squares
    if n == 1:
        assert np.isnan(got[6:]).all() and got[3] == got[4] == got[5] == 0.0
        return got
    r = exp[6]
    if two_points:                                                # two points always lie on a line: |r| = 1
        assert abs(abs(got[6]) - 1.0) <= 8 * n * U and np.sign(got[6]) == np.sign(r)
    else:
        assert 0.1 < abs(r) < 0.999, r                            # keeps the bounds below meaningful
        assert abs(got[6] - r) <= 8 * n * U / (1 - r * r) * abs(r)
    # |sum dx dy| >= |r| sum |dx dy| fails in general, but sum |dx dy| <= sqrt(sxx syy) = |sxy| / |r|: the
    # centred cross sum carries a relative error of up to (n + 2) u / |r|, sxx one of (n + 2) u
    slope_tol = 8 * n * U * (1 + 1 / abs(r))
    assert abs(got[5] - exp[5]) <= 8 * n * U / abs(r) * abs(exp[5])
    assert abs(got[7] - exp[7]) <= slope_tol * abs(exp[7])
    assert abs(got[8] - exp[8]) <= slope_tol * abs(exp[7] * exp[1]) + 4 * U * (abs(exp[2]) + abs(exp[7] * exp[1]))
    return got


def test_nwc_pair_model_tables(dev):
    m = M.smallcnn(10, 224)
    n = D.param_offsets(m)[-1]
    for lt, seed in (("conv", 180), ("bn", 181)):                # lane groups 4 and 64; rows of length 1
        table = D.row_table(m, lt)
        orig, a, b = pair_inputs(rng(seed), n, table)
        a[::7] = orig[::7]                                        # exact zeros among the differences
        got = check_pair(dev, orig, a, b, table)
        assert got[0] == 160


def test_nwc_pair_odd_and_extreme_tables(dev):
    r = rng(182)
    odd = [3, 3, 5, 19, 1, 300]                                   # 3 rows of 5 at an unaligned offset, 1 row of 300
    check_pair(dev, *pair_inputs(r, 330, odd), odd)
    view = torch.tensor(r.standard_normal(331).astype(np.float32), device=dev)[1:]    # a 4-byte phase
    assert view.data_ptr() % 16 == 4
    out = torch.ops.abd.nwc_pair(view, view * 2, view * 3, odd)
    ref = torch.ops.abd.row_abs_sums(view * 2, view, odd)
    assert torch.equal(out[0], ref[0]) and torch.equal(out[2], ref[1])
    two = [1, 2, 9]                                               # 2 rows: the minimum that has a correlation
    check_pair(dev, *pair_inputs(r, 32, two), two, two_points=True)
    one = [0, 1, 40]                                              # 1 row: no correlation, no line
    got = check_pair(dev, *pair_inputs(r, 40, one), one)
    assert got[0] == 1 and np.isnan(got[6]) and np.isnan(got[7]) and np.isnan(got[8]) and got[1] > 0
    most = [5, L.MAX_REINIT_ROWS, 1]                              # 1024 rows of length 1: the maximum
    got = check_pair(dev, *pair_inputs(r, 5 + L.MAX_REINIT_ROWS, most), most)
    assert got[0] == L.MAX_REINIT_ROWS
    over = torch.zeros(L.MAX_REINIT_ROWS + 1, device=dev)
    with pytest.raises(L.AbdError, match="rows"):
        torch.ops.abd.nwc_pair(over, over, over, [0, L.MAX_REINIT_ROWS + 1, 1])
    with pytest.raises(L.AbdError):
        torch.ops.abd.nwc_pair(over, over, over, [2, L.MAX_REINIT_ROWS, 1])          # past the buffer
    with pytest.raises(L.AbdError):
        torch.ops.abd.nwc_pair(over, over[:-1], over, [0, 4, 1])


def segments32():
    """32 segments, the most a table holds: 1..3 rows of 1, 3, 65 or 4 values, a one-element gap after every other."""
    table, off = [], 1
    for s in range(32):
        rows, ln = 1 + s % 3, (1, 3, 65, 4)[s % 4]
        table += [off, rows, ln]
        off += rows * ln + s % 2
    return table


# the smallest tables that reach each branch of the row body nwc_pair and row_abs_sums share
ROW_BODY_TABLES = {"row_len 1: lane group 1": [2, 7, 1],
                   "row_len 3: lane group 4, one dead lane": [1, 5, 3],
                   "row_len 65: lane group 64, two strides": [3, 6, 65],
                   "70 rows of 4: the second block has dead rows": [0, 70, 4],
                   "32 segments": segments32()}


@pytest.mark.parametrize("name", list(ROW_BODY_TABLES))
def test_nwc_pair_and_row_abs_sums_share_one_row_body(dev, name):
    table = ROW_BODY_TABLES[name]
    n = max(s + ln for s, ln in table_rows(table)) + 3
    orig, a, b = (torch.tensor(v, device=dev) for v in pair_inputs(rng(183), n, table))
    ab_a, ab_b, s32_a, s32_b, s64, _ = torch.ops.abd.nwc_pair(orig, a, b, table)
    for params, absdiff, s32, col in ((a, ab_a, s32_a, 0), (b, ab_b, s32_b, 1)):
        ref_abs, ref_sums = torch.ops.abd.row_abs_sums(params, orig, table)
        assert torch.equal(absdiff, ref_abs) and torch.equal(s32, ref_sums)
        assert torch.equal(s64[col].to(torch.float32), s32)                          # the same sum, rounded once
        assert torch.equal(absdiff, torch.cat([(params[s:s + ln] - orig[s:s + ln]).abs() for s, ln in table_rows(table)]))
    none = torch.ops.abd.nwc_pair(orig, a, b, table, False)
    assert none[0].numel() == none[1].numel() == 0 and torch.equal(none[2], s32_a) and torch.equal(none[3], s32_b)


def test_step_mask_messages(dev):
    """The mask checks of the four step ops on device tensors: today's texts for a wrong dtype and a wrong or
    missing leading dimension."""
    from abd_amd import ops
    m1 = torch.zeros((2, 6), dtype=torch.uint8, device=dev)
    m2 = torch.zeros((2, 128), dtype=torch.uint8, device=dev)
    ops._check_masks((m1, m2, m1, m2), 2, 6)
    with pytest.raises(L.AbdError, match=r"mask1_in must be uint8 \(2, 6\), got \(2, 6\)"):
        ops._check_masks((m1.float(), m2, None, None), 2, 6)
    with pytest.raises(L.AbdError, match=r"mask1_in must be uint8 \(3, 2, 6\), got \(2, 6\)"):
        ops._check_masks((m1, m2, None, None), 2, 6, lead=(3,))
    with pytest.raises(L.AbdError, match=r"mask2_out must be uint8 \(3, 2, 128\), got \(4, 2, 128\)"):
        ops._check_masks((None, None, m1.expand(3, 2, 6).contiguous(), m2.expand(4, 2, 128).contiguous()), 2, 6, (3,))


def test_nwc_pair_constant_column_gives_nan(dev):
    m = M.smallcnn(10, 224)
    n = D.param_offsets(m)[-1]
    table = D.row_table(m, "bn")
    orig = torch.zeros(n, device=dev)
    const = torch.full((n,), 0.5, device=dev)                     # every row sum exactly 0.5
    moving = torch.tensor(np.abs(rng(183).standard_normal(n)).astype(np.float32) + 0.1, device=dev)
    stats = torch.ops.abd.nwc_pair(orig, moving, const, table)[5].cpu().numpy()          # constant y
    assert np.isnan(stats[6]) and stats[4] == 0.0 and stats[3] > 0 and stats[7] == 0.0 and stats[8] == 0.5
    stats = torch.ops.abd.nwc_pair(orig, const, moving, table)[5].cpu().numpy()          # constant x
    assert np.isnan(stats[6]) and np.isnan(stats[7]) and np.isnan(stats[8]) and stats[3] == 0.0 and stats[1] == 0.5
    stats = torch.ops.abd.nwc_pair(orig, orig, orig, table)[5].cpu().numpy()             # nothing moved at all
    assert np.isnan(stats[6:]).all() and stats[0] == 160 and not stats[1:6].any()


# ------------------------------------------------------------------ 3. end to end
@pytest.fixture(scope="module")
def fixture_run(dev):
    """correlation_analysis on the golden fixture (its masks, its permutation), the float64 restatement and the
    stepwise twins (computed once)."""
    g = np.load(GOLDEN)
    c = FIXTURE
    st, cx, cy, bx, by = fixture_inputs(c)
    flat = st["fc1.weight"].shape[1]
    perm = g["perm"]
    host = {t: (unpack_mask(g[f"{t}_mask1"], flat).astype(np.uint8), unpack_mask(g[f"{t}_mask2"], 128).astype(np.uint8))
            for t in ("clean", "bd")}
    masks = tuple(tuple(torch.tensor(np.ascontiguousarray(m), device=dev) for m in host[t]) for t in ("clean", "bd"))
    sets = [torch.tensor(v, device=dev) for v in (cx, cy, bx, by)]
    bd_model = build(st, c["K"], dev)
    bd_model.engine(sets[0][:c["B"]])
    before = bd_model._engine.params.clone()
    res = D.correlation_analysis(bd_model, *sets, lr_un=c["lr"], unlearn_epochs=c["epochs"], batch_size=c["B"],
                                 order=perm, masks=masks)
    ref = analyse(st, (cx, cy), (bx, by), list(zip(*host["clean"])), list(zip(*host["bd"])), perm, c["B"], c["lr"])
    twins = []
    for (xs, ys), (m1, m2) in zip(((sets[0], sets[1]), (sets[2], sets[3])), masks):
        m = build(st, c["K"], dev)
        feed = iter(zip(m1, m2))
        m.step_masks = lambda B, device, feed=feed: next(feed)    # unlearn_epoch asks the model for its masks
        opt = torch.optim.Adam(m.parameters(), lr=c["lr"])
        steps = [D.unlearn_epoch(m, xs, ys, opt, record_layer=None, batch_size=c["B"], order=perm)[:2]
                 for _ in range(c["epochs"])]
        twins.append((m, opt, steps))
    return dict(res=res, ref=ref, twins=twins, bd_model=bd_model, before=before, st=st, g=g)


def test_correlation_analysis_equals_stepwise_composition(dev, fixture_run):
    f = fixture_run
    res, c = f["res"], FIXTURE
    assert torch.equal(f["bd_model"]._engine.params, f["before"])                    # read, never modified
    assert torch.equal(D._flat_params(f["bd_model"], dev), f["before"])
    assert res.names == D.neuron_names(None, "conv") and res.layer_type == "conv"
    for (twin, opt, steps), model, losses, accs, scores, text, absdiff in (
            (f["twins"][0], res.model_clean, res.clean_losses, res.clean_accs, res.clean_scores, res.ucn_clean,
             res.absdiff_clean),
            (f["twins"][1], res.model_bd, res.bd_losses, res.bd_accs, res.bd_scores, res.ucn_bd, res.absdiff_bd)):
        assert torch.equal(model._engine.params, twin._engine.params)
        assert torch.equal(model._engine.running, twin._engine.running) and model._engine.nbt.tolist() == [c["epochs"]] * 3
        assert torch.equal(model._engine.exp_avg, twin._engine.exp_avg)
        assert torch.equal(model._engine.exp_avg_sq, twin._engine.exp_avg_sq)
        assert [(lo, ac) for lo, ac in zip(losses, accs)] == steps                    # per-step loss and accuracy
        assert model._step == twin._step == c["epochs"]
        assert all(p.grad is not None and torch.equal(p.grad, q.grad) for p, q in zip(model._param_list(), twin._param_list()))
        names, s32, ad = D.neuron_weight_change(twin, f["st"], "conv")
        assert torch.equal(absdiff, ad) and scores.dtype == np.float64
        assert np.array_equal(scores.astype(np.float32), s32)                         # the same sums, rounded once
        assert text == D.ucn_text(names, s32)
    assert all(int(o.state[p]["step"]) == c["epochs"] for _, o, _ in f["twins"] for p in o.param_groups[0]["params"])
    out = torch.ops.abd.nwc_pair(f["before"], f["twins"][0][0]._engine.params, f["twins"][1][0]._engine.params,
                                 D.row_table(f["bd_model"], "conv"))
    s64, stats = out[4].cpu().numpy(), out[5].cpu().numpy()
    assert np.array_equal(res.clean_scores, s64[0]) and np.array_equal(res.bd_scores, s64[1])
    assert (res.correlation, res.slope, res.intercept) == (stats[6], stats[7], stats[8])
    assert (res.clean_unlr_loss, res.clean_unlr_acc) == (res.bd_losses[-1], res.bd_accs[-1])     # the reference's quirk
    host = D.correlation_stats(res.clean_scores, res.bd_scores)
    assert res.correlation == pytest.approx(host[0], rel=1e-12) and res.slope == pytest.approx(host[1], rel=1e-12)


def test_correlation_analysis_against_float64_restatement(dev, fixture_run):
    f = fixture_run
    res, ref = f["res"], f["ref"]
    for tag, losses, accs in (("clean", res.clean_losses, res.clean_accs), ("bd", res.bd_losses, res.bd_accs)):
        assert abs(losses[0] - ref[tag]["losses"][0]) <= RTOL * abs(ref[tag]["losses"][0])       # step 1
        assert accs[0] == ref[tag]["accs"][0]
    rel = max(np.abs(got - ref[tag]["scores"]).max() / ref[tag]["scores"].max()
              for tag, got in (("clean", res.clean_scores), ("bd", res.bd_scores)))
    rowrel = max((np.abs(got - ref[tag]["scores"]) / ref[tag]["scores"]).max()
                 for tag, got in (("clean", res.clean_scores), ("bd", res.bd_scores)))
    dr = abs(res.correlation - ref["r"])
    gold = abs(res.correlation - float(f["g"]["correlation"]))
    note(f"| fixture 32x13 K=10 B=16, 3 steps | {rowrel:.2e} | {rel:.2e} | {dr:.2e} | {gold:.2e} | "
         f"{res.correlation!r} | {ref['r']!r} |")
    assert rowrel <= SCORE_BOUND <= 1e-2
    assert dr <= R_BOUND


def test_save_outputs_from_a_device_result(dev, fixture_run, tmp_path):
    res = fixture_run["res"]
    D.save_correlation_outputs(res, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == sorted(D.CORRELATION_FILES)
    n2w = torch.load(tmp_path / "n2w_dict_bdunlr.pt", weights_only=False)
    assert n2w["conv1.weight.1"] == res.absdiff_bd[4:8].tolist()
    assert float(sum(n2w["conv3.weight.5"])) == pytest.approx(res.bd_scores[128 + 5], rel=256 * U)
    sd = torch.load(tmp_path / "unlearned_model_cleanunlr.pt", weights_only=True)
    assert torch.equal(sd["conv2.weight"].to(dev), res.model_clean.conv2.weight)


# ------------------------------------------------------------------ 4. opcheck
def test_opcheck_new_ops(dev):
    H, W, K, B, n = 32, 13, 10, 4, 2
    st, x, y = case_inputs(H, W, K, B, seed=190)
    flat = st["fc1.weight"].shape[1]
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    s = Side(st, K, dev, "f32split", xd)
    metrics = torch.zeros((n, L.METRICS_WORDS), dtype=torch.int64, device=dev)
    mo1 = torch.zeros((n, B, flat), dtype=torch.uint8, device=dev)
    mo2 = torch.zeros((n, B, 128), dtype=torch.uint8, device=dev)
    args = (xd, yd, s.e.params, s.e.grads, s.mm, s.mv, s.e.running, s.e.nbt, metrics)
    tail = (K, n, 1, LR, B1, B2, EPS, 3, 0)
    torch.library.opcheck(torch.ops.abd.smallcnn_unlearn_run.default, args + (None, None) + tail)
    torch.library.opcheck(torch.ops.abd.smallcnn_unlearn_run.default, args + (mo1, mo2) + tail,
                          dict(mask1_in=mo1.clone(), mask2_in=mo2.clone()))
    table = D.row_table(s.m, "conv")
    orig = s.e.params.clone()                                     # three different buffers: no NaN among the outputs
    moved = orig + 0.01 * torch.randn_like(orig)
    torch.library.opcheck(torch.ops.abd.nwc_pair.default, (orig, moved, orig * 1.5, table))
    torch.library.opcheck(torch.ops.abd.nwc_pair.default, (orig, moved, orig * 1.5, table, False))
