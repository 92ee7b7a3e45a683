"""Shared inputs and the float64 reference of the correlation-analysis tests (test_correlation_cpu.py,
test_gpu_correlation.py, tests/golden/make_correlation_golden.py).

``analyse`` restates correlation_analysis.py:128-158 in float64 numpy on top of tsbd_cases.Unlearner / nwc:
two copies of one state, each unlearned ``epochs`` times on the FIRST batch of the permuted set (the
reference's train_unlearning returns inside its batch loop and its loaders do not shuffle), the per-neuron
weight changes, their sequential double sums (Python's ``sum()`` over a list, :149-150), the Pearson
correlation pandas computes and the least-squares line sns.lmplot draws.
tests/golden/correlation_golden.npz pins it to the reference's own function (test_correlation_cpu.py).
"""
from __future__ import annotations

import numpy as np

from tsbd_cases import Unlearner, case_inputs, nwc

# The fixture (tests/golden/correlation_golden.npz): 2 batches of 16 rows, 3 unlearning epochs, Adam(1e-3)
FIXTURE = dict(H=32, W=13, K=10, B=16, n_batches=2, epochs=3, seed=11, lr=1e-3, target=3)
CSV_HEAD = "Clean_unlearn,Poison_unlearn\n"


def fixture_inputs(c=FIXTURE):
    """(state, clean_x, clean_y, bd_x, bd_y): the backdoor set is the clean one with a corner patch added to
    every row and every label set to the target class."""
    N = c["B"] * c["n_batches"]
    st, x, y = case_inputs(c["H"], c["W"], c["K"], N, c["seed"])
    bx = x.copy()
    bx[:, :, -4:, :3] += np.float32(1.5)
    by = np.full(N, c["target"], np.int64)
    return st, x, y, bx, by


def seq_sum(values):
    """Python's ``sum()`` over a list of floats: a sequential double sum starting from int 0."""
    return float(sum(float(v) for v in values))


def pearson(x, y):
    """Pearson r with the means taken first, then the centred sums; NaN for n < 2 or a constant column."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    dx, dy = x - x.mean(), y - y.mean()
    sxx, syy, sxy = (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum()
    if len(x) < 2 or sxx * syy == 0:
        return float("nan")
    return float(sxy / np.sqrt(sxx * syy))


def line_fit(x, y):
    """(slope, intercept) of the least-squares line of y over x; NaN for a constant x."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    dx = x - x.mean()
    sxx = (dx * dx).sum()
    if sxx == 0:
        return float("nan"), float("nan")
    slope = float((dx * (y - y.mean())).sum() / sxx)
    return slope, float(y.mean() - slope * x.mean())


def unlearn(state, x, y, masks, perm, B, lr, dropout_dtype="float32"):
    """len(masks) calls of train_unlearning on rows perm[:B] of (x, y).  Returns (Unlearner, losses, accs) with
    the reference's divisors: the number of batches and the size of the set."""
    un = Unlearner(state, lr, dropout_dtype=dropout_dtype)
    rows = np.asarray(perm)[:B]
    xb, yb = np.asarray(x)[rows], np.asarray(y)[rows]
    n_batches = -(-len(y) // B)
    losses, accs = [], []
    for mk in masks:
        _, loss, hits, _ = un.step(xb, yb, mk)
        losses.append(loss / n_batches)
        accs.append(hits / len(y))
    return un, losses, accs


def analyse(state, clean, bd, masks_clean, masks_bd, perm, B, lr, dropout_dtype="float32", layer_type="conv"):
    """The whole analysis in float64.  clean / bd: (x, y); masks_*: [(mask1, mask2)] per epoch."""
    orig = {k: np.asarray(v, np.float64) for k, v in state.items()}
    out = {}
    for tag, (x, y), masks in (("clean", clean, masks_clean), ("bd", bd, masks_bd)):
        un, losses, accs = unlearn(state, x, y, masks, perm, B, lr, dropout_dtype)
        names, sums, rows = nwc(un.m.state_dict(), orig, layer_type)
        out[tag] = dict(un=un, losses=losses, accs=accs, names=names, sums=sums, rows=rows,
                        scores=np.array([seq_sum(r) for r in rows]))
    x, y = out["clean"]["scores"], out["bd"]["scores"]
    out["r"] = pearson(x, y)
    out["slope"], out["intercept"] = line_fit(x, y)
    return out


def csv_text(clean_scores, bd_scores):
    """``DataFrame.to_csv(index=False)`` of the two columns: repr(float) values, '\\n' line ends."""
    return CSV_HEAD + "".join(f"{float(a)!r},{float(b)!r}\n" for a, b in zip(clean_scores, bd_scores))
