"""Shared inputs and the float64 reference of the neuron-ablation tests (test_ablation_cpu.py,
test_gpu_ablation.py, tests/golden/make_ablation_golden.py).

The reference value of a variant is always oracle.smallcnn's eval forward on PATCHED parameters
(``state[layer][idx] = 0`` as ft_reg.py:173-177 does); OracleSweep only skips the layers in front of
the earliest patched one, whose parameters -- and so whose outputs -- are the unpatched model's.
"""
from __future__ import annotations

import numpy as np

from golden_inputs import make_state, mfcc_like, rng
from oracle import smallcnn as oc

LAYERS = ((1, 0, 64), (2, 64, 64), (3, 128, 32))   # (layer, first mask column, channels)
NCOL = 160

# The fixture (tests/golden/ablation_golden.npz): the degenerate 32 x 13 geometry, 6 rows
FIXTURE = dict(H=32, W=13, K=10, B=6, seed=4)

# (H, W, K, B) -> seed of case_inputs, searched on the CPU (float64 oracle) for a top-2 log-prob margin
# above 3e-3 on every (variant, row) of the single-filter and general masks, both kinds
SEEDS = {(32, 40, 10, 5): 36, (32, 40, 10, 1): 31, (101, 40, 35, 5): 33, (101, 40, 35, 1): 30}


def single_masks():
    return np.eye(NCOL, dtype=np.uint8)


def general_masks():
    """empty / one channel per layer / all of conv2 / 57 of 64 conv1 channels + 3 conv3 / conv3 only"""
    m = np.zeros((5, NCOL), np.uint8)
    m[1, [3, 64 + 10, 128 + 5]] = 1
    m[2, 64:128] = 1
    m[3, np.r_[0:64][np.arange(64) % 9 != 4]] = 1      # 57 conv1 channels
    m[3, [128 + 0, 128 + 17, 128 + 31]] = 1
    m[4, [128 + 2, 128 + 30]] = 1
    assert m[3, :64].sum() == 57
    return m


def fixture_variants():
    """(masks (167, 160), kinds (167): 0 conv / 1 bn): 160 single filters, 4 bn weights, 3 multi-channel masks."""
    bn = np.zeros((4, NCOL), np.uint8)
    for i, col in enumerate((0, 63, 64 + 7, 128 + 31)):   # column 0 and 64 + 7 have negative gamma (make_state)
        bn[i, col] = 1
    masks = np.concatenate([single_masks(), bn, general_masks()[1:4]])
    kinds = np.r_[np.zeros(160, np.uint8), np.ones(4, np.uint8), np.zeros(3, np.uint8)]
    return masks, kinds


def case_inputs(H, W, K, B, seed):
    """(state, x (B,1,H,W) float32, y (B) int64) of one test case."""
    flat = oc.geometry(H, W)["flat"]
    st = make_state(H, W, K, flat, seed=seed, trained_bn=True)
    r = rng(1000 + seed)
    x = mfcc_like(r, B, H, W)
    y = r.integers(0, K, B).astype(np.int64)
    return st, x, y


def patched_state(state, mask, kind):
    """ft_reg.py:173-177 on a numpy state dict: <kind><i>.weight[c] = 0 for every set mask column."""
    st = dict(state)
    for i, first, c in LAYERS:
        idx = np.nonzero(mask[first:first + c])[0]
        if len(idx):
            key = f"{kind}{i}.weight"
            st[key] = np.array(st[key], copy=True)
            st[key][idx] = 0.0
    return st


def conv2x2(x, w, b):
    """oracle.smallcnn.conv2x2 as four BLAS products over contiguous tap slices (same float64 sums,
    several times faster; test_ablation_cpu.py pins OracleSweep to SmallCNN.forward_eval)."""
    B, C, H, W = x.shape
    out = np.empty((B, w.shape[0], H - 1, W - 1))
    out[:] = b[None, :, None, None]
    for kh in range(2):
        for kw in range(2):
            xs = np.ascontiguousarray(x[:, :, kh:kh + H - 1, kw:kw + W - 1])
            out += np.tensordot(w[:, :, kh, kw], xs, axes=([1], [1])).transpose(1, 0, 2, 3)
    return out


class OracleSweep:
    """float64 eval log-probs of patched models on one batch, the baseline's activations cached."""

    def __init__(self, state, x):
        self.state = state
        self.h = {1: np.asarray(x, np.float64)}
        m = oc.SmallCNN(state)
        for i in (1, 2, 3):
            self.h[i + 1] = self._layer(m, i, self.h[i])

    @staticmethod
    def _layer(m, i, h):
        p, b = m.p, m.buf
        h = np.maximum(conv2x2(h, p[f"conv{i}.weight"], p[f"conv{i}.bias"]), 0.0)
        h = oc.bn_eval(h, p[f"bn{i}.weight"], p[f"bn{i}.bias"], b[f"bn{i}.running_mean"], b[f"bn{i}.running_var"])
        return oc.maxpool(h, *oc.POOLS[i])[0]

    def logp(self, mask, kind="conv"):
        m = oc.SmallCNN(patched_state(self.state, mask, kind))
        first = [i for i, f, c in LAYERS if mask[f:f + c].any()]
        k = first[0] if first else 4
        h = self.h[k]
        for i in range(k, 4):
            h = self._layer(m, i, h)
        h = h.reshape(h.shape[0], -1)
        h = np.maximum(h @ m.p["fc1.weight"].T + m.p["fc1.bias"], 0.0)
        return oc.log_softmax(h @ m.p["fc2.weight"].T + m.p["fc2.bias"])


def ce_rows(logp, y):
    """nn.CrossEntropyLoss(reduction='none') on the model's log-prob output."""
    lp = oc.log_softmax(logp)
    return -lp[np.arange(len(y)), y]


def top2_margin(logp):
    s = np.sort(logp, axis=1)
    return s[:, -1] - s[:, -2]


def oracle_case(state, x, y, masks, kind):
    """Per variant: row losses (V, B), predictions (V, B), the smallest top-2 log-prob margin."""
    sw = OracleSweep(state, x)
    loss = np.empty((len(masks), len(y)))
    pred = np.empty((len(masks), len(y)), np.int64)
    margin = np.inf
    for v, m in enumerate(masks):
        lp = sw.logp(m, kind)
        loss[v] = ce_rows(lp, y)
        pred[v] = lp.argmax(1)
        margin = min(margin, float(top2_margin(lp).min()))
    return loss, pred, margin
