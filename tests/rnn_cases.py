"""Fixture of the RNN tests: deterministic cases and a float64 restatement of the model.

Per case (numpy-seeded): the 14 parameters under the reference's state_dict names, an input, labels and
poison indicators.  H = 768 is fixed by the model, so the roughly 12 M parameters are drawn, never
committed.  Weights AND biases are drawn three times wider than torch's default U(-1/sqrt(768), 1/sqrt(768)):
the gate pre-activations reach the saturating range and a dropped bias moves the logits far past the bound.

``Restated`` restates utils/models.py:231-257 from torch CPU primitives (nn.LSTM from zero states, linear on
the last step); ``unroll`` steps the three layers one time step at a time for the h / c / activated gates the
device saves.  In float64 this is the oracle of the GPU tests (the reference checkout is not on the GPU
machine); tests/test_rnn_cpu.py ties it to the reference's own module through tests/golden/rnn_golden.npz.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

H, LAYERS = 768, 3
REC_ROWS = 32       # batch rows of a recurrent workgroup           (abd_rnn_tile_info 0)
SMALL_TILE = 64     # edge of the small GEMM block tile             (abd_rnn_tile_info 1)
LARGE_TILE = 128    # edge of the large GEMM block tile             (abd_rnn_tile_info 2)
SLICE_ROWS = 256    # least rows of one weight-gradient slice       (abd_rnn_tile_info 3)
COLSUM_ROWS = 512   # rows above which column sums take two stages  (abd_rnn_tile_info 4)
LARGE_MIN_BLOCKS = 96   # least count of large tiles for the large tile to be used (abd_rnn_tile_info 5)

# name -> (B, T, F, K, seed).  The seeds are picked so that the float32 restatement stays within 1e-5 of the
# float64 one and every row's top-2 logit gap exceeds 1e-3 (asserted in tests/test_rnn_cpu.py).
CASES = {
    "tiny": (3, 4, 13, 10, 1),             # B below a tile; F = 13 below one K-step and no multiple of 4
    "one_step": (1, 1, 13, 10, 2),         # one row; the recurrent GEMM never runs; dW_hh exactly 0
    "ragged_tiles": (2 * REC_ROWS + 1, 5, 40, 35, 3),   # two full recurrent row tiles plus a ragged one; B*T = 325
                                           # = 5 small GEMM tiles + 5 rows
    "long": (5, 101, 40, 10, 4),           # odd T; 303 chained cell updates
    "one_class": (2, 3, 1, 1, 5),          # F = 1; K = 1: loss 0 and every gradient 0
    "cap_seq": (1, 1024, 1, 10, 6),        # T at the cap
    "wide": (2, 3, 128, 200, 7),           # F at the cap; K past one N-tile (64) of the head
    # B*T = 513: the smallest B at T = 3 with B*T // SLICE_ROWS = 2 slices of the weight gradients AND more than
    # COLSUM_ROWS rows (two-stage column sums).  It is also the only case whose input projection (5 x 24 large
    # tiles >= LARGE_MIN_BLOCKS) and weight gradients (24 x 6 x 2) run the 128 x 128 tile, ragged in M.
    "big_batch": (COLSUM_ROWS // 3 + 1, 3, 16, 10, 8),
}

# (case, tensor) -> bound of the device result where float32 on the CPU misses 1e-5: ten times the float32-CPU
# distance measured for that seed.  Everything else: 1e-4.
BOUNDS: dict = {}

PARAM_ORDER = (
    *[f"lstm.{n}_l{k}" for k in range(LAYERS) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")],
    "fc.weight", "fc.bias",
)
WIDEN = 3.0
X_SIGMA = 2.0
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
SAMPLE_MAX = 1024
LSTM_GRADS = PARAM_ORDER[:-2]


def bound(name, tensor, default=1e-4):
    return BOUNDS.get((name, tensor), default)


def param_shapes(Fd, K):
    s = {}
    for k in range(LAYERS):
        s[f"lstm.weight_ih_l{k}"] = (4 * H, Fd if k == 0 else H)
        s[f"lstm.weight_hh_l{k}"] = (4 * H, H)
        s[f"lstm.bias_ih_l{k}"] = (4 * H,)
        s[f"lstm.bias_hh_l{k}"] = (4 * H,)
    s["fc.weight"] = (K, H)
    s["fc.bias"] = (K,)
    return {n: s[n] for n in PARAM_ORDER}


def make_state(name):
    """The case's state_dict as float32 numpy arrays."""
    B, T, Fd, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(3000 + seed))
    return {n: (WIDEN * r.uniform(-1, 1, shp) / np.sqrt(H)).astype(np.float32) for n, shp in param_shapes(Fd, K).items()}


def make_inputs(name):
    """x (B,1,T,F) float32, labels, indicators (int64)."""
    B, T, Fd, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(4000 + seed))
    x = (X_SIGMA * r.normal(size=(B, 1, T, Fd))).astype(np.float32)
    y = r.integers(0, K, B).astype(np.int64)
    ind = (r.uniform(size=B) < 0.4).astype(np.int64)
    return x, y, ind


class Restated(nn.Module):
    """utils/models.py:231-257 from torch primitives, in any dtype (the reference casts its input to float32)."""

    def __init__(self, state, dtype=torch.float64):
        super().__init__()
        Fd = state["lstm.weight_ih_l0"].shape[1]
        self.lstm = nn.LSTM(Fd, H, LAYERS, batch_first=True)
        self.fc = nn.Linear(H, state["fc.weight"].shape[0])
        self.to(dtype)
        self.load_state_dict({k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in state.items()})

    def forward(self, x):
        x = x.squeeze(1)
        z = x.new_zeros((LAYERS, x.shape[0], H))
        out, _ = self.lstm(x, (z, z))
        return self.fc(out[:, -1, :])

    def grads(self):
        d = dict(self.named_parameters())
        return {n: d[n].grad.detach().clone() for n in PARAM_ORDER}


def unroll(x, lstm):
    """Step the stack one time step at a time: per layer (h, c, gates) with h, c (B, T, 768) and gates
    (B, T, 3072) activated, torch order i f g o."""
    B, T, _ = x.shape
    out = []
    inp = x
    for k in range(LAYERS):
        wi, wh = getattr(lstm, f"weight_ih_l{k}"), getattr(lstm, f"weight_hh_l{k}")
        b = getattr(lstm, f"bias_ih_l{k}") + getattr(lstm, f"bias_hh_l{k}")
        xp = inp @ wi.T + b
        h = x.new_zeros((B, H))
        c = x.new_zeros((B, H))
        hs, cs, gs = [], [], []
        for t in range(T):
            z = xp[:, t] + h @ wh.T
            i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), \
                torch.sigmoid(z[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            hs.append(h)
            cs.append(c)
            gs.append(torch.cat([i, f, g, o], 1))
        inp = torch.stack(hs, 1)
        out.append((inp, torch.stack(cs, 1), torch.stack(gs, 1)))
    return out


_CACHE: dict = {}


def run_case(name, dtype=torch.float64, states=True):
    """Everything the tests compare against, computed once per (case, dtype) and shared (read only): logits,
    loss, gradients and (states) the unrolled h / c / gates."""
    key = (name, dtype)
    if key in _CACHE and (not states or "states" in _CACHE[key]):
        return _CACHE[key]
    out = _CACHE.get(key)
    x, y, ind = make_inputs(name)
    xt, yt = torch.tensor(x, dtype=dtype), torch.tensor(y)
    if out is None:
        out = {}
        m = Restated(make_state(name), dtype)
        logits = m(xt)
        loss = F.cross_entropy(logits, yt)
        loss.backward()
        out["logits"], out["loss"] = logits.detach(), loss.detach()
        out["grads"] = m.grads()
        out["_model"] = m
    if states:
        with torch.no_grad():
            out["states"] = unroll(xt.squeeze(1), out["_model"].lstm)
    _CACHE[key] = out
    return out


def rel_err(a, b):
    """max |a - b| relative to the largest magnitude of the reference b."""
    a = torch.as_tensor(a, dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(b, dtype=torch.float64).reshape(-1)
    d = float((a - b).abs().max())
    s = float(b.abs().max())
    return d / s if s > 0 else d


def digest(t):
    """What the golden file stores of an LSTM gradient tensor: float64 (sum, L2 norm) and a fixed-stride sample
    of at most 1024 elements (stored as float32: the reference
    computes in float32)."""
    f = np.asarray(t, dtype=np.float64).reshape(-1)
    stride = max(1, -(-f.size // SAMPLE_MAX))
    return np.array([f.sum(), np.sqrt((f * f).sum())]), f[::stride]


DIGEST_MODELS = ((10, 40), (35, 13))   # (num_classes, time_len) whose seeded init is compared with a plain build
DIGEST_SEED = 1234
# Cases recorded from the reference's own module.  wide (a 200 x 768 fc gradient in full) and cap_seq would take
# the golden file past its size limit; they are compared with the restatement only, which the other cases pin to the
# reference and which is parametric in T, F and K.
GOLDEN_CASES = ("tiny", "one_step", "ragged_tiles", "long", "one_class", "big_batch")
