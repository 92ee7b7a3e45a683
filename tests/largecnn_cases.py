"""Fixture of the largecnn tests: deterministic cases and a float64 restatement of the model.

Per case (numpy-seeded): the 16 parameters under the reference's state_dict names, an input, labels, poison
indicators and the two dropout keep-masks.  The channel widths are fixed by the model (about 3.4 M conv
parameters plus 256 * linear_features of fc1), so the parameters are drawn, never committed.  Weights and biases
are drawn 2.5 times wider than torch's default U(-1/sqrt(fan_in), 1/sqrt(fan_in)): the signal then keeps its
size through the five convs, and a dropped bias moves the log-probabilities far past the bound.

``restate`` restates utils/models.py:68-119 from torch functional primitives, returning every activation the
device saves.  In float64 it is the oracle of the GPU tests (the reference checkout is not on the GPU machine);
tests/test_largecnn_cpu.py ties it to the reference's own module through tests/golden/largecnn_golden.npz.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

SMALL_TILE = 64     # edge of the small GEMM block tile             (abd_largecnn_tile_info 0)
LARGE_TILE = 128    # edge of the large GEMM block tile             (abd_largecnn_tile_info 1)
SLICE_ROWS = 256    # least pixels of one weight-gradient slice     (abd_largecnn_tile_info 2)
COLSUM_ROWS = 512   # rows above which column sums take two stages  (abd_largecnn_tile_info 3)
LARGE_MIN_BLOCKS = 96   # least count of large tiles for the large tile to be used (abd_largecnn_tile_info 4)
MAX_SLICES = 16     # most slices of a weight gradient              (abd_largecnn_tile_info 5)

CONVS = (("conv1", 1, 96), ("conv2", 96, 256), ("conv3", 256, 384), ("conv4", 384, 384), ("conv5", 384, 256))
FC1, FC2 = 256, 128
PARAM_ORDER = tuple(f"{m}.{p}" for m in ("conv1", "conv2", "conv3", "conv4", "conv5", "fc1", "fc2", "fc3")
                    for p in ("weight", "bias"))

# The smallest B at 12 x 16 whose conv2 pixels (B * 6 * 8) exceed COLSUM_ROWS (conv1's and conv2's bias column
# sums take two stages) and make two weight-gradient slices (>= 2 * SLICE_ROWS); 48 B and 12 B (conv3..conv5)
# are then no multiple of either M tile.
RAGGED_B = COLSUM_ROWS // 48 + 1

# name -> (B, H, W, K, seed)
CASES = {
    "tiny": (2, 12, 12, 3, 1),          # smallest accepted input: maps after pool2 are 3 x 3, pool3 gives 1 x 1
    "odd": (2, 13, 15, 5, 2),           # both 2 x 2 pools drop a row and a column
    "flowmur": (3, 32, 13, 10, 3),      # linear_features 768; pool3 output width 1
    "daba": (2, 32, 40, 10, 4),         # linear_features 3072
    # linear_features 12288: fc1 at its largest K; odd H.  B = 3 is the smallest batch at which every conv weight
    # gradient has LARGE_MIN_BLOCKS blocks of the large tile (750 conv3..conv5 pixels make two slices) and so runs
    # it by the kernels' own choice, with ragged pixel slices (tests/test_largecnn_cpu.py does the count)
    "jingleback": (3, 101, 40, 10, 5),
    "ragged_batch": (RAGGED_B, 12, 16, 10, 6),
    "k1": (2, 12, 12, 1, 7),            # K = 1: loss 0, every gradient exactly 0
    "k35": (2, 12, 16, 35, 8),
}

# (case, tensor) -> bound of the device result where 1e-4 does not hold: four times the float32 CPU
# restatement's own distance from float64 at that case (profiles/largecnn/parity.md).  Everything else: 1e-4.
BOUNDS: dict = {}

WIDEN = 2.5
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
SAMPLE_MAX = 1024
FULL_GRADS = ("conv1.weight", "conv1.bias", "fc3.weight", "fc3.bias")   # recorded in full in the golden file
ACTIVATIONS = ("a1", "p1", "a2", "p2", "a3", "a4", "a5", "p3", "h1", "h2", "logits")


def bound(name, tensor, default=1e-4):
    return BOUNDS.get((name, tensor), default)


def linear_features(H, W):
    return 256 * ((H // 4 - 3) // 2 + 1) * ((W // 4 - 3) // 2 + 1)


def param_shapes(lf, K):
    s = {}
    for n, cin, cout in CONVS:
        s[f"{n}.weight"], s[f"{n}.bias"] = (cout, cin, 3, 3), (cout,)
    for n, i, o in (("fc1", lf, FC1), ("fc2", FC1, FC2), ("fc3", FC2, K)):
        s[f"{n}.weight"], s[f"{n}.bias"] = (o, i), (o,)
    return {n: s[n] for n in PARAM_ORDER}


def plan_slices(rows, max_slices=MAX_SLICES, min_rows=SLICE_ROWS, k_step=32):
    """net_common.inc's plan_slices: (slices, rows per slice) of a reduction over `rows` rows."""
    ksplit = max(1, min(max_slices, rows // min_rows))
    kchunk = -(-rows // ksplit)
    kchunk = -(-kchunk // k_step) * k_step
    return -(-rows // kchunk), kchunk


def large_blocks(name):
    """Per conv2..conv5 GEMM of a case, the count of 128 x 128 blocks launch_gemm compares with LARGE_MIN_BLOCKS:
    {(layer, 'fwd' | 'dgrad' | 'wgrad'): blocks}."""
    B, H, W, K, _ = CASES[name]
    t = lambda n: -(-n // LARGE_TILE)   # noqa: E731
    out = {}
    for layer, cin, cout in CONVS[1:]:
        px = B * (H // 2) * (W // 2) if layer == "conv2" else B * (H // 4) * (W // 4)
        out[layer, "fwd"] = t(px) * t(cout)
        out[layer, "dgrad"] = t(px) * t(cin)
        out[layer, "wgrad"] = t(cout) * t(cin) * 9 * plan_slices(px)[0]
    return out


def make_state(name):
    """The case's state_dict as float32 numpy arrays."""
    B, H, W, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(5000 + seed))
    out = {}
    for n, shp in param_shapes(linear_features(H, W), K).items():
        fan = int(np.prod(shp[1:])) if n.endswith("weight") else int(np.prod(out[n.replace("bias", "weight")].shape[1:]))
        out[n] = (WIDEN * r.uniform(-1, 1, shp) / np.sqrt(fan)).astype(np.float32)
    return out


def make_inputs(name):
    """x (B,1,H,W) float32, labels, indicators (int64), mask1 (B,256), mask2 (B,128) uint8."""
    B, H, W, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(6000 + seed))
    x = r.normal(size=(B, 1, H, W)).astype(np.float32)
    y = r.integers(0, K, B).astype(np.int64)
    ind = (r.uniform(size=B) < 0.4).astype(np.int64)
    m1 = (r.uniform(size=(B, FC1)) < 0.5).astype(np.uint8)
    m2 = (r.uniform(size=(B, FC2)) < 0.5).astype(np.uint8)
    return x, y, ind, m1, m2


def restate(p, x, masks=None):
    """utils/models.py:96-119 on parameters p (name -> tensor): every activation by the name the device saves
    it under, in the reference's own (B, C, H, W) layout.  masks: the two keep-masks of a train-mode forward
    (scale 2), None for eval."""
    a = {}
    a["a1"] = F.conv2d(x, p["conv1.weight"], p["conv1.bias"], padding=1)
    a["p1"] = F.max_pool2d(a["a1"], 2)
    a["a2"] = F.conv2d(a["p1"], p["conv2.weight"], p["conv2.bias"], padding=1)
    a["p2"] = F.max_pool2d(a["a2"], 2)
    a["a3"] = F.relu(F.conv2d(a["p2"], p["conv3.weight"], p["conv3.bias"], padding=1))
    a["a4"] = F.relu(F.conv2d(a["a3"], p["conv4.weight"], p["conv4.bias"], padding=1))
    a["a5"] = F.relu(F.conv2d(a["a4"], p["conv5.weight"], p["conv5.bias"], padding=1))
    a["p3"] = F.max_pool2d(a["a5"], 3, stride=2)
    h = F.relu(F.linear(a["p3"].flatten(1), p["fc1.weight"], p["fc1.bias"]))
    a["h1"] = h * masks[0].to(h.dtype) * 2.0 if masks is not None else h
    h = F.relu(F.linear(a["h1"], p["fc2.weight"], p["fc2.bias"]))
    a["h2"] = h * masks[1].to(h.dtype) * 2.0 if masks is not None else h
    a["logits"] = F.log_softmax(F.linear(a["h2"], p["fc3.weight"], p["fc3.bias"]), dim=1)
    return a


_CACHE: dict = {}


def run_case(name, dtype=torch.float64):
    """Everything the tests compare against, computed once per (case, dtype) and shared (read only): the
    eval-mode log-probabilities and loss, the train-mode activations, loss and the 16 gradients."""
    key = (name, dtype)
    if key in _CACHE:
        return _CACHE[key]
    x, y, ind, m1, m2 = make_inputs(name)
    xt, yt = torch.tensor(x, dtype=dtype), torch.tensor(y)
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in make_state(name).items()}
    out = {}
    with torch.no_grad():
        ev = restate(p, xt)["logits"]
        out["eval_logits"], out["eval_loss"] = ev, F.cross_entropy(ev, yt)
    acts = restate(p, xt, (torch.tensor(m1), torch.tensor(m2)))
    loss = F.cross_entropy(acts["logits"], yt)   # log_softmax a second time, as the reference trains
    loss.backward()
    out["acts"] = {k: v.detach() for k, v in acts.items()}
    out["loss"] = loss.detach()
    out["grads"] = {n: p[n].grad.detach().clone() for n in PARAM_ORDER}
    _CACHE[key] = out
    return out


def channels_first(t, shape):
    """A saved channels-last (B, H, W, C) device map as (B, C, H, W); shape is the (B, C, H, W) wanted."""
    B, Cc, H, W = shape
    return t.reshape(B, H, W, Cc).permute(0, 3, 1, 2)


def rel_err(a, b):
    """max |a - b| relative to the largest magnitude of the reference b."""
    a = torch.as_tensor(a, dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(b, dtype=torch.float64).reshape(-1)
    d = float((a - b).abs().max())
    s = float(b.abs().max())
    return d / s if s > 0 else d


def digest(t):
    """What the golden file stores of a large gradient tensor: float64 (sum, L2 norm) and a fixed-stride
    sample of at most 1024 elements."""
    f = np.asarray(t, dtype=np.float64).reshape(-1)
    stride = max(1, -(-f.size // SAMPLE_MAX))
    return np.array([f.sum(), np.sqrt((f * f).sum())]), f[::stride]


DIGEST_MODELS = ((10, 768), (35, 3072))   # (num_classes, linear_features) whose seeded init is compared
DIGEST_SEED = 1234
