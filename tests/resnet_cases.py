"""Fixture of the ResNet tests: deterministic cases and a float64 restatement of the model.

Per case (numpy-seeded): the 49 parameters and 45 buffers under the reference's state_dict names, an input, labels
and poison indicators.  Conv and linear weights are drawn 2.5 times wider than torch's default
U(-1/sqrt(fan_in), 1/sqrt(fan_in)); BatchNorm weights in U(0.5, 1.5) and biases in U(-0.5, 0.5), away from 1 and
0, so a dropped gamma or beta shows; running means in U(-0.5, 0.5), running variances in U(0.5, 2) and
num_batches_tracked = 3 + the unit's index, so a step that ignores the old running value shows.

``restate`` restates utils/models.py:261-332 from torch functional primitives, returning every map the device
saves and the BatchNorm batch statistics.  In float64 it is the oracle of the GPU tests (the reference checkout is
not on the GPU machine); tests/test_resnet_cpu.py ties it to the reference's own module through
tests/golden/resnet_golden.npz.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

TILE_ROWS = 64      # rows of a GEMM block tile                      (abd_resnet_tile_info 0)
K_STEP = 16         # the K-step                                     (abd_resnet_tile_info 1)
SLICE_ROWS = 512    # least pixels of one weight-gradient slice      (abd_resnet_tile_info 2)
MAX_SLICES = 128    # most slices of a weight gradient               (abd_resnet_tile_info 3)
STAT_ROWS = 1024    # least pixels of one BatchNorm partial block    (abd_resnet_tile_info 4)
STAT_BLOCKS = 256   # most such blocks                               (abd_resnet_tile_info 5)

# (conv, bn, Cin, Cout, stride) in named_parameters() order
UNITS = (
    ("conv", "bn", 1, 16, 1),
    ("layer1.0.conv1", "layer1.0.bn1", 16, 16, 1), ("layer1.0.conv2", "layer1.0.bn2", 16, 16, 1),
    ("layer1.1.conv1", "layer1.1.bn1", 16, 16, 1), ("layer1.1.conv2", "layer1.1.bn2", 16, 16, 1),
    ("layer2.0.conv1", "layer2.0.bn1", 16, 32, 2), ("layer2.0.conv2", "layer2.0.bn2", 32, 32, 1),
    ("layer2.0.downsample.0", "layer2.0.downsample.1", 16, 32, 2),
    ("layer2.1.conv1", "layer2.1.bn1", 32, 32, 1), ("layer2.1.conv2", "layer2.1.bn2", 32, 32, 1),
    ("layer3.0.conv1", "layer3.0.bn1", 32, 64, 2), ("layer3.0.conv2", "layer3.0.bn2", 64, 64, 1),
    ("layer3.0.downsample.0", "layer3.0.downsample.1", 32, 64, 2),
    ("layer3.1.conv1", "layer3.1.bn1", 64, 64, 1), ("layer3.1.conv2", "layer3.1.bn2", 64, 64, 1),
)
# (the unit whose output the block reads, conv1 unit, conv2 unit, downsample unit or -1)
BLOCKS = ((0, 1, 2, -1), (2, 3, 4, -1), (4, 5, 6, 7), (6, 8, 9, -1), (9, 10, 11, 12), (11, 13, 14, -1))
PARAM_ORDER = tuple(n for cv, bn, *_ in UNITS for n in (f"{cv}.weight", f"{bn}.weight", f"{bn}.bias")) + (
    "conv2d.weight", "conv2d.bias", "fc.weight", "fc.bias")
BUFFER_ORDER = tuple(f"{bn}.{b}" for _, bn, *_ in UNITS for b in ("running_mean", "running_var",
                                                                  "num_batches_tracked"))
MIN_H, MIN_W = 25, 13


def half(n):
    return (n - 1) // 2 + 1


def plan_slices(rows, max_slices=MAX_SLICES, min_rows=SLICE_ROWS, k_step=K_STEP):
    """net_common.inc's plan_slices: (slices, rows per slice) of a reduction over `rows` rows."""
    ksplit = max(1, min(max_slices, rows // min_rows))
    kchunk = -(-rows // ksplit)
    kchunk = -(-kchunk // k_step) * k_step
    return -(-rows // kchunk), kchunk


def ragged_batch(stat_rows=STAT_ROWS, slice_rows=SLICE_ROWS, tile_rows=TILE_ROWS, max_slices=MAX_SLICES,
                 k_step=K_STEP):
    """The smallest B at 25 x 13 whose layer-1 pixels (325 B) exceed one BatchNorm partial block, make at least
    two weight-gradient slices and are no multiple of the M tile."""
    B = 1
    while not (325 * B > stat_rows and plan_slices(325 * B, max_slices, slice_rows, k_step)[0] >= 2
               and (325 * B) % tile_rows):
        B += 1
    return B


RAGGED_B = ragged_batch()

# name -> (B, H, W, K, seed)
CASES = {
    "tiny": (2, 25, 13, 3, 1),          # smallest accepted input: every stage has odd sides (25 13 7 4, 13 7 4)
    "b1": (1, 25, 13, 3, 2),            # BatchNorm over one clip
    "odd": (5, 27, 17, 5, 3),           # 27 14 7, 17 9 5: the average pool drops a column
    "flowmur": (3, 32, 13, 10, 4),      # linear_features 64
    "daba": (2, 32, 40, 10, 5),         # linear_features 128, PW = 2
    "jingleback": (2, 101, 40, 10, 6),  # linear_features 384, PH = 3, H4 = 13: the average pool drops a row
    "k1": (2, 25, 13, 1, 7),            # K = 1: loss 0, every gradient exactly 0
    "k35": (2, 25, 16, 35, 8),
    "ragged": (RAGGED_B, 25, 13, 10, 9),
    # the stem's BatchNorm input has a channel mean of at least ten standard deviations (OFFSET below)
    "offset": (2, 25, 13, 3, 10),
}
# `offset`: the input is 15 + N(0, 1) and the stem kernel is drawn with a positive mean, all of it on the centre
# tap (1 + 0.25 U there, 0.02 U elsewhere, times the usual width): off-centre taps with a mean would turn the
# input's offset into a step at the zero padding, whose spread would hide the effect.
OFFSET_X = 15.0

# (case, tensor) -> bound of the device result where 1e-4 does not hold: four times the float32 CPU
# restatement's own distance from float64 at that case (profiles/resnet/parity.md).  Everything else: 1e-4.
BOUNDS: dict = {}

WIDEN = 2.5
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
SAMPLE_MAX = 64
FULL_GRADS = ("conv.weight", "conv2d.weight", "conv2d.bias", "fc.weight", "fc.bias")   # in full in the golden file
FULL_RUNNING = ("bn", "layer3.1.bn2")


def bound(name, tensor, default=1e-4):
    return BOUNDS.get((name, tensor), default)


def geometry(H, W):
    """(H2, W2, H3, W3, H4, PH, PW)"""
    H2, W2 = half(H), half(W)
    H3, W3 = half(H2), half(W2)
    H4 = half(H3)
    return H2, W2, H3, W3, H4, H4 // 4, W3 // 4


def linear_features(H, W):
    if H < MIN_H or W < MIN_W:
        return -1
    *_, PH, PW = geometry(H, W)
    return 64 * PH * PW


def param_shapes(lf, K):
    s = {}
    for cv, bn, cin, cout, _ in UNITS:
        s[f"{cv}.weight"], s[f"{bn}.weight"], s[f"{bn}.bias"] = (cout, cin, 3, 3), (cout,), (cout,)
    s["conv2d.weight"], s["conv2d.bias"] = (64, 64, 1, 1), (64,)
    s["fc.weight"], s["fc.bias"] = (K, lf), (K,)
    return {n: s[n] for n in PARAM_ORDER}


def unit_stage(u):
    """Stage (1..3) of unit u's output map."""
    return {16: 1, 32: 2, 64: 3}[UNITS[u][3]]


def unit_shape(u, B, H, W):
    """(B, C, h, w) of unit u's output map."""
    H2, W2, H3, W3, *_ = geometry(H, W)
    h, w = ((H, W), (H2, W2), (H3, W3))[unit_stage(u) - 1]
    return B, UNITS[u][3], h, w


def make_state(name):
    """The case's state_dict (parameters and buffers) as numpy arrays."""
    B, H, W, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(7000 + seed))
    out = {}
    bns = {bn for _, bn, *_ in UNITS}
    for n, shp in param_shapes(linear_features(H, W), K).items():
        mod = n.rsplit(".", 1)[0]
        if mod in bns:
            out[n] = (r.uniform(0.5, 1.5, shp) if n.endswith("weight") else r.uniform(-0.5, 0.5, shp)).astype(np.float32)
            continue
        fan = int(np.prod(shp[1:])) if n.endswith("weight") else int(np.prod(out[n.replace("bias", "weight")].shape[1:]))
        out[n] = (WIDEN * r.uniform(-1, 1, shp) / np.sqrt(fan)).astype(np.float32)
    if name == "offset":
        w = 0.02 * r.uniform(-1, 1, (16, 1, 3, 3))
        w[:, :, 1, 1] = 1.0 + 0.25 * r.uniform(-1, 1, (16, 1))
        out["conv.weight"] = (WIDEN / 3.0 * w).astype(np.float32)
    for u, (_, bn, _, cout, _) in enumerate(UNITS):
        out[f"{bn}.running_mean"] = r.uniform(-0.5, 0.5, cout).astype(np.float32)
        out[f"{bn}.running_var"] = r.uniform(0.5, 2.0, cout).astype(np.float32)
        out[f"{bn}.num_batches_tracked"] = np.array(3 + u, dtype=np.int64)
    return out


def make_inputs(name):
    """x (B,1,H,W) float32, labels, indicators (int64)."""
    B, H, W, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(8000 + seed))
    x = r.normal(size=(B, 1, H, W)).astype(np.float32)
    if name == "offset":
        x = (x + OFFSET_X).astype(np.float32)
    y = r.integers(0, K, B).astype(np.int64)
    ind = (r.uniform(size=B) < 0.4).astype(np.int64)
    return x, y, ind


def restate(p, bufs, x, train):
    """utils/models.py:277-332 on parameters p and buffers bufs (name -> tensor): every map by the name the
    device saves it under, in the reference's own (B, C, H, W) layout: z<u> unit u's conv output, a<u> what its
    BatchNorm pass gives (after the residual add and the relu where the unit has them), mean<u> / var<u> the
    batch mean and biased variance (train) or the running ones (eval), c2, pool, logits.  train: returns the
    updated running statistics too, as 'run/<buffer name>'; bufs itself is left unchanged."""
    a = {}

    def unit(u, inp, res=None, relu=True):
        cv, bn, _, _, stride = UNITS[u]
        z = F.conv2d(inp, p[f"{cv}.weight"], None, stride=stride, padding=1)
        rm, rv = bufs[f"{bn}.running_mean"].clone(), bufs[f"{bn}.running_var"].clone()
        if train:
            a[f"mean{u}"], a[f"var{u}"] = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        else:
            a[f"mean{u}"], a[f"var{u}"] = rm, rv
        y = F.batch_norm(z, rm, rv, p[f"{bn}.weight"], p[f"{bn}.bias"], train, BN_MOMENTUM, BN_EPS)
        if train:
            a[f"run/{bn}.running_mean"], a[f"run/{bn}.running_var"] = rm, rv
            a[f"run/{bn}.num_batches_tracked"] = bufs[f"{bn}.num_batches_tracked"] + 1
        if res is not None:
            y = y + res
        if relu:
            y = F.relu(y)
        a[f"z{u}"], a[f"a{u}"] = z, y
        return y

    unit(0, x)
    for i, u1, u2, ud in BLOCKS:
        unit(u1, a[f"a{i}"])
        res = unit(ud, a[f"a{i}"], relu=False) if ud >= 0 else a[f"a{i}"]
        unit(u2, a[f"a{u1}"], res=res)
    a["c2"] = F.conv2d(a["a14"], p["conv2d.weight"], p["conv2d.bias"], stride=(2, 1))
    a["pool"] = F.avg_pool2d(a["c2"], 4)
    a["logits"] = F.linear(a["pool"].flatten(1), p["fc.weight"], p["fc.bias"])
    return a


_CACHE: dict = {}


def run_case(name, dtype=torch.float64):
    """Everything the tests compare against, computed once per (case, dtype) and shared (read only): the
    eval-mode logits and loss, the train-mode maps, statistics, loss, the 49 gradients and the running statistics
    after the step."""
    key = (name, dtype)
    if key in _CACHE:
        return _CACHE[key]
    x, y, ind = make_inputs(name)
    xt, yt = torch.tensor(x, dtype=dtype), torch.tensor(y)
    st = make_state(name)
    p = {k: torch.tensor(st[k], dtype=dtype, requires_grad=True) for k in PARAM_ORDER}
    bufs = {k: torch.tensor(st[k], dtype=dtype if st[k].dtype != np.int64 else torch.int64) for k in BUFFER_ORDER}
    out = {}
    with torch.no_grad():
        ev = restate(p, bufs, xt, False)["logits"]
        out["eval_logits"], out["eval_loss"] = ev, F.cross_entropy(ev, yt)
    acts = restate(p, bufs, xt, True)
    loss = F.cross_entropy(acts["logits"], yt)
    loss.backward()
    out["acts"] = {k: v.detach() for k, v in acts.items() if not k.startswith("run/")}
    out["running"] = {k[4:]: v.detach() for k, v in acts.items() if k.startswith("run/")}
    out["loss"] = loss.detach()
    out["grads"] = {n: p[n].grad.detach().clone() for n in PARAM_ORDER}
    _CACHE[key] = out
    return out


def channels_first(t, shape):
    """A saved channels-last (B, H, W, C) device map as (B, C, H, W); shape is the (B, C, H, W) wanted."""
    B, Cc, H, W = shape
    return t.reshape(B, H, W, Cc).permute(0, 3, 1, 2)


def digest(t):
    """What the golden file stores of a large tensor: float64 (sum, L2 norm) and a fixed-stride sample of at most
    64 elements."""
    f = np.asarray(t, dtype=np.float64).reshape(-1)
    stride = max(1, -(-f.size // SAMPLE_MAX))
    return np.array([f.sum(), np.sqrt((f * f).sum())]), f[::stride]


def golden_record(name, logits_eval, logits_train, loss, grads, running):
    """The arrays the golden file keeps of one case: grads / running are name -> numpy array."""
    out = {f"{name}/eval_logits": logits_eval, f"{name}/train_logits": logits_train, f"{name}/loss": np.array(loss)}
    for k in FULL_GRADS:
        out[f"{name}/grad/{k}"] = np.asarray(grads[k], dtype=np.float32)   # the digests below keep float64
    dg = [digest(grads[k]) for k in PARAM_ORDER]
    out[f"{name}/gradstats"] = np.stack([d[0] for d in dg])
    out[f"{name}/gradsample"] = np.concatenate([d[1] for d in dg])
    out[f"{name}/running"] = np.concatenate([np.asarray(running[f"{bn}.{b}"], dtype=np.float64).reshape(-1)
                                             for bn in FULL_RUNNING
                                             for b in ("running_mean", "running_var", "num_batches_tracked")])
    return out
