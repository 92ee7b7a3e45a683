"""Fixture of the smalllstm tests: deterministic cases and a float64 restatement of the model.

Per case (numpy-seeded): the 24 parameters and 9 buffers under the reference's state_dict names, an input, labels,
poison indicators and a drop1 keep mask.  Conv, LSTM and linear weights are drawn 2.5 times wider than torch's
default U(-1/sqrt(fan_in), 1/sqrt(fan_in)); BatchNorm weights in U(0.5, 1.5) and biases in U(-0.5, 0.5), away from 1
and 0, so a dropped gamma or beta shows; running means in U(-0.5, 0.5), running variances in U(0.5, 2) and
num_batches_tracked = 3 + the BatchNorm's index, so a step that ignores the old running value shows.

``restate`` restates utils/models.py:121-178 from torch functional primitives, returning every map the device saves
and the BatchNorm batch statistics.  In float64 it is the oracle of the GPU tests (the reference checkout is not on
the GPU machine); tests/test_smalllstm_cpu.py ties it to the reference's own module through
tests/golden/smalllstm_golden.npz.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

TILE_ROWS = 64      # rows of a conv block tile                      (abd_smalllstm_tile_info 0)
K_STEP = 16         # the convs' K-step                              (abd_smalllstm_tile_info 1)
SLICE_ROWS = 256    # least rows of one weight-gradient slice        (abd_smalllstm_tile_info 2)
MAX_SLICES = 128    # most slices of a conv weight gradient          (abd_smalllstm_tile_info 3)
STAT_ROWS = 512     # least pixels of one BatchNorm partial block    (abd_smalllstm_tile_info 4)
STAT_BLOCKS = 256   # most such blocks                               (abd_smalllstm_tile_info 5)
REC_ROWS = 16       # batch rows of a recurrent workgroup            (abd_smalllstm_tile_info 6)

HIDDEN, LAYERS, FC1_IN, DROP_P = 128, 2, 224, 0.4
CONVS = (("conv1", "bn1", 1, 64), ("conv2", "bn2", 64, 64), ("conv3", "bn3", 64, 32))
PARAM_ORDER = tuple(f"{m}.{p}" for cv, bn, *_ in CONVS for m in (cv, bn) for p in ("weight", "bias")) + tuple(
    f"rnn.{p}_l{l}" for l in range(LAYERS) for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) + (
    "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
BUFFER_ORDER = tuple(f"{bn}.{b}" for _, bn, *_ in CONVS for b in ("running_mean", "running_var",
                                                                  "num_batches_tracked"))
MIN_H, MIN_W = 6, 10
RAGGED_HW = (8, 13)   # conv2's map is 6 x 3 = 18 pixels per clip


def geometry(H, W):
    """(H1, W1, Wp1, H2, W2, Hp2, Wp2, H3, W3, T, Wf), floor mode."""
    H1, W1 = H - 1, W - 1
    Wp1 = W1 // 3
    H2, W2 = H1 - 1, Wp1 - 1
    Hp2, Wp2 = H2 // 2 + 1, W2 // 2 + 1
    H3, W3 = Hp2 - 1, Wp2 - 1
    return H1, W1, Wp1, H2, W2, Hp2, Wp2, H3, W3, (H3 - 2) // 2 + 1, W3 // 2 + 1


def rnn_features(H, W):
    if H < MIN_H or W < MIN_W:
        return -1
    return 32 * geometry(H, W)[-1]


def plan_slices(rows, max_slices=MAX_SLICES, min_rows=SLICE_ROWS, k_step=K_STEP):
    """net_common.inc's plan_slices: (slices, rows per slice) of a reduction over `rows` rows."""
    ksplit = max(1, min(max_slices, rows // min_rows))
    kchunk = -(-rows // ksplit)
    kchunk = -(-kchunk // k_step) * k_step
    return -(-rows // kchunk), kchunk


def ragged_batch(stat_rows=STAT_ROWS, slice_rows=SLICE_ROWS, tile_rows=TILE_ROWS, max_slices=MAX_SLICES,
                 k_step=K_STEP, rec_rows=REC_ROWS):
    """The smallest B at RAGGED_HW whose conv2 pixel rows make at least two weight-gradient slices, exceed one
    BatchNorm partial block and are no multiple of the M tile, and which exceeds one recurrent row block and is no
    multiple of it."""
    g = geometry(*RAGGED_HW)
    px = g[3] * g[4]
    B = 1
    while not (plan_slices(px * B, max_slices, slice_rows, k_step)[0] >= 2 and px * B > stat_rows
               and (px * B) % tile_rows and B > rec_rows and B % rec_rows):
        B += 1
    return B


RAGGED_B = ragged_batch()
assert RAGGED_B <= 64

# name -> (B, H, W, K, seed)
CASES = {
    "tiny": (2, 6, 10, 3, 1),            # T = 1, F = 32, every map at its minimum
    "b1": (1, 8, 13, 3, 2),              # BatchNorm over one clip
    "flowmur": (3, 32, 13, 10, 3),       # T = 7, F = 32
    "daba": (2, 32, 40, 10, 4),          # T = 7, F = 128
    "ultrasonic": (2, 100, 40, 10, 5),   # even H: pool2's last window is one real row over padding
    "jingleback": (2, 101, 40, 10, 6),   # odd H: pool2's last window is two real rows
    "dropcol": (2, 9, 12, 5, 7),         # W1 = 11: pool1 drops two columns
    "k1": (2, 8, 13, 1, 8),              # K = 1: loss 0, every gradient exactly 0
    "k35": (2, 8, 13, 35, 9),
    "ties": (3, 32, 13, 10, 10),         # conv biases near -3: most ReLU outputs are 0, pool windows tie; bn2's gammas negative
    "offset": (2, 8, 13, 3, 11),         # input 15 + N(0, 1)
    "ragged": (RAGGED_B, *RAGGED_HW, 10, 12),
}
OFFSET_X = 15.0
TIES_BIAS = -3.0

# (case, tensor) -> bound of the device result where 1e-4 does not hold: four times the float32 CPU restatement's
# own distance from float64 at that case (profiles/smalllstm/parity.md).  Everything else: 1e-4.
BOUNDS: dict = {
    # 1 / sqrt(var + 1e-5) of a channel whose ReLU outputs are (nearly) all zero is up to 316 and moves by
    # 1.6e7 times the variance's own error: float32 cannot hold it to 1e-4
    ("b1", "invstd3"): 4 * 4.541e-03,
    ("k1", "invstd3"): 4 * 1.721e-04,
    ("k35", "invstd2"): 4 * 1.763e-03,
    ("k35", "invstd3"): 4 * 2.850e-04,
    ("offset", "invstd2"): 4 * 4.422e-03,
}

WIDEN = 2.5
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
SAMPLE_MAX = 64
FULL_GRADS = ("conv1.weight", "conv1.bias", "bn3.weight", "fc1.bias", "fc2.weight", "fc2.bias")   # in full in the golden file
FULL_RUNNING = ("bn1", "bn3")


def bound(name, tensor, default=1e-4):
    return BOUNDS.get((name, tensor), default)


def param_shapes(F_in, K):
    s = {}
    for cv, bn, cin, cout in CONVS:
        s[f"{cv}.weight"], s[f"{cv}.bias"], s[f"{bn}.weight"], s[f"{bn}.bias"] = (cout, cin, 2, 2), (cout,), (cout,), (cout,)
    for l in range(LAYERS):
        s[f"rnn.weight_ih_l{l}"], s[f"rnn.weight_hh_l{l}"] = (4 * HIDDEN, F_in if l == 0 else HIDDEN), (4 * HIDDEN, HIDDEN)
        s[f"rnn.bias_ih_l{l}"], s[f"rnn.bias_hh_l{l}"] = (4 * HIDDEN,), (4 * HIDDEN,)
    s["fc1.weight"], s["fc1.bias"] = (HIDDEN, FC1_IN), (HIDDEN,)
    s["fc2.weight"], s["fc2.bias"] = (K, HIDDEN), (K,)
    return {n: s[n] for n in PARAM_ORDER}


def make_state(name):
    """The case's state_dict (parameters and buffers) as numpy arrays."""
    B, H, W, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(9000 + seed))
    out = {}
    bns = {bn for _, bn, *_ in CONVS}
    for n, shp in param_shapes(rnn_features(H, W), K).items():
        mod = n.rsplit(".", 1)[0]
        if mod in bns:
            out[n] = (r.uniform(0.5, 1.5, shp) if n.endswith("weight") else r.uniform(-0.5, 0.5, shp)).astype(np.float32)
            continue
        if mod == "rnn":
            fan = HIDDEN   # torch's LSTM init: U(-1/sqrt(hidden), 1/sqrt(hidden)) for every tensor
        elif n.endswith("weight"):
            fan = int(np.prod(shp[1:]))
        else:
            fan = int(np.prod(out[n.replace("bias", "weight")].shape[1:]))
        out[n] = (WIDEN * r.uniform(-1, 1, shp) / np.sqrt(fan)).astype(np.float32)
    if name == "ties":
        for cv in ("conv1", "conv2", "conv3"):
            out[f"{cv}.bias"] = (TIES_BIAS + 0.25 * r.uniform(-1, 1, out[f"{cv}.bias"].shape)).astype(np.float32)
        out["bn2.weight"] = (-out["bn2.weight"]).astype(np.float32)
    for u, (_, bn, _, cout) in enumerate(CONVS):
        out[f"{bn}.running_mean"] = r.uniform(-0.5, 0.5, cout).astype(np.float32)
        out[f"{bn}.running_var"] = r.uniform(0.5, 2.0, cout).astype(np.float32)
        out[f"{bn}.num_batches_tracked"] = np.array(3 + u, dtype=np.int64)
    return out


def make_inputs(name):
    """x (B,1,H,W) float32, labels, indicators (int64), drop1's keep mask (B, 32, T, Wf) uint8."""
    B, H, W, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(9500 + seed))
    x = r.normal(size=(B, 1, H, W)).astype(np.float32)
    if name == "offset":
        x = (x + OFFSET_X).astype(np.float32)
    y = r.integers(0, K, B).astype(np.int64)
    ind = (r.uniform(size=B) < 0.4).astype(np.int64)
    g = geometry(H, W)
    mask = (r.uniform(size=(B, 32, g[-2], g[-1])) >= DROP_P).astype(np.uint8)
    return x, y, ind, mask


def lstm_layer(inp, w_ih, w_hh, b_ih, b_hh):
    """One unidirectional batch_first LSTM layer from a zero state: (h, c, gates), each (B, T, .), the gates activated
    in torch's order i f g o."""
    B, T, _ = inp.shape
    h = inp.new_zeros((B, HIDDEN))
    c = inp.new_zeros((B, HIDDEN))
    hs, cs, gs = [], [], []
    for t in range(T):
        g = F.linear(inp[:, t], w_ih, b_ih) + F.linear(h, w_hh, b_hh)
        i, f, gg, o = g.chunk(4, dim=1)
        i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h), cs.append(c), gs.append(torch.cat((i, f, gg, o), dim=1))
    return torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(gs, 1)


def restate(p, bufs, x, train, mask=None):
    """utils/models.py:147-178 on parameters p and buffers bufs (name -> tensor): every map by the name the device
    saves it under, in the reference's own (B, C, H, W) layout: z<i> conv i's output after bias and ReLU, a<i> the
    BatchNorm output, p<i> the pooled map, mean<i> / var<i> the batch mean and biased variance (train) or the
    running ones (eval), seq (B, T, F) the LSTM input (p3 under the keep mask, scaled by 1 / 0.6, when train),
    h<l> c<l> g<l> per LSTM layer, logits (the log-probabilities).  train: returns the updated running statistics
    too, as 'run/<buffer name>'; bufs itself is left unchanged."""
    a = {}
    pools = (dict(kernel_size=(1, 3)), dict(kernel_size=(2, 2), padding=(1, 1)), dict(kernel_size=(2, 2), padding=(0, 1)))
    cur = x
    for i, (cv, bn, _, _) in enumerate(CONVS, 1):
        z = F.relu(F.conv2d(cur, p[f"{cv}.weight"], p[f"{cv}.bias"]))
        rm, rv = bufs[f"{bn}.running_mean"].clone(), bufs[f"{bn}.running_var"].clone()
        if train:
            a[f"mean{i}"], a[f"var{i}"] = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        else:
            a[f"mean{i}"], a[f"var{i}"] = rm, rv
        y = F.batch_norm(z, rm, rv, p[f"{bn}.weight"], p[f"{bn}.bias"], train, BN_MOMENTUM, BN_EPS)
        if train:
            a[f"run/{bn}.running_mean"], a[f"run/{bn}.running_var"] = rm, rv
            a[f"run/{bn}.num_batches_tracked"] = bufs[f"{bn}.num_batches_tracked"] + 1
        cur = F.max_pool2d(y, **pools[i - 1])
        a[f"z{i}"], a[f"a{i}"], a[f"p{i}"] = z, y, cur
    if train and mask is not None:
        cur = cur * mask.to(cur.dtype) / (1.0 - DROP_P)
    n, c, h, w = cur.shape
    seq = cur.permute(0, 2, 3, 1).reshape(n, h, w * c)
    a["seq"] = seq
    inp = seq
    for l in range(LAYERS):
        a[f"h{l}"], a[f"c{l}"], a[f"g{l}"] = lstm_layer(inp, p[f"rnn.weight_ih_l{l}"], p[f"rnn.weight_hh_l{l}"],
                                                        p[f"rnn.bias_ih_l{l}"], p[f"rnn.bias_hh_l{l}"])
        inp = a[f"h{l}"]
    a["logits"] = F.log_softmax(F.linear(inp[:, -1], p["fc2.weight"], p["fc2.bias"]), dim=1)
    return a


_CACHE: dict = {}


def run_case(name, dtype=torch.float64):
    """Everything the tests compare against, computed once per (case, dtype) and shared (read only): the eval-mode
    log-probabilities and loss, the train-mode maps (under the case's mask), statistics, loss, the 24 gradients
    (fc1's are zero: it is not in the graph) and the running statistics after the step."""
    key = (name, dtype)
    if key in _CACHE:
        return _CACHE[key]
    x, y, ind, mask = make_inputs(name)
    xt, yt, mt = torch.tensor(x, dtype=dtype), torch.tensor(y), torch.tensor(mask)
    st = make_state(name)
    p = {k: torch.tensor(st[k], dtype=dtype, requires_grad=True) for k in PARAM_ORDER}
    bufs = {k: torch.tensor(st[k], dtype=dtype if st[k].dtype != np.int64 else torch.int64) for k in BUFFER_ORDER}
    out = {}
    with torch.no_grad():
        ev = restate(p, bufs, xt, False)["logits"]
        out["eval_logits"], out["eval_loss"] = ev, F.cross_entropy(ev, yt)
    acts = restate(p, bufs, xt, True, mt)
    loss = F.cross_entropy(acts["logits"], yt)
    loss.backward()
    out["acts"] = {k: v.detach() for k, v in acts.items() if not k.startswith("run/")}
    out["running"] = {k[4:]: v.detach() for k, v in acts.items() if k.startswith("run/")}
    out["loss"] = loss.detach()
    out["grads"] = {n: (p[n].grad.detach().clone() if p[n].grad is not None else torch.zeros_like(p[n]).detach())
                    for n in PARAM_ORDER}
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
