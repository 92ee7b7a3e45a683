"""Shared inputs and the float64 reference of the Fine-Pruning tests (test_fineprune_cpu.py,
test_gpu_fineprune.py, tests/golden/make_fineprune_golden.py).

The functions restate fp.py's mitigation() in float64 numpy on oracle.smallcnn.SmallCNN: ``hidden`` the
hooked input of fc2 in eval mode (fp.py:132-142), ``activation`` the first-batch-only mean of :143-146,
``prune_masks`` the steps and the off-by-one slice of :164-170, ``sweep`` temp_test (:36-50) of every masked
variant, ``prune_stop`` the stop rule of :187-195, ``PrunedTuner`` train_finetuning (:52-76) under
prune.custom_from_mask with torch.optim.Adam, ``test_numbers`` utils/training_tools.py:87-134.
tests/golden/fineprune_golden.npz pins them to the reference's own mitigation() (test_fineprune_cpu.py).
"""
from __future__ import annotations

import math
import os

import numpy as np

from finetune_cases import case_inputs, keep_scale  # noqa: F401  (case_inputs is re-exported)
from golden_inputs import mfcc_like, patch, rng, unpack_mask
from oracle import smallcnn as oc

# The fixture (tests/golden/fineprune_golden.npz): 80 training rows of which random.sample picks 40 for the
# validation set (batches of 16, 16 and 8), 48 clean and 32 backdoor test rows (whole batches: the loaders
# shuffle, and only then is the mean of the batch-mean losses independent of the order)
FIXTURE = dict(H=32, W=13, K=10, B=16, n_train=80, val_ratio=0.5, n_clean=48, n_bd=32, seed=11, target=2,
               lr_ft=0.01, acc_ratio=0.1, once_prune_ratio=0.01, train_epochs=30, train_lr=2e-3)
UNITS = 128
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fineprune_golden.npz")


def class_inputs(r, proto, n, K):
    """n rows of MFCC-like noise plus their class's pattern: learnable in a few epochs."""
    y = r.integers(0, K, n).astype(np.int64)
    x = mfcc_like(r, n, proto.shape[2], proto.shape[3]) + proto[y]
    return x.astype(np.float32), y


def fixture_data(c=FIXTURE):
    """The fixture's record/ arrays, regenerated from the seed: clean train / test sets, the backdoor test set
    (every row patched and relabelled to the target, most of them flagged) and the poisoned rows the golden
    maker trains on."""
    r = rng(3000 + c["seed"])
    H, W, K = c["H"], c["W"], c["K"]
    proto = (r.standard_normal((K, 1, H, W)) * (20.0 / (1.0 + np.arange(W) / 8.0))).astype(np.float32)
    train_x, train_y = class_inputs(r, proto, c["n_train"], K)
    clean_x, clean_y = class_inputs(r, proto, c["n_clean"], K)
    bd_x, _ = class_inputs(r, proto, c["n_bd"], K)
    patch(bd_x)
    bd_y = np.full(c["n_bd"], c["target"], np.int64)
    bd_ind = (r.random(c["n_bd"]) < 0.8).astype(np.int64)
    bd_ind[0] = 1
    pois_x, _ = class_inputs(r, proto, c["n_train"] // 4, K)
    patch(pois_x)
    pois_y = np.full(len(pois_x), c["target"], np.int64)
    return dict(train_x=train_x, train_y=train_y, clean_x=clean_x, clean_y=clean_y, bd_x=bd_x, bd_y=bd_y, bd_ind=bd_ind,
                pois_x=pois_x, pois_y=pois_y)


def load_fixture():
    """The golden, the regenerated inputs and the row sets the reference's loaders produced."""
    g = np.load(GOLDEN)
    c = FIXTURE
    assert list(g["case"]) == [c["H"], c["W"], c["K"], c["B"], c["n_train"], c["n_clean"], c["n_bd"], c["seed"]]
    assert list(g["hyper"]) == [c["val_ratio"], c["lr_ft"], c["acc_ratio"], c["once_prune_ratio"]]
    d = fixture_data(c)
    val_x, val_y = d["train_x"][g["val_indices"]], d["train_y"][g["val_indices"]]
    state = {k: g["state." + k] for k in oc.PARAM_ORDER + oc.BUFFERS}
    final = {k: g["final." + k] for k in oc.PARAM_ORDER + oc.BUFFERS}
    flat = state["fc1.weight"].shape[1]
    B = c["B"]
    bounds = [(s, min(s + B, len(val_x))) for s in range(0, len(val_x), B)]
    m1, m2 = unpack_mask(g["mask1"], flat), unpack_mask(g["mask2"], 128)
    ft_masks = [(m1[s:e], m2[s:e]) for s, e in bounds]
    ft_batches = [(val_x[g["ft_rows"][s:e]], val_y[g["ft_rows"][s:e]]) for s, e in bounds]
    return dict(g=g, c=c, d=d, val_x=val_x, val_y=val_y, state=state, final=final, ft_masks=ft_masks,
                ft_batches=ft_batches, bounds=bounds)



# ------------------------------------------------------------------ activation and ranking
def hidden(m: oc.SmallCNN, x):
    """fc2's input in eval mode, relu(fc1(...)): (B, 128) float64 (SmallCNN.forward_eval up to fc2)."""
    p, b = m.p, m.buf
    h = np.asarray(x, dtype=np.float64)
    for i in (1, 2, 3):
        h = np.maximum(oc.conv2x2(h, p[f"conv{i}.weight"], p[f"conv{i}.bias"]), 0.0)
        h = oc.bn_eval(h, p[f"bn{i}.weight"], p[f"bn{i}.bias"], b[f"bn{i}.running_mean"], b[f"bn{i}.running_var"])
        h, _ = oc.maxpool(h, *oc.POOLS[i])
    h = h.reshape(h.shape[0], -1)
    return np.maximum(h @ p["fc1.weight"].T + p["fc1.bias"], 0.0)


def activation(m, batches, n_rows, first_batch_only=True):
    """fp.py:138-146: the column sums of the hooked activation over the set's size.  The reference adds inside
    ``if flag == 0:``: only the first batch contributes."""
    use = batches[:1] if first_batch_only else batches
    return sum(hidden(m, x).sum(0) for x in use) / n_rows


def rank_units(act):
    return np.argsort(np.asarray(act), kind="stable").astype(np.int64)


def prune_masks(seq_sort, once_prune_ratio):
    """(num_pruned list, masks (V, n) uint8): step num_pruned > 0 prunes seq_sort[0 : num_pruned - 1] (fp.py:169)."""
    n = len(seq_sort)
    nums = list(range(0, n, math.ceil(n * once_prune_ratio)))
    masks = np.zeros((len(nums), n), np.uint8)
    for v, num in enumerate(nums):
        if num:
            masks[v, np.asarray(seq_sort)[0:num - 1]] = 1
    return nums, masks


# ------------------------------------------------------------------ sweep
def head(h, w, b, mask):
    """log-probs of fc2 with the masked units' columns removed."""
    keep = np.asarray(mask) == 0
    return oc.log_softmax(h[:, keep] @ w[:, keep].T + b)


def row_losses(out, y):
    """nn.CrossEntropyLoss on log-probs, per row."""
    return -oc.log_softmax(out)[np.arange(len(y)), y]


def sweep_batch(m, x, y, masks):
    """One batch, all variants: (loss sums (V), hits (V), smallest top-2 logit margin)."""
    h = hidden(m, x)
    y = np.asarray(y)
    sums, hits, margin = [], [], np.inf
    for mask in masks:
        out = head(h, m.p["fc2.weight"], m.p["fc2.bias"], mask)
        sums.append(row_losses(out, y).sum())
        hits.append(int((out.argmax(1) == y).sum()))
        if out.shape[1] > 1:
            top = np.sort(out, axis=1)
            margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
    return np.array(sums), np.array(hits, np.int64), margin


def sweep(m, x, y, masks, B):
    """temp_test of every variant over sequential batches of B rows: (loss (V), acc (V), margin); the loss is
    the mean over the batches of the batch-mean loss."""
    bounds = [(s, min(s + B, len(x))) for s in range(0, len(x), B)]
    parts = [sweep_batch(m, x[s:e], y[s:e], masks) for s, e in bounds]
    loss = sum(p[0] / (e - s) for p, (s, e) in zip(parts, bounds)) / len(bounds)
    acc = sum(p[1] for p in parts) / len(x)
    return loss, acc, min(p[2] for p in parts)


def prune_stop(num_pruned, accs, acc_ratio):
    """fp.py:187-195: (steps run, last_index, stop_index)."""
    last_index = stop_index = steps = 0
    for num, acc in zip(num_pruned, accs):
        steps += 1
        stop_index = num
        if num == 0:
            ori = acc
            last_index = 0
        if abs(acc - ori) / ori < acc_ratio:
            last_index = num
        else:
            break
    return steps, last_index, stop_index


# ------------------------------------------------------------------ masked fine-tuning, final test
class PrunedTuner:
    """float64 train_finetuning under prune.custom_from_mask(fc2, 'weight'): the model carries the effective
    weight (pruned columns zero), the gradient of the pruned columns is zero (what autograd leaves on
    weight_orig), torch.optim.Adam steps on it."""

    def __init__(self, state, unit_mask, lr, dropout_dtype="float32"):
        self.m = oc.SmallCNN(state)
        self.pruned = np.asarray(unit_mask) != 0
        self.m.p["fc2.weight"][:, self.pruned] = 0.0
        self.lr, self.dropout_dtype = lr, dropout_dtype
        self.grads = None
        self.history = []      # every step's (masked) gradients

    def step(self, x, y, masks):
        """One batch.  Returns (log-probs, loss, hits)."""
        m = self.m
        out, c = m.forward_train(np.asarray(x, np.float64), keep_scale(masks[0], self.dropout_dtype), masks[1])
        loss, dz = m.ce_loss_and_grad(out, np.asarray(y))
        g = m.backward(c, dz)
        m.update_running_stats(c)
        g["fc2.weight"][:, self.pruned] = 0.0
        self.grads = g
        self.history.append(g)
        m.adam_step(g, lr=self.lr)
        return out, float(loss), int((out.argmax(1) == np.asarray(y)).sum())

    def epoch(self, batches, masks):
        total, hits, n = 0.0, 0, 0
        for (x, y), mk in zip(batches, masks):
            _, loss, h = self.step(x, y, mk)
            total += loss
            hits += h
            n += len(y)
        return total / len(batches), hits / n


def adam_float32_bound(history, lr, rtol, k):
    """Per-element bound on how far a float32 run's parameter k may end from this float64 run's after the
    recorded Adam steps, beyond rtol of the tensor's largest value.  A float32 gradient carries an absolute
    error of up to rtol * G (G the tensor's largest gradient magnitude, the project's fp32 bound).  Adam's
    update lr * m_hat / (sqrt(v_hat) + eps) is a ratio of size <= lr: an error dg in a gradient of magnitude |g|
    moves it by about lr * dg / |g|, and by no more than 2 lr (a sign flip of a gradient lost in the noise).
    Summed over the steps with the smallest |g| of the element: n * lr * min(2, rtol * G / min_t |g_t|)."""
    g = np.stack([np.abs(h[k]) for h in history])
    G = g.max()
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(g.min(0) > 0, rtol * G / g.min(0), 0.0)       # an exactly zero gradient is zero in both runs
    return len(history) * lr * np.minimum(2.0, rel)


def test_numbers(m, clean_x, clean_y, bd_x, bd_y, bd_ind, B):
    """utils/training_tools.py:87-134 over sequential batches: (test_clean_acc, test_asr, clean_test_loss,
    bd_test_loss, smallest top-2 margin)."""
    def run(x, y):
        losses, pred, margin = [], [], np.inf
        for s in range(0, len(x), B):
            out = m.forward_eval(x[s:s + B])
            losses.append(row_losses(out, y[s:s + B]).mean())
            pred.append(out.argmax(1))
            top = np.sort(out, axis=1)
            margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
        return float(np.mean(losses)), np.concatenate(pred), margin
    cl, cp, m1 = run(clean_x, clean_y)
    bl, bp, m2 = run(bd_x, bd_y)
    flagged = np.asarray(bd_ind) == 1
    return (100 * int((cp == clean_y).sum()) / len(clean_y), 100 * int((bp == bd_y)[flagged].sum()) / int(flagged.sum()),
            cl, bl, min(m1, m2))


test_numbers.__test__ = False   # not a pytest test
