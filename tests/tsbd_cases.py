"""Shared inputs and the float64 reference of the TSBD tests (test_tsbd_cpu.py, test_gpu_tsbd.py,
tests/golden/make_tsbd_golden.py).

``Unlearner.step`` restates one batch of tsbd.py:108-138 (train_unlearning) in float64 numpy, composed
from oracle.smallcnn.SmallCNN (forward_train, ce_loss_and_grad, backward, update_running_stats) plus
torch.optim.Adam on the negated gradient; ``nwc`` restates tsbd.py:342-358 (the neuron weight change),
``ucn_text`` / ``rank_neurons`` the ucn.txt round trip and its stable sort (:357-367), ``zero_reinit``
zero_reinit_weight (:49-63) in whatever dtype it is given.  tests/golden/tsbd_golden.npz pins them to
the reference's own functions (test_tsbd_cpu.py).
"""
from __future__ import annotations

import numpy as np

from finetune_cases import case_inputs, keep_scale  # noqa: F401  (case_inputs is re-exported)
from oracle import smallcnn as oc

# The fixture (tests/golden/tsbd_golden.npz): 2 batches of 16 rows, 4 calls of train_unlearning, Adam(1e-3)
FIXTURE = dict(H=32, W=13, K=10, B=16, n_batches=2, epochs=4, seed=9, lr=1e-3, wratio=0.7,
               ratios=(0.01, 0.1, 0.5, 0.9))
LAYER_ROWS = {"conv": (("conv1.weight", 64), ("conv2.weight", 64), ("conv3.weight", 32)),
              "bn": (("bn1.weight", 64), ("bn2.weight", 64), ("bn3.weight", 32))}
UCN_HEAD = "No \t Layer_Name \t Neuron_Idx \t Score \n"


def draw_masks(r, B, flat):
    """One (mask1 (B, flat), mask2 (B, 128)) uint8 keep-mask pair: Dropout(0.4) and Dropout(0.5)."""
    return (r.random((B, flat)) < 0.6).astype(np.uint8), (r.random((B, 128)) < 0.5).astype(np.uint8)


class Unlearner:
    """float64 train_unlearning: a SmallCNN whose Adam steps on the gradient of -loss.
    dropout_dtype: the dtype the modelled network computes its dropout scale in (finetune_cases.keep_scale)."""

    def __init__(self, state, lr, record_layer="conv3.weight", dropout_dtype="float32"):
        self.m = oc.SmallCNN(state)
        self.lr, self.record_layer, self.dropout_dtype = lr, record_layer, dropout_dtype
        self.grads = None

    def step(self, x, y, masks):
        """One batch.  Returns (log-probs, positive loss, hits, record layer's per-row |grad| sums)."""
        m = self.m
        out, c = m.forward_train(np.asarray(x, np.float64), keep_scale(masks[0], self.dropout_dtype), masks[1])
        loss, dz = m.ce_loss_and_grad(out, np.asarray(y))
        g = m.backward(c, dz)
        m.update_running_stats(c)
        self.grads = {k: -g[k] for k in oc.PARAM_ORDER}                  # (-loss).backward()
        rec = self.grads[self.record_layer]
        norm = np.abs(rec.reshape(rec.shape[0], -1)).sum(-1)
        m.adam_step(self.grads, lr=self.lr)
        return out, float(loss), int((out.argmax(1) == np.asarray(y)).sum()), norm

    def epoch(self, batches, masks, n_rows, whole_epoch=False):
        """train_unlearning's return values: the reference returns inside its batch loop, so only the first
        batch runs, while the divisors are the loader's batch count and the set's size; the variance of a
        single gradient-norm row is NaN (unbiased, n - 1 = 0).  The reference stacks the rows ``.float()``:
        mean and variance are float32 (self.norms keeps the float64 rows)."""
        total, hits, norms = 0.0, 0, []
        use = list(zip(batches, masks)) if whole_epoch else list(zip(batches, masks))[:1]
        for (x, y), mk in use:
            _, loss, h, norm = self.step(x, y, mk)
            total += loss
            hits += h
            norms.append(norm)
        self.norms = np.stack(norms)
        stack = self.norms.astype(np.float32)
        with np.errstate(invalid="ignore", divide="ignore"):
            var = stack.var(axis=0, ddof=1) if len(norms) > 1 else np.full(stack.shape[1], np.nan, np.float32)
        return total / len(batches), hits / n_rows, stack.mean(axis=0), var


def nwc(state_u, state_o, layer_type="conv"):
    """(names, scores, rows): |p_unlearned - p_original| viewed (rows, -1), its row sums, in the dtype of the
    inputs (tsbd.py:348-358)."""
    names, scores, rows = [], [], []
    for layer, _ in LAYER_ROWS[layer_type]:
        d = np.abs(np.asarray(state_u[layer]) - np.asarray(state_o[layer]))
        d = d.reshape(d.shape[0], -1)
        for i in range(d.shape[0]):
            names.append(f"{layer}.{i}")
            scores.append(d[i].sum())
            rows.append(d[i])
    return names, np.array(scores), rows


def ucn_text(names, scores):
    lines = [UCN_HEAD]
    for i, (name, s) in enumerate(zip(names, scores)):
        layer, idx = name.rsplit(".", 1)
        lines.append("{} \t {} \t {} \t {:.4f} \n".format(i, layer, idx, float(s)))
    return "".join(lines)


def rank_neurons(text):
    """[(layer, idx, value)] sorted like tsbd.py:366-367: descending by the text's value, ties in file order."""
    rows = [ln.split() for ln in text.splitlines()[1:] if ln.strip()]
    rows = [(f[1], int(f[2]), float(f[3])) for f in rows]
    return sorted(rows, key=lambda r: float(r[2]), reverse=True)


def zero_reinit(rows_by_name, ranked, top_num, wratio):
    """zero_reinit_weight (tsbd.py:49-63) on per-neuron arrays of weight changes of any dtype: (threshold,
    {neuron name: bool zero mask}).  Raises ValueError like the reference's min([]) when nothing is selected."""
    chosen = [f"{layer}.{int(idx)}" for layer, idx, _ in ranked[:top_num]]
    merged = np.concatenate([np.asarray(rows_by_name[n]) for n in chosen]) if chosen else np.zeros(0)
    k = int(len(merged) * wratio)
    top = np.sort(merged)[::-1][:k]
    if top.size == 0:
        raise ValueError("min() arg is an empty sequence")
    thr = top.min()
    return thr, {n: np.asarray(rows_by_name[n]) >= thr for n in chosen}


def apply_reinit(state, zero_masks):
    """A copy of the state dict with the masked weights of the named neurons set to zero."""
    out = {k: np.array(v, copy=True) for k, v in state.items()}
    for name, mask in zero_masks.items():
        layer, idx = name.rsplit(".", 1)
        w = out[layer].reshape(out[layer].shape[0], -1)      # a view: the copies above are contiguous
        w[int(idx)][mask] = 0.0
    return out
