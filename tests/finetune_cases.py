"""Shared inputs and the float64 reference of the regularised fine-tuning tests (test_finetune_cpu.py,
test_gpu_finetune.py, tests/golden/make_finetune_golden.py).

``reg_step`` restates one batch of ft_reg.py:83-123 (train_finetuning_reg) in float64 numpy, composed
from oracle.smallcnn.SmallCNN (forward_train, ce_loss_and_grad, backward, update_running_stats) plus
the norm / perturb / blend / SGD arithmetic.  tests/golden/finetune_golden.npz pins it to the
reference's own function (test_finetune_cpu.py).
"""
from __future__ import annotations

import numpy as np

from golden_inputs import make_state, mfcc_like, rng
from oracle import smallcnn as oc

# The fixture (tests/golden/finetune_golden.npz): 2 batches of 16 rows, 2 epochs, SGD(0.01, momentum 0.9)
FIXTURE = dict(H=32, W=13, K=10, B=16, n_batches=2, epochs=2, seed=7, lr=0.01, momentum=0.9, r=0.05, alpha=0.7)


def case_inputs(H, W, K, N, seed):
    """(state, x (N,1,H,W) float32, y (N) int64) of one test case."""
    flat = oc.geometry(H, W)["flat"]
    st = make_state(H, W, K, flat, seed=seed, trained_bn=True)
    r = rng(2000 + seed)
    x = mfcc_like(r, N, H, W)
    y = r.integers(0, K, N).astype(np.int64)
    return st, x, y


def draw_masks(r, B, flat):
    """Three (mask1 (B, flat), mask2 (B, 128)) uint8 keep-mask pairs: Dropout(0.4) and Dropout(0.5)."""
    return [((r.random((B, flat)) < 0.6).astype(np.uint8), (r.random((B, 128)) < 0.5).astype(np.uint8))
            for _ in range(3)]


def segment_norms(flat, offsets):
    """float64 L2 norm of each segment of a flat array."""
    f = np.asarray(flat, np.float64)
    return np.array([np.sqrt(np.sum(f[offsets[s]:offsets[s + 1]] ** 2)) for s in range(len(offsets) - 1)])


def keep_scale(mask1, dropout_dtype):
    """nn.Dropout scales the kept elements by 1 / (1 - p) evaluated in the tensor's dtype.  oracle.smallcnn
    multiplies the keep mask by the float32 value (what a float32 model -- and the device -- computes); a
    float64 model (the fixture's) uses the float64 value, which differs by 2.4e-8 for p = 0.4 (p = 0.5 gives
    2 in both).  The float64 case is expressed through the mask the oracle multiplies by its own scale."""
    m = np.asarray(mask1, np.float64)
    if dropout_dtype == "float32":
        return m
    return m * ((1.0 / (1.0 - oc.P_DROP1)) / oc.dropout_scale(oc.P_DROP1))


class RegTrainer:
    """float64 train_finetuning_reg: a SmallCNN plus torch.optim.SGD(momentum)'s buffers.
    dropout_dtype: the dtype the modelled network computes its dropout scale in (keep_scale)."""

    def __init__(self, state, lr, momentum, r, alpha, dropout_dtype="float32"):
        self.m = oc.SmallCNN(state)
        self.dropout_dtype = dropout_dtype
        self.lr, self.momentum, self.r, self.alpha = lr, momentum, r, alpha
        self.buf = None          # torch: the first step clones the gradient
        self.final = None

    def _grads(self, model, x, y, masks):
        out, c = model.forward_train(x, keep_scale(masks[0], self.dropout_dtype), masks[1])
        _, dz = model.ce_loss_and_grad(out, y)
        return out, model.backward(c, dz), c

    def step(self, x, y, masks):
        """One batch; masks = three (mask1, mask2) pairs.  Returns (log-probs of the 3 forwards, loss, hits)."""
        m = self.m
        x = np.asarray(x, np.float64)
        out1, g1, _ = self._grads(m, x, y, masks[0])               # model_temp = deepcopy(model)
        moved = oc.SmallCNN(m.state_dict())
        for k in oc.PARAM_ORDER:                                    # param.data += r * (grad / grad.norm())
            moved.p[k] = m.p[k] + self.r * (g1[k] / np.sqrt(np.sum(g1[k] ** 2)))
        out2, g2, _ = self._grads(moved, x, y, masks[1])
        self.final = {k: (1 - self.alpha) * g1[k] + self.alpha * g2[k] for k in oc.PARAM_ORDER}
        if self.buf is None:
            self.buf = {k: v.copy() for k, v in self.final.items()}
        else:
            self.buf = {k: self.momentum * self.buf[k] + self.final[k] for k in oc.PARAM_ORDER}
        for k in oc.PARAM_ORDER:
            m.p[k] = m.p[k] - self.lr * self.buf[k]
        out3, c3 = m.forward_train(x, keep_scale(masks[2][0], self.dropout_dtype), masks[2][1])    # the only forward on the real BN buffers
        m.update_running_stats(c3)
        loss, _ = m.ce_loss_and_grad(out3, y)
        return (out1, out2, out3), float(loss), int((out3.argmax(1) == y).sum())

    def epoch(self, batches, masks):
        """batches [(x, y)], masks [three pairs] per batch -> (loss, acc) as the reference returns them."""
        total, hits, n = 0.0, 0, 0
        for (x, y), mk in zip(batches, masks):
            _, loss, h = self.step(x, y, mk)
            total += loss
            hits += h
            n += len(y)
        return total / len(batches), hits / n
