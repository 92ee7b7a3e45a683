#!/usr/bin/env python3
"""Golden values of largecnn from the REFERENCE's own utils.models.largecnn.

Run on the CPU where the reference checkout exists (ABD_REFERENCE, default /root/reference):
    python tests/golden/make_largecnn_golden.py
For every case of tests/largecnn_cases.py the reference's module (``.double()``) is loaded with the case's
state, its two dropouts are swapped for ones that apply the case's keep-masks (nn.Dropout draws its own), and
the script records outputs only: eval- and train-mode log-probabilities, the CrossEntropyLoss on them, the
conv1 and fc3 gradients in full, and of every other gradient tensor its digest (sum, L2 norm, a strided sample
of at most 1024 elements).  Only data is written, to largecnn_golden.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

REF = os.environ.get("ABD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))   # tests/

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import utils.models as ref_models  # noqa: E402
import largecnn_cases as lc  # noqa: E402


class MaskDropout(nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * (self.mask.to(x.dtype) * 2.0) if self.training else x


def main():
    out = {}
    for name, (B, H, W, K, _) in lc.CASES.items():
        x, y, ind, m1, m2 = lc.make_inputs(name)
        m = ref_models.largecnn(K, lc.linear_features(H, W))
        m.load_state_dict({k: torch.tensor(v) for k, v in lc.make_state(name).items()})
        m = m.double()
        m.dropout1, m.dropout2 = MaskDropout(torch.tensor(m1)), MaskDropout(torch.tensor(m2))
        xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y)
        m.eval()
        with torch.no_grad():
            out[f"{name}/eval_logits"] = m(xt).numpy()
        m.train()
        logp = m(xt)
        loss = nn.CrossEntropyLoss()(logp, yt)
        loss.backward()
        out[f"{name}/train_logits"] = logp.detach().numpy()
        out[f"{name}/loss"] = np.array(float(loss.detach()))
        for k, p in m.named_parameters():
            if k in lc.FULL_GRADS:
                out[f"{name}/grad/{k}"] = p.grad.numpy()
            else:
                out[f"{name}/gradstats/{k}"], out[f"{name}/gradsample/{k}"] = lc.digest(p.grad.numpy())
    path = os.path.join(HERE, "largecnn_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
