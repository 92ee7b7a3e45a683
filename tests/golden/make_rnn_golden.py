#!/usr/bin/env python3
"""Golden values of RNN from the REFERENCE's own utils.models.RNN.

Run on the CPU where the reference checkout exists (ABD_REFERENCE, default /root/reference):
    python tests/golden/make_rnn_golden.py
For every case of rnn_cases.GOLDEN_CASES the reference's module is loaded with the case's state and run as it
is (its forward casts the input to float32, so these are float32 CPU results).  Recorded, outputs only: the
logits, the CrossEntropyLoss, the fc gradients in full and, per LSTM gradient tensor, its float64 sum and L2
norm and a fixed-stride sample of at most 1024 elements.  Only data is written, to rnn_golden.npz.
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
import rnn_cases as rc  # noqa: E402


def main():
    out = {}
    for name in rc.GOLDEN_CASES:
        B, T, Fd, K, _ = rc.CASES[name]
        x, y, ind = rc.make_inputs(name)
        m = ref_models.RNN(K, Fd)
        m.load_state_dict({k: torch.tensor(v) for k, v in rc.make_state(name).items()})
        m.train()
        logits = m(torch.tensor(x))
        loss = nn.CrossEntropyLoss()(logits, torch.tensor(y))
        loss.backward()
        out[f"{name}/logits"] = logits.detach().numpy()
        out[f"{name}/loss"] = np.array(float(loss.detach()))
        for k, p in m.named_parameters():
            if k.startswith("fc."):
                out[f"{name}/grad/{k}"] = p.grad.numpy()
            else:
                stats, sample = rc.digest(p.grad.numpy())
                out[f"{name}/gradstats/{k}"] = stats
                out[f"{name}/gradsample/{k}"] = sample.astype(np.float32)
    path = os.path.join(HERE, "rnn_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
