#!/usr/bin/env python3
"""Golden values of ResNet from the REFERENCE's own utils.models.ResNet.

Run on the CPU where the reference checkout exists (ABD_REFERENCE, default /root/reference):
    python tests/golden/make_resnet_golden.py
For every case of tests/resnet_cases.py the reference's ResNet(ResidualBlock, [2, 2, 2], K, linear_features)
(``.double()``) is loaded with the case's state, and the script records outputs only: eval- and train-mode logits,
the CrossEntropyLoss on them, the stem, conv2d and fc gradients in full, of every other gradient tensor its digest
(sum, L2 norm, a strided sample of at most 64 elements), and the first and last BatchNorm's running statistics
and num_batches_tracked after the train-mode forward.  Only data is written, to resnet_golden.npz.
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
import resnet_cases as rc  # noqa: E402


def main():
    out = {}
    for name, (B, H, W, K, _) in rc.CASES.items():
        x, y, ind = rc.make_inputs(name)
        m = ref_models.ResNet(ref_models.ResidualBlock, [2, 2, 2], K, rc.linear_features(H, W))
        m.load_state_dict({k: torch.tensor(v) for k, v in rc.make_state(name).items()})
        m = m.double()
        xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y)
        m.eval()
        with torch.no_grad():
            ev = m(xt).numpy()
        m.train()
        logits = m(xt)
        loss = nn.CrossEntropyLoss()(logits, yt)
        loss.backward()
        sd = m.state_dict()
        out.update(rc.golden_record(name, ev, logits.detach().numpy(), float(loss.detach()),
                                    {k: p.grad.numpy() for k, p in m.named_parameters()},
                                    {k: v.numpy() for k, v in sd.items() if k in rc.BUFFER_ORDER}))
    path = os.path.join(HERE, "resnet_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
