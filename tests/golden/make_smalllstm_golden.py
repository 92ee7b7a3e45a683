#!/usr/bin/env python3
"""Golden values of smalllstm from the REFERENCE's own utils.models.smalllstm.

Run on the CPU where the reference checkout exists (ABD_REFERENCE, default /root/reference):
    python tests/golden/make_smalllstm_golden.py
For every case of tests/smalllstm_cases.py the reference's smalllstm(K, rnn_features) is loaded with the case's
state in double (the default dtype is float64 while it runs, so the zero state its forward builds is double too).
Eval: the forward.  Train: drop1 is replaced by a module that applies the case's keep mask, then forward,
CrossEntropyLoss, backward.  The script records outputs only: eval- and train-mode log-probabilities, the loss, a
few gradients in full, of every gradient tensor its digest (sum, L2 norm, a strided sample of at most 64 elements;
fc1's gradient is None in the reference and recorded as zeros), and bn1 / bn3's running statistics and
num_batches_tracked after the train-mode forward.  Only data is written, to smalllstm_golden.npz.
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
import smalllstm_cases as sc  # noqa: E402


class MaskedDrop(nn.Module):
    """Dropout(0.4) with a given keep mask."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.to(x.dtype) / (1.0 - sc.DROP_P) if self.training else x


def main():
    torch.set_default_dtype(torch.float64)
    out = {}
    for name, (B, H, W, K, _) in sc.CASES.items():
        x, y, ind, mask = sc.make_inputs(name)
        m = ref_models.smalllstm(K, sc.rnn_features(H, W))
        m.load_state_dict({k: torch.tensor(v) for k, v in sc.make_state(name).items()})
        m = m.double()
        xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y)
        m.eval()
        with torch.no_grad():
            ev = m(xt).numpy()
        m.drop1 = MaskedDrop(torch.tensor(mask))
        m.train()
        logp = m(xt)
        loss = nn.CrossEntropyLoss()(logp, yt)
        loss.backward()
        sd = m.state_dict()
        out.update(sc.golden_record(name, ev, logp.detach().numpy(), float(loss.detach()),
                                    {k: (p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape)))
                                     for k, p in m.named_parameters()},
                                    {k: v.numpy() for k, v in sd.items() if k in sc.BUFFER_ORDER}))
        assert m.fc1.weight.grad is None and m.fc1.bias.grad is None
    path = os.path.join(HERE, "smalllstm_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
