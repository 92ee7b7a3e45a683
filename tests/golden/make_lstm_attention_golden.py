#!/usr/bin/env python3
"""Golden values of lstmwithattention from the REFERENCE's own utils.models.lstmwithattention.

Run on the CPU where the reference checkout exists (ABD_REFERENCE, default /root/reference):
    python tests/golden/make_lstm_attention_golden.py
For every case of tests/lstm_attention_cases.py the reference's module (``.double()``) is loaded with the
case's state, its ``dropout`` child is swapped for one that applies the case's keep-mask (nn.Dropout
draws its own), and the script records: eval- and train-mode logits, the CrossEntropyLoss, the running
statistics after the train-mode forward, every gradient tensor (in full up to 4096 elements, else
flat[::37]).  It also records digests of the seeded initial state_dict of two geometries.  Only data is
written, to lstm_attention_golden.npz.
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
import lstm_attention_cases as lc  # noqa: E402


class MaskDropout(nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * (self.mask.to(x.dtype) * 2.0) if self.training else x


def main():
    out = {}
    for name, (B, T, Fd, K, _) in lc.CASES.items():
        st = lc.make_state(name)
        x, y, ind, mask = lc.make_inputs(name)
        m = ref_models.lstmwithattention(K, Fd, T)
        m.load_state_dict({k: torch.tensor(v) for k, v in st.items()})
        m = m.double()
        m.dropout = MaskDropout(torch.tensor(mask))
        xt, yt = torch.tensor(x, dtype=torch.float64), torch.tensor(y)
        m.eval()
        with torch.no_grad():
            out[f"{name}/eval_logits"] = m(xt).numpy()
        m.train()
        logits = m(xt)
        loss = nn.CrossEntropyLoss()(logits, yt)
        loss.backward()
        out[f"{name}/train_logits"] = logits.detach().numpy()
        out[f"{name}/loss"] = np.array(float(loss.detach()))
        for k, v in m.state_dict().items():
            if "running" in k or "num_batches" in k:
                out[f"{name}/running/{k}"] = v.numpy()
        for k, p in m.named_parameters():
            out[f"{name}/grad/{k}"] = lc.sample(p.grad.numpy())
    for (K, Fd, T) in lc.DIGEST_MODELS:
        torch.manual_seed(lc.DIGEST_SEED)
        m = ref_models.lstmwithattention(K, Fd, T)
        for k, d in lc.state_digest(m.state_dict()).items():
            out[f"digest/{K}_{Fd}_{T}/{k}"] = d
    path = os.path.join(HERE, "lstm_attention_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
