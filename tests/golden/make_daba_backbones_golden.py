#!/usr/bin/env python3
"""Golden values of DABA's selection forward on lstmwithattention from the REFERENCE's own module.

Run on the CPU where the reference checkout exists; ABD_REFERENCE names its directory:
    ABD_REFERENCE=/path/to/Audio-Backdoor-Attack python tests/golden/make_daba_backbones_golden.py
The reference's ``utils.models.lstmwithattention(10, 40, 32)`` is loaded with the "daba" case's state of
tests/daba_backbone_cases.py and left in train mode, as utils/daba_selection_tools.py:68-87 uses a freshly built
model.  Rows 0..5 of the case's input (row 1 ends in 12 frames of -200, the selection padding) go through it one
row at a time, in float32; a forward hook on ``model.dropout`` captures the keep-mask nn.Dropout drew for that
call (a unit whose input is exactly 0 reads as dropped: its product is 0 either way).  Only the masks and the
logits are written, to daba_backbones_golden.npz; state and inputs are regenerated from the seed.
RNN needs no golden of its own: its forward is pinned by rnn_golden.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np

REF = os.environ["ABD_REFERENCE"]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))   # tests/

import torch  # noqa: E402

import utils.models as ref_models  # noqa: E402
import daba_backbone_cases as dc  # noqa: E402


def main():
    B, T, Fd, K, _ = dc.CASES[dc.GOLDEN_CASE]
    x, _ = dc.make_inputs(dc.GOLDEN_CASE)
    m = ref_models.lstmwithattention(K, Fd, T)
    m.load_state_dict({k: torch.tensor(v) for k, v in dc.make_state(dc.GOLDEN_CASE).items()})
    assert m.training
    drawn = []
    m.dropout.register_forward_hook(lambda mod, inp, out: drawn.append((out != 0).to(torch.uint8).numpy().copy()))
    torch.manual_seed(dc.GOLDEN_TORCH_SEED)
    logits = []
    with torch.no_grad():
        for i in range(dc.GOLDEN_ROWS):
            logits.append(m.forward(torch.tensor(x[i:i + 1])).numpy()[0])
    out = {"mask": np.concatenate(drawn), "logits": np.stack(logits)}
    assert out["mask"].shape == (dc.GOLDEN_ROWS, 64) and out["logits"].dtype == np.float32
    path = os.path.join(HERE, "daba_backbones_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
