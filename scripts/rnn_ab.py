#!/usr/bin/env python3
"""A/B timing of the RNN train step on one GPU, one process.

A: abd_rnn_train_step (forward + CE + backward + Adam, one C-ABI call).
B: the tests' torch restatement (tests/rnn_cases.Restated: PyTorch-ROCm's own nn.LSTM + linear, autograd,
   torch.optim.Adam) on the same box, same data, same weights.
The two alternate in warmed blocks; per-block times are HIP-event totals over the block.  The script also
times the tiled GEMM on the input-projection shape (25600 x 3072 x 768 for layers 1 and 2): a forward of a
one-step sequence of 25600 rows is those three GEMMs plus three recurrent steps that skip theirs.

A report, not a gate.  Usage: python scripts/rnn_ab.py [--blocks 6] [--steps 5] [--out FILE]
Per-kernel shares of A come from a profiler run of --profile N:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/rnn_ab.py --profile 5
and are summarised with
    python scripts/rnn_ab.py --shares DIR/.../<pid>_kernel_stats.csv --profile 5
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import abd_amd  # noqa: E402
from abd_amd import training as T  # noqa: E402
from abd_amd.models_rnn import RNN  # noqa: E402
import rnn_cases as rc  # noqa: E402

B, TN, FD, K = 256, 100, 40, 10
WARM = 2
PROJ_FLOP = 2.0 * B * TN * 3072 * 768   # one input projection of layers 1 / 2
PEAK_TF = 155.0                         # measured rate of the fp32 matrix pipe


def shares(path, steps):
    """Per-kernel share of the traced GPU time from a rocprofv3 --stats kernel_stats.csv, and the tiled
    GEMM's rate on the input projection where its launches can be told apart."""
    import csv
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    name = next(k for k in rows[0] if k.lower() == "name")
    dur = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    calls = next(k for k in rows[0] if k.lower() == "calls")
    tot = sum(float(r[dur]) for r in rows)
    rows.sort(key=lambda r: -float(r[dur]))
    lines = ["| kernel | launches / step | us / step | share |", "|---|---|---|---|"]
    for r in rows:
        d = float(r[dur])
        short = r[name].replace("(anonymous namespace)::", "").replace("void ", "")
        short = short.split("(")[0][:60]
        lines.append(f"| `{short}` | {int(r[calls]) / steps:.1f} | {d / 1e3 / steps:.1f} | {100 * d / tot:.1f} % |")
    lines.append(f"| total | | {tot / 1e3 / steps:.1f} | 100 % |")
    return "\n".join(lines)


def projection_rate(dev, reps=5):
    """TFLOP/s of the layer-1 input projection alone: an eval forward of a T = 1 sequence with B*T rows is
    that GEMM (K = 768 for layers 1, 2) plus three single recurrent steps without their GEMM; timing the whole
    call therefore bounds the GEMM's rate from below."""
    rows = B * TN
    m = RNN(K, FD).to(dev).eval()
    x = torch.randn((rows, 1, 1, FD), device=dev)
    with torch.no_grad():
        for _ in range(2):
            m(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            m(x)
        e1.record()
        e1.synchronize()
    ms = e0.elapsed_time(e1) / reps
    flop = 2.0 * rows * 3072 * (FD + 2 * 768)
    return flop / (ms * 1e-3) / 1e12, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=0, help="run only N libabd steps (for a profiler)")
    ap.add_argument("--shares", default=None, help="a rocprofv3 kernel_stats.csv to summarise")
    a = ap.parse_args()
    if a.shares:
        text = shares(a.shares, (a.profile or 5) + WARM)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    abd_amd.load_library()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = RNN(K, FD).to(dev).train()
    state = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    r = np.random.Generator(np.random.PCG64(1))
    x = torch.tensor((2 * r.normal(size=(B, 1, TN, FD))).astype(np.float32), device=dev)
    y = torch.tensor(r.integers(0, K, B), device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    eng = m.engine(x)
    adam = T.AdamBinding(m, opt)

    def step_a():
        T.rnn_train_step(m, x, y, None, adam, None)

    if a.profile:
        for _ in range(WARM + a.profile):
            step_a()
        torch.cuda.synchronize()
        return
    ref = rc.Restated(state, torch.float32).to(dev)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    crit = nn.CrossEntropyLoss()

    def step_b():
        ropt.zero_grad(set_to_none=True)
        crit(ref(x), y).backward()
        ropt.step()

    for f in (step_a, step_b):
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    times = {"abd": [], "torch": []}
    for _ in range(a.blocks):
        for name, f in (("abd", step_a), ("torch", step_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
    ws = abd_amd.load_library().abd_rnn_workspace_bytes(eng.h, B)
    lines = [f"RNN train step, B={B} T={TN} F={FD} K={K}, {a.blocks} alternating blocks of {a.steps} steps, "
             f"workspace {ws / 2**30:.2f} GiB"]
    for name, v in times.items():
        lines.append(f"{name}: median {statistics.median(v):.3f} ms/step (min {min(v):.3f}, max {max(v):.3f})")
    lines.append(f"ratio torch / abd: {statistics.median(times['torch']) / statistics.median(times['abd']):.2f}")
    tf, ms = projection_rate(dev)
    lines.append(f"input projections of {B * TN} rows (K = {FD}, 768, 768; three launches and three GEMM-less recurrent "
                 f"steps): {ms:.3f} ms, at least {tf:.1f} TFLOP/s = {100 * tf / PEAK_TF:.0f} % of {PEAK_TF:.0f} TF")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
