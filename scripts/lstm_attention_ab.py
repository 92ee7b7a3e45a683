#!/usr/bin/env python3
"""A/B timing of the lstmwithattention train step on one GPU, one process.

A: abd_lstmattn_train_step (forward + CE + backward + Adam, one C-ABI call).
B: the tests' torch restatement (tests/lstm_attention_cases.Restated: PyTorch-ROCm's own LSTM, conv2d,
   batch_norm, linear) on the device in float32: forward + CrossEntropyLoss + backward + torch.optim.Adam.
B = 256, T = 100, F = 40, K = 35.  The two are timed in alternating blocks (ABAB...), each block bracketed
by device events after a warm-up; the report gives the median block time per step of each side.
A report, not a gate.  Usage: python scripts/lstm_attention_ab.py [--blocks 8] [--steps 20] [--out FILE]

Kernel-trace shares of the libabd step:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/lstm_attention_ab.py --profile 20
runs only the libabd step (5 warm-up steps, then 20), and
    python scripts/lstm_attention_ab.py --shares DIR/.../<pid>_kernel_stats.csv --profile 20
prints each kernel's share of the traced time and its time per step (needs no GPU).
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
from abd_amd.models_lstm import lstmwithattention  # noqa: E402
import lstm_attention_cases as lc  # noqa: E402

B, TN, FD, K = 256, 100, 40, 35


def shares(path, steps):
    """Per-kernel share of the traced GPU time from a rocprofv3 --stats kernel_stats.csv."""
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
        short = short.split("(")[0].split("::")[-1][:60]
        lines.append(f"| `{short}` | {int(r[calls]) / steps:.1f} | {d / 1e3 / steps:.1f} | {100 * d / tot:.1f} % |")
    lines.append(f"| total | | {tot / 1e3 / steps:.1f} | 100 % |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=0, help="run only N libabd steps (for a profiler)")
    ap.add_argument("--shares", default=None, help="a rocprofv3 kernel_stats.csv to summarise")
    a = ap.parse_args()
    if a.shares:
        text = shares(a.shares, (a.profile or 20) + 5)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    abd_amd.load_library()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = lstmwithattention(K, FD, TN).to(dev).train()
    state = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    r = np.random.Generator(np.random.PCG64(1))
    x = torch.tensor((20 * r.normal(size=(B, 1, TN, FD))).astype(np.float32), device=dev)
    y = torch.tensor(r.integers(0, K, B), device=dev)
    mask = torch.tensor((r.uniform(size=(B, 64)) < 0.5).astype(np.uint8), device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    m.engine(x)
    adam = T.AdamBinding(m, opt)
    ref = lc.Restated(state, torch.float32).to(dev)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    crit = nn.CrossEntropyLoss()

    def step_a():
        T.lstm_train_step(m, x, y, None, adam, None, mask=mask)

    def step_b():
        ropt.zero_grad(set_to_none=True)
        crit(ref(x, True, mask), y).backward()
        ropt.step()

    if a.profile:
        for _ in range(5 + a.profile):
            step_a()
        torch.cuda.synchronize()
        return
    for f in (step_a, step_b):
        for _ in range(5):
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
    lines = [f"lstmwithattention train step, B={B} T={TN} F={FD} K={K}, {a.blocks} alternating blocks of {a.steps} steps"]
    for name, v in times.items():
        lines.append(f"{name}: median {statistics.median(v):.3f} ms/step (min {min(v):.3f}, max {max(v):.3f})")
    lines.append(f"ratio torch / abd: {statistics.median(times['torch']) / statistics.median(times['abd']):.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
