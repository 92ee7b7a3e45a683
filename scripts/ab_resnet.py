#!/usr/bin/env python3
"""A/B of the ResNet train step: libabd's fused step against PyTorch-ROCm's eager step on the same module.

    python scripts/ab_resnet.py [--batch 256] [--rounds 5] [--steps 10] [--out profiles/resnet/ab.md]

For (100, 40) and (32, 13) at the given batch: a reference-shaped torch.nn ResNet([2, 2, 2]) is trained one step at a
time either by torch (forward, CrossEntropyLoss, backward, Adam.step) or by training.resnet_train_step on the
adopted module.  The two sides alternate round by round in one process (same box, same session); each round times
`steps` steps between two device events after a warm-up, and the median round is reported.  One more fused step
runs under torch.profiler to list each launch's device time and, for the conv GEMMs, the fraction of the 157.3 TF
fp32 matrix peak their useful FLOPs reach.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import abd_amd  # noqa: E402
from abd_amd import training as T  # noqa: E402
from abd_amd.models_resnet import UNITS, adopt  # noqa: E402
import resnet_cases as rc  # noqa: E402
from test_gpu_resnet import Reference  # noqa: E402

PEAK_TF = 157.3


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def conv_flops(B, H, W):
    """Useful FLOPs of one product (forward, data or weight gradient) of the fourteen GEMM convs, summed."""
    total = 0
    for u in range(1, len(UNITS)):
        _, C, h, w = rc.unit_shape(u, B, H, W)
        total += 2 * B * h * w * C * 9 * UNITS[u][2]
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    abd_amd.load_library()
    dev = torch.device("cuda", 0)
    lines = ["# ResNet train step: fused libabd step against PyTorch-ROCm eager", "",
             f"B = {args.batch}, {args.rounds} interleaved rounds of {args.steps} steps, median round, ms per step.", ""]
    for H, W in ((100, 40), (32, 13)):
        K = 10
        torch.manual_seed(0)
        x = torch.randn(args.batch, 1, H, W, device=dev)
        y = torch.randint(0, K, (args.batch,), device=dev)
        eager = Reference(K, rc.linear_features(H, W)).to(dev).train()
        ours = Reference(K, rc.linear_features(H, W)).to(dev).train()
        ours.load_state_dict(eager.state_dict())
        oe = torch.optim.Adam(eager.parameters(), lr=1e-4)
        oo = torch.optim.Adam(ours.parameters(), lr=1e-4)
        crit = nn.CrossEntropyLoss()
        m = adopt(ours)
        m.engine(x)
        adam = T.AdamBinding(m, oo)

        def step_eager():
            oe.zero_grad(set_to_none=True)
            crit(eager(x), y).backward()
            oe.step()

        def step_fused():
            T.resnet_train_step(m, x, y, None, adam, None)

        for fn in (step_eager, step_fused):
            timed(fn, 3)
        te, tf = [], []
        for _ in range(args.rounds):
            te.append(timed(step_eager, args.steps))
            tf.append(timed(step_fused, args.steps))
        e, f = statistics.median(te), statistics.median(tf)
        lines += [f"## ({H}, {W})", "", f"- eager: {e:.3f} ms (rounds {', '.join(f'{v:.3f}' for v in te)})",
                  f"- fused: {f:.3f} ms (rounds {', '.join(f'{v:.3f}' for v in tf)})",
                  f"- fused / eager: {f / e:.2f}", ""]
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step_fused()
                torch.cuda.synchronize()
            rows = sorted(prof.key_averages(), key=lambda r: -getattr(r, "device_time_total", 0))
            lines += ["| launch | calls | device time, us |", "|---|---|---|"]
            conv_us = {1: 0.0, 2: 0.0}
            for r in rows:
                us = getattr(r, "device_time_total", 0)
                if us <= 0:
                    continue
                lines.append(f"| `{r.key[:90]}` | {r.count} | {us:.1f} |")
                if "conv_kernel" in r.key:
                    conv_us[2 if r.key.rstrip(">( )").endswith("2") or ", 2>" in r.key else 1] += us
            fl = conv_flops(args.batch, H, W)
            lines.append("")
            if conv_us[1] > 0:
                lines.append(f"- conv GEMMs, forward + data gradient: {2 * fl / 1e6 / conv_us[1]:.2f} TF useful, "
                             f"{100 * 2 * fl / 1e6 / conv_us[1] / PEAK_TF:.1f} % of the {PEAK_TF} TF fp32 matrix peak")
            if conv_us[2] > 0:
                lines.append(f"- conv GEMMs, weight gradient: {fl / 1e6 / conv_us[2]:.2f} TF useful, "
                             f"{100 * fl / 1e6 / conv_us[2] / PEAK_TF:.1f} % of the peak")
            lines.append("")
        except Exception as ex:   # the timing above stands without the per-launch table
            lines += [f"(no per-launch table: {type(ex).__name__}: {ex})", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
