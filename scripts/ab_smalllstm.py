#!/usr/bin/env python3
"""A/B of the smalllstm train step: libabd's fused step against PyTorch-ROCm's eager step on the same module.

    python scripts/ab_smalllstm.py [--batch 256] [--rounds 5] [--steps 10] [--out profiles/smalllstm/ab.md]

For (100, 40) and (32, 13) at the given batch: a reference-shaped torch.nn smalllstm is trained one step at a time
either by torch (forward, CrossEntropyLoss, backward, Adam.step) or by training.smalllstm_train_step on the adopted
module.  The two sides alternate round by round in one process (same box, same session); each round times `steps`
steps between two device events after a warm-up, and the median round is reported with every round beside it.

    python scripts/ab_smalllstm.py --trace [--out profiles/smalllstm/ab.md]

A run of its own: after a warm-up, ONE fused step per geometry under torch.profiler (device activities only), every
launch's device time listed and grouped into the trunk, the projections and weight-gradient GEMMs, the four
recurrent launches and the rest.  With --out the table is appended to the file the timing run wrote.
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
from abd_amd.models_smalllstm import adopt  # noqa: E402
import smalllstm_cases as sc  # noqa: E402
from test_gpu_smalllstm import Reference  # noqa: E402

GROUPS = (("recurrence", ("lstm_rec_",)), ("projections and weight-gradient GEMMs", ("gemm_tiled_kernel",)),
          ("trunk", ("conv", "bn_", "pool_", "repack", "wgrad_reduce", "part_sum", "dropout_")))


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="the per-launch table of one fused step, nothing timed")
    args = ap.parse_args()
    abd_amd.load_library()
    dev = torch.device("cuda", 0)
    lines = ([f"# Per-launch device time, B = {args.batch}", ""] if args.trace else
             ["# smalllstm train step: fused libabd step against PyTorch-ROCm eager", "",
              f"B = {args.batch}, {args.rounds} interleaved rounds of {args.steps} steps, median round, ms per step.", ""])
    for H, W in ((100, 40), (32, 13)):
        K = 10
        torch.manual_seed(0)
        x = torch.randn(args.batch, 1, H, W, device=dev)
        y = torch.randint(0, K, (args.batch,), device=dev)
        eager = Reference(K, sc.rnn_features(H, W)).to(dev).train()
        ours = Reference(K, sc.rnn_features(H, W)).to(dev).train()
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
            T.smalllstm_train_step(m, x, y, None, adam, None)

        for fn in (step_eager, step_fused):
            timed(fn, 3)
        if args.trace:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                step_fused()
                torch.cuda.synchronize()
            rows = sorted(prof.key_averages(), key=lambda r: -getattr(r, "device_time_total", 0))
            lines += [f"## ({H}, {W}): one fused step under torch.profiler, a run of its own", "",
                      "| launch | calls | device time, us |", "|---|---|---|"]
            group_us = {g: 0.0 for g, _ in GROUPS}
            group_us["rest"] = 0.0
            for r in rows:
                us = getattr(r, "device_time_total", 0)
                if us <= 0:
                    continue
                lines.append(f"| `{r.key[:90]}` | {r.count} | {us:.1f} |")
                group_us[next((g for g, keys in GROUPS if any(k in r.key for k in keys)), "rest")] += us
            lines += ["", "| group | device time, us |", "|---|---|"] + [f"| {g} | {us:.1f} |" for g, us in group_us.items()]
            lines.append("")
            continue
        te, tf = [], []
        for _ in range(args.rounds):
            te.append(timed(step_eager, args.steps))
            tf.append(timed(step_fused, args.steps))
        e, f = statistics.median(te), statistics.median(tf)
        lines += [f"## ({H}, {W})", "", f"- eager: {e:.3f} ms (rounds {', '.join(f'{v:.3f}' for v in te)})",
                  f"- fused: {f:.3f} ms (rounds {', '.join(f'{v:.3f}' for v in tf)})",
                  f"- fused / eager: {f / e:.2f}", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a" if args.trace else "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
