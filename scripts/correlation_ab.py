#!/usr/bin/env python3
"""A/B: the unlearning correlation analysis two ways (profiles/correlation/ab.md).

Workload: by default 512 device-resident rows of 100 x 40, K = 35, batch 256, f32split, Adam(lr 1e-4), 200
unlearning epochs per model (correlation_analysis.py:141-143: 400 steps in all, each on its set's first batch).
  (a) new        defense.correlation_analysis: one abd::smallcnn_unlearn_run per model, one abd::nwc_pair
  (b) composed   from what the library offered before: defense.unlearn_epoch(record_layer=None) 400 times,
                 alternating between the two models as the reference's loop does, two
                 defense.neuron_weight_change calls, Pearson r in numpy on the host
Runs alternate after a warm-up of each; every run is timed on the host clock around a device sync.  The
"enqueue" columns time the bare ops without any read-back: n steps through abd::smallcnn_unlearn_run against n
abd::smallcnn_unlearn_step calls, host time until the last call returns (per step) and until the device is done.
The sides draw their own dropout masks and are compared by time only; parity is tests/test_gpu_correlation.py's job.

    python scripts/correlation_ab.py [--epochs 200] [--batch 256] [--repeats 5] [--out profiles/correlation/ab.md]
"""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abd_amd  # noqa: E402
from abd_amd import _lib as L, defense as D, models as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--W", type=int, default=40)
    ap.add_argument("--classes", type=int, default=35)
    ap.add_argument("--precision", default="f32split")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlation", "ab.md"))
    a = ap.parse_args()
    abd_amd.load_library()
    from abd_amd import ops  # noqa: F401
    dev = torch.device("cuda", 0)
    lr = 1e-4
    g = torch.Generator().manual_seed(13)
    cx = (torch.randn((a.rows, 1, a.H, a.W), generator=g) * 10.0).to(dev)
    cy = torch.randint(0, a.classes, (a.rows,), generator=g).to(dev)
    bx = cx.clone()
    bx[:, :, -8:, :6] += 15.0
    by = torch.full((a.rows,), 3, dtype=torch.int64, device=dev)
    bd_model = M.smallcnn(a.classes, M.geometry(a.H, a.W)).to(dev).set_gemm_precision(a.precision)
    bd_model.engine(cx[:a.batch])

    def new():
        return D.correlation_analysis(bd_model, cx, cy, bx, by, lr_un=lr, unlearn_epochs=a.epochs,
                                      batch_size=a.batch).correlation

    def composed():
        mc, mb = copy.deepcopy(bd_model), copy.deepcopy(bd_model)
        oc, ob = (torch.optim.Adam(m.parameters(), lr=lr) for m in (mc, mb))
        for _ in range(a.epochs):
            D.unlearn_epoch(mc, cx, cy, oc, record_layer=None, batch_size=a.batch)
            D.unlearn_epoch(mb, bx, by, ob, record_layer=None, batch_size=a.batch)
        _, sc, _ = D.neuron_weight_change(mc, bd_model)
        _, sb, _ = D.neuron_weight_change(mb, bd_model)
        return float(np.corrcoef(sc.astype(np.float64), sb.astype(np.float64))[0, 1])

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def bare(run):
        """(host ms until the last call returned, ms until the device finished) of n bare steps."""
        m = copy.deepcopy(bd_model)
        e = m.engine(cx[:a.batch])
        mm, mv = torch.zeros_like(e.params), torch.zeros_like(e.params)
        n = a.epochs
        metrics = torch.zeros((n, L.METRICS_WORDS), dtype=torch.int64, device=dev)
        xb, yb = cx[:a.batch].contiguous(), cy[:a.batch].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if run:
            torch.ops.abd.smallcnn_unlearn_run(xb, yb, e.params, e.grads, mm, mv, e.running, e.nbt, metrics, None, None,
                                               a.classes, n, 1, lr, 0.9, 0.999, 1e-8, 1, 0, None, None, a.precision)
        else:
            for i in range(n):
                torch.ops.abd.smallcnn_unlearn_step(xb, yb, e.params, e.grads, mm, mv, e.running, e.nbt, metrics[i], None,
                                                    None, None, a.classes, 1 + i, lr, 0.9, 0.999, 1e-8, 1, i, None, None,
                                                    None, a.precision)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3

    sides = (("new", new), ("composed", composed))
    for _ in range(a.warmup):
        for _, fn in sides:
            fn()
        bare(True), bare(False)
    times = {k: [] for k, _ in sides}
    enq = {True: [], False: []}
    last = {}
    for _ in range(a.repeats):                                    # alternate: A B A B ...
        for k, fn in sides:
            ms, last[k] = timed(fn)
            times[k].append(ms)
        for run in (True, False):
            enq[run].append(bare(run))
    steps = 2 * a.epochs
    lines = [f"| form | runs (ms) | median ms | per step (us, {steps} steps) |", "|---|---|---|---|"]
    for k, _ in sides:
        med = statistics.median(times[k])
        lines.append(f"| {k} | {', '.join(f'{t:.1f}' for t in times[k])} | {med:.1f} | {med * 1e3 / steps:.1f} |")
    lines += ["", f"| bare ops, {a.epochs} steps | host enqueue per step (us), median | until device done per step (us), median |",
              "|---|---|---|"]
    for run, name in ((True, "abd::smallcnn_unlearn_run (one call)"), (False, "abd::smallcnn_unlearn_step x n")):
        h = statistics.median(t[0] for t in enq[run]) * 1e3 / a.epochs
        d = statistics.median(t[1] for t in enq[run]) * 1e3 / a.epochs
        lines.append(f"| {name} | {h:.1f} | {d:.1f} |")
    ratio = statistics.median(times["composed"]) / statistics.median(times["new"])
    lines += ["", f"composed / new = {ratio:.2f}x; r (own masks per side): new {last['new']:.4f}, composed {last['composed']:.4f}",
              f"geometry {a.H}x{a.W}, K={a.classes}, B={a.batch}, {a.precision}, {a.epochs} epochs per model, "
              f"{a.repeats} alternated repeats after {a.warmup} warm-up"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
