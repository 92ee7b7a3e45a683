#!/usr/bin/env python3
"""A/B: one epoch of regularised fine-tuning (ft_reg.py:83-123) three ways (profiles/finetune_reg/ab.md).

Workload: by default 2,048 device-resident rows of 100 x 40, K = 35, batch 256, f32split,
SGD(lr 0.01, momentum 0.9), r = 0.05, alpha = 0.7.
  (a) epoch      defense.finetune_reg_epoch: one abd::smallcnn_finetune_reg_step per batch
  (b) composed   the same arithmetic from what the library offered before: two no-update train steps, the
                 norms / displacement / blend / SGD as torch tensor ops on the flat buffers, a train-mode
                 forward, torch's CrossEntropyLoss
  (c) reference  the reference's loop shape on the package's autograd smallcnn: copy.deepcopy(model) per
                 batch, two .backward() calls, torch.optim.SGD, a third forward
Runs alternate (a, b, c, a, b, c, ...) after a warm-up of each; every run is timed with HIP events around
the whole epoch and ends with a device sync.  The dropout masks differ between the sides (each draws its
own), so the sides are compared by time only; parity is tests/test_gpu_finetune.py's job.

    python scripts/finetune_reg_ab.py [--rows 2048] [--batch 256] [--repeats 5] [--only epoch]
                                      [--out profiles/finetune_reg/ab.md]
"""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abd_amd  # noqa: E402
from abd_amd import defense as D, models as M, training as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--H", type=int, default=100)
    ap.add_argument("--W", type=int, default=40)
    ap.add_argument("--classes", type=int, default=35)
    ap.add_argument("--precision", default="f32split")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="", help="time one side only: epoch, composed or reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune_reg", "ab.md"))
    a = ap.parse_args()
    abd_amd.load_library()
    from abd_amd import ops  # noqa: F401
    dev = torch.device("cuda", 0)
    r, alpha, lr, mu = 0.05, 0.7, 0.01, 0.9
    flat = M.geometry(a.H, a.W)
    g = torch.Generator().manual_seed(12)
    x = (torch.randn((a.rows, 1, a.H, a.W), generator=g) * 10.0).to(dev)
    y = torch.randint(0, a.classes, (a.rows,), generator=g).to(dev)
    bounds = D.batch_bounds(a.rows, a.batch)
    criterion = torch.nn.CrossEntropyLoss()

    def fresh():
        torch.manual_seed(11)
        m = M.smallcnn(a.classes, flat).to(dev).set_gemm_precision(a.precision).train()
        m.engine(x[:a.batch])
        return m, torch.optim.SGD(m.parameters(), lr=lr, momentum=mu)

    ma, oa = fresh()
    mb, _ = fresh()
    mc, oc_ = fresh()
    eb = mb._engine
    bufb = torch.zeros_like(eb.params)

    def run_epoch():
        return D.finetune_reg_epoch(ma, x, y, oa, r, alpha, batch_size=a.batch)[:2]

    def run_composed():
        total, hits = torch.zeros((), device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        for s, e in bounds:
            xb, yb = x[s:e], y[s:e]
            p0, run0, nbt0 = eb.params.clone(), eb.running.clone(), eb.nbt.clone()
            T.train_step(mb, xb, yb, None, None, None, do_update=False)
            g1 = eb.grads.clone()
            norms = torch.stack(torch._foreach_norm(eb.views(g1)))
            sizes = torch.tensor([v.numel() for v in eb.views(g1)], device=dev)
            eb.params.add_(g1 / torch.repeat_interleave(norms, sizes), alpha=r)
            T.train_step(mb, xb, yb, None, None, None, do_update=False)
            eb.params.copy_(p0)
            eb.running.copy_(run0)
            eb.nbt.copy_(nbt0)
            eb.grads.mul_(alpha).add_(g1, alpha=1 - alpha)
            bufb.mul_(mu).add_(eb.grads)
            eb.params.add_(bufb, alpha=-lr)
            out = mb.hip_forward(xb, train=True)
            total += criterion(out, yb)
            hits += (out.max(1)[1] == yb).sum()
        return float(total) / len(bounds), int(hits) / a.rows

    def run_reference():
        total, hits = 0.0, 0
        for s, e in bounds:
            xb, yb = x[s:e], y[s:e]
            tmp = copy.deepcopy(mc)
            loss1 = criterion(tmp(xb), yb)
            tmp.zero_grad()
            loss1.backward()
            g1 = [p.grad.data.clone() for p in tmp.parameters()]
            with torch.no_grad():
                for p, gr in zip(tmp.parameters(), g1):
                    p.data += r * (gr / gr.norm())
            loss2 = criterion(tmp(xb), yb)
            tmp.zero_grad()
            loss2.backward()
            g2 = [p.grad.data.clone() for p in tmp.parameters()]
            oc_.zero_grad()
            for p, u, v in zip(mc.parameters(), g1, g2):
                p.grad = (1 - alpha) * u + alpha * v
            oc_.step()
            out = mc(xb)
            total += criterion(out, yb).item()
            hits += int((out.data.max(1)[1] == yb).sum())
        return total / len(bounds), hits / a.rows

    sides = {"epoch": ("(a) finetune_reg_epoch, one op per batch", run_epoch),
             "composed": ("(b) composed from the earlier primitives + torch tensor ops", run_composed),
             "reference": ("(c) reference loop shape: deepcopy, 2 x backward(), torch SGD", run_reference)}
    if a.only:
        sides = {a.only: sides[a.only]}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    for _ in range(a.warmup):
        for _, fn in sides.values():
            timed(fn)
    times = {k: [] for k in sides}
    last = {}
    for _ in range(a.repeats):
        for k, (_, fn) in sides.items():
            ms, last[k] = timed(fn)
            times[k].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["# Regularised fine-tuning: one epoch three ways", "",
             f"Workload: {a.rows} rows of {a.H} x {a.W}, K = {a.classes}, batch {a.batch} ({len(bounds)} batches), "
             f"{a.precision}, SGD(lr {lr}, momentum {mu}), r = {r}, alpha = {alpha}.  Device: "
             f"{torch.cuda.get_device_name(0)}.  `scripts/finetune_reg_ab.py`, {a.warmup} warm-up and {a.repeats} "
             "alternated timed epochs of each side, HIP events around the whole epoch.", "",
             "| side | median ms / epoch | min | max | ms / batch | last (loss, acc) |", "|---|---|---|---|---|---|"]
    for k, (label, _) in sides.items():
        lines.append(f"| {label} | {med[k]:.2f} | {min(times[k]):.2f} | {max(times[k]):.2f} | "
                     f"{med[k] / len(bounds):.3f} | {last[k][0]:.4f}, {last[k][1]:.4f} |")
    if "epoch" in med:
        lines += [""] + [f"Measured {k} / epoch = {med[k] / med['epoch']:.2f}." for k in med if k != "epoch"]
    lines.append("")
    if a.out and a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
