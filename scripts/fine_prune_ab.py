#!/usr/bin/env python3
"""A/B: Fine-Pruning's prune sweep two ways (profiles/fine_prune/ab.md).

Workload: the sweep of fp.py:164-195 over one clean and one backdoor test set, by default 2,048 device-resident
rows each of 101 x 40, K = 10, batch 256, f32split, 65 variants (the nested masks of a 128-unit ranking).
  (a) new        defense.fc_prune_sweep on both sets: one abd::smallcnn_fcprune_eval per batch, all variants
  (b) baseline   what the library offered before: per variant a patched flat parameter set (fc2.weight columns
                 zeroed, built once outside the timed region) and one abd::smallcnn_eval_metrics per batch
  (c) one eval   a single plain evaluation of both sets (one variant of (b)): the floor (a) is expected near
Runs alternate after a warm-up of each; every run is timed with HIP events and ends with a device sync.  Both
sides must return the same accuracies and losses within 1e-4; the script fails otherwise.

    python scripts/fine_prune_ab.py [--rows 2048] [--batch 256] [--variants 65] [--out profiles/fine_prune/ab.md]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import abd_amd  # noqa: E402
from abd_amd import _lib as L, defense as D, models as M, training as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--H", type=int, default=101)
    ap.add_argument("--W", type=int, default=40)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--variants", type=int, default=65)
    ap.add_argument("--precision", default="f32split")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_prune", "ab.md"))
    a = ap.parse_args()
    abd_amd.load_library()
    from abd_amd import ops  # noqa: F401
    dev = torch.device("cuda", 0)
    flat = M.geometry(a.H, a.W)
    g = torch.Generator().manual_seed(21)
    sets = []
    for _ in range(2):                                      # the clean and the backdoor test set
        x = (torch.randn((a.rows, 1, a.H, a.W), generator=g) * 10.0).to(dev)
        y = torch.randint(0, a.classes, (a.rows,), generator=g).to(dev)
        sets.append((x, y))
    torch.manual_seed(22)
    model = M.smallcnn(a.classes, flat).to(dev).set_gemm_precision(a.precision).eval()
    eng = model.engine(sets[0][0][:a.batch])
    act = D.hidden_activation(model, sets[0][0], a.batch)
    seq = D.rank_units(act)
    masks = torch.zeros((a.variants, 128), dtype=torch.uint8)
    for v in range(a.variants):                             # nested, as the sweep's own: the 2 v lowest units
        masks[v, torch.from_numpy(seq[:max(2 * v - 1, 0)])] = 1
    w0 = eng.offsets[14]
    patched = eng.params.repeat(a.variants, 1)
    for v in range(a.variants):
        patched[v, w0:w0 + a.classes * 128].view(a.classes, 128)[:, masks[v].ne(0).to(dev)] = 0.0
    bounds = D.batch_bounds(a.rows, a.batch)

    def eval_one(params, x, y):
        metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
        for s, e in bounds:
            torch.ops.abd.smallcnn_eval_metrics(x[s:e], params, eng.running, eng.K, a.precision, y[s:e], None, metrics)
        return metrics

    def new():
        return [D.fc_prune_sweep(model, x, y, masks, a.batch) for x, y in sets]

    def baseline():
        out = []
        for x, y in sets:
            words = [T.read_metrics(m) for m in [eval_one(patched[v], x, y) for v in range(a.variants)]]
            out.append((np.array([w[0] / len(bounds) for w in words]), np.array([w[2] / w[1] for w in words])))
        return out

    def one_eval():
        return [T.read_metrics(eval_one(eng.params, x, y)) for x, y in sets]

    sides = (("new", new), ("baseline", baseline), ("one eval", one_eval))
    results, times = {}, {name: [] for name, _ in sides}
    for _ in range(a.warmup):
        for name, fn in sides:
            results[name] = fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for name, fn in sides:                              # alternate
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
    worst_loss = worst_acc = 0.0
    for (nl, na), (bl, ba) in zip(results["new"], results["baseline"]):
        worst_loss = max(worst_loss, float(np.abs(nl.numpy() - bl).max()))
        worst_acc = max(worst_acc, float(np.abs(na.numpy() - ba).max()))
    if worst_loss > 1e-4 or worst_acc != 0.0:
        raise SystemExit(f"the two sides disagree: loss {worst_loss:.2e}, accuracy {worst_acc:.2e}")
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [
        "# Fine-Pruning's prune sweep: A/B on one MI355X", "",
        f"`python scripts/fine_prune_ab.py --rows {a.rows} --batch {a.batch} --variants {a.variants}`: two sets of "
        f"{a.rows} rows of {a.H}x{a.W}, K = {a.classes}, {a.precision}, {len(bounds)} batches per set; runs alternate, "
        f"{a.warmup} warm-up and {a.repeats} timed runs per side, HIP events around each run (device sync at the end).",
        "", "| side | median ms | min | max | launches of an eval forward per set |", "|---|---|---|---|---|"]
    per = {"new": len(bounds), "baseline": a.variants * len(bounds), "one eval": len(bounds)}
    for name, _ in sides:
        v = times[name]
        lines.append(f"| {name} | {med[name]:.2f} | {min(v):.2f} | {max(v):.2f} | {per[name]} |")
    lines += ["", f"baseline / new = {med['baseline'] / med['new']:.1f}x; new / one eval = "
              f"{med['new'] / med['one eval']:.2f}x.  Largest difference between the sides over both sets and all "
              f"variants: loss {worst_loss:.2e}, accuracy {worst_acc:.1e}."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
