#!/usr/bin/env python3
"""A/B: the batched neuron-ablation sweep against per-variant evals (profiles/ablation_sweep/ab.md).

Workload: the defenses' loss-change scan (ft_reg.py:173-190) of all 160 conv filters over one
device-resident set -- by default 2,048 rows of 100 x 40, K = 35, batch 256, f32split.
  (a) sweep      torch.ops.abd.smallcnn_ablate_eval, one call per batch for all variants
  (b) per-eval   what the library offered before: one abd_smallcnn_eval per (variant, batch) on 160
                 device-resident patched parameter copies (no deepcopy, no load_state_dict, no host
                 loader: the comparison flatters the old way)
Runs alternate (a, b, a, b, ...) after a warm-up of both; each run is timed with HIP events around
the whole set and ends with a device sync; the table reports the median and the spread.  Both sides'
losses are compared, so the A/B times the same computation.

    python scripts/ablation_ab.py [--rows 2048] [--batch 256] [--repeats 5] [--out profiles/ablation_sweep/ab.md]
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
from abd_amd import _lib as L, defense as D, models as M  # noqa: E402


def layer_flops(H0, W0, K):
    """Multiply-adds per input row of each stage (the work model's units)."""
    H1, W1 = H0 - 1, W0 - 1
    W1p = W1 // 3
    H2, W2 = H1 - 1, W1p - 1
    H2p, W2p = H2 // 2 + 1, W2 // 2 + 1
    H3, W3 = H2p - 1, W2p - 1
    flat = 32 * ((H3 - 2) // 2 + 1) * (W3 // 2 + 1)
    f = dict(conv1=H1 * W1 * 64 * 4, conv2=H2 * W2 * 64 * 256, conv3=H3 * W3 * 32 * 256, head=flat * 128 + 128 * K)
    bytes_fuse2 = 4 * (H2 * W2 * 64 + H2p * W2p * 64)      # z2 read (L2-resident across variants) + p2' written
    bytes_fuse3 = 4 * (H3 * W3 * 32 + flat)
    return f, bytes_fuse2, bytes_fuse3, flat


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ablation_sweep", "ab.md"))
    a = ap.parse_args()
    abd_amd.load_library()
    from abd_amd import ops
    dev = torch.device("cuda", 0)
    torch.manual_seed(11)
    flops, bf2, bf3, flat = layer_flops(a.H, a.W, a.classes)
    model = M.smallcnn(a.classes, flat).eval().set_gemm_precision(a.precision)
    with torch.no_grad():   # BN statistics of a trained model, not the identity
        for bn in (model.bn1, model.bn2, model.bn3):
            bn.running_mean.normal_(0.5, 0.5)
            bn.running_var.uniform_(0.2, 3.0)
    g = torch.Generator().manual_seed(12)
    x = (torch.randn((a.rows, 1, a.H, a.W), generator=g) * 10.0).to(dev)
    y = torch.randint(0, a.classes, (a.rows,), generator=g).to(dev)
    names = D.neuron_names(model, "conv")
    masks, _ = D.pack_masks([[n] for n in names])
    V = len(names)
    params, running = D._flat_state(model, dev)
    bounds = D.batch_bounds(a.rows, a.batch)
    h = ops._net(a.H, a.W, a.classes, a.precision)
    vpp = D.pick_variants_per_pass(h, a.batch, V, a.H, a.W, dev)

    # (b): patched parameter copies, resident
    import ctypes as C
    o = (C.c_int64 * 17)()
    L.check(L.lib().abd_smallcnn_param_offsets(h, o), "offsets")
    offs = list(o)
    patched = params.repeat(V, 1)
    for v in range(V):
        layer, c = (0, v) if v < 64 else (1, v - 64) if v < 128 else (2, v - 128)
        w0 = offs[4 * layer]
        per = (offs[4 * layer + 1] - w0) // (64 if layer < 2 else 32)
        patched[v, w0 + c * per:w0 + (c + 1) * per] = 0.0
    metrics = torch.zeros((V, L.METRICS_WORDS), dtype=torch.int64, device=dev)

    def run_sweep():
        ls = torch.zeros((len(bounds), V), dtype=torch.float64, device=dev)
        co = torch.zeros(V, dtype=torch.int64, device=dev)
        for i, (s, e) in enumerate(bounds):
            torch.ops.abd.smallcnn_ablate_eval(x[s:e], params, running, y[s:e], masks, 0, vpp, ls[i], co, a.classes,
                                               a.precision)
        return ls, co

    def run_evals():
        metrics.zero_()
        for s, e in bounds:
            for v in range(V):
                torch.ops.abd.smallcnn_eval_metrics(x[s:e], patched[v], running, a.classes, a.precision, y[s:e], None,
                                                    metrics[v])
        return metrics

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    for _ in range(a.warmup):
        timed(run_sweep)
        timed(run_evals)
    ta, tb = [], []
    for _ in range(a.repeats):
        ms, (ls, co) = timed(run_sweep)
        ta.append(ms)
        ms, met = timed(run_evals)
        tb.append(ms)
    # same numbers on both sides: mean of batch means, correct counts
    sizes = torch.tensor([e - s for s, e in bounds], dtype=torch.float64, device=dev)
    loss_a = (ls / sizes[:, None]).mean(0).cpu().numpy()
    loss_b = (met[:, 0].view(torch.float64) / met[:, 5].to(torch.float64)).cpu().numpy()
    rel = float(np.abs(loss_a / loss_b - 1).max())
    same_correct = bool(torch.equal(co, met[:, 2]))

    full = sum(flops.values())
    model_work = full + 64 * (flops["conv3"] + flops["head"]) + 96 * flops["head"]
    traffic = a.rows * (64 * bf2 + 64 * bf3)
    med_a, med_b = statistics.median(ta), statistics.median(tb)
    lines = [
        "# Neuron-ablation sweep vs per-variant evals", "",
        f"Workload: {a.rows} rows of {a.H} x {a.W}, K = {a.classes}, batch {a.batch}, {a.precision}, all {V} "
        f"single-filter variants, {vpp} variants per pass.  Device: {torch.cuda.get_device_name(0)}.  "
        f"`scripts/ablation_ab.py`, {a.warmup} warm-up and {a.repeats} alternated timed runs of each side, HIP "
        "events around the whole set.", "",
        "| side | median ms | min | max |", "|---|---|---|---|",
        f"| (a) sweep, one call per batch | {med_a:.2f} | {min(ta):.2f} | {max(ta):.2f} |",
        f"| (b) {V} x abd_smallcnn_eval per batch, resident patched copies | {med_b:.2f} | {min(tb):.2f} | {max(tb):.2f} |",
        "", f"Measured (b) / (a) = {med_b / med_a:.2f}.", "",
        f"Both sides computed the same scan: max relative loss difference {rel:.2e}, correct counts "
        f"{'equal' if same_correct else 'DIFFER'}.", "",
        "## Work model", "",
        "Multiply-adds per row: " + ", ".join(f"{k} {v:,}" for k, v in flops.items()) + f" (full forward {full:,}).",
        f"(b) does {V} full forwards per row: {V * full:,}.  (a) does 1 baseline forward + 64 x (conv3 + head) + "
        f"96 x head = {model_work:,}, plus the fused kernels' traffic ({traffic / 1e9:.2f} GB over the set: z and "
        "the pooled rows of 64 conv1 + 64 conv2 variants).",
        f"Predicted ratio from multiply-adds alone: {V * full / model_work:.1f}x; the sweep's added traffic and "
        "its per-pass launches pull the measured ratio below that.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
