#!/usr/bin/env python3
"""A/B: TSBD's unlearning epoch and re-initialisation sweep three ways (profiles/tsbd/ab.md).

Workload: by default 2,048 device-resident rows of 100 x 40, K = 35, batch 256, f32split, Adam(lr 1e-4);
the same rows serve as validation, clean test and backdoor test set.
  unlearn   one call of train_unlearning (tsbd.py:108-138: the first batch) plus the three evaluations that
            follow it (tsbd.py:319-321)
  sweep     the 11-ratio re-initialisation sweep (tsbd.py:371-380), clean and backdoor evaluation per ratio
  (a) new        defense.unlearn_epoch / reinit_sweep: abd::smallcnn_unlearn_step, abd::reinit_weights
  (b) composed   from what the library offered before: a no-update train step, negation, abd::adam, the
                 record norm, the threshold (torch.topk) and the zeroing as torch tensor ops, load_state_dict
                 per variant, the same eval op
  (c) reference  the reference's loop shape on the package's autograd smallcnn: (-loss).backward(),
                 torch.optim.Adam, .item() per batch; copy.deepcopy per ratio and zero_reinit_weight on
                 Python lists
Runs alternate after a warm-up of each; every run is timed with HIP events and ends with a device sync.
The sides draw their own dropout masks and are compared by time only; parity is tests/test_gpu_tsbd.py's job.

    python scripts/tsbd_ab.py [--rows 2048] [--batch 256] [--repeats 5] [--out profiles/tsbd/ab.md]
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
from abd_amd import _lib as L, defense as D, models as M, training as T  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsbd", "ab.md"))
    a = ap.parse_args()
    abd_amd.load_library()
    from abd_amd import ops  # noqa: F401
    dev = torch.device("cuda", 0)
    lr, wratio = 1e-4, 0.7
    flat = M.geometry(a.H, a.W)
    g = torch.Generator().manual_seed(12)
    x = (torch.randn((a.rows, 1, a.H, a.W), generator=g) * 10.0).to(dev)
    y = torch.randint(0, a.classes, (a.rows,), generator=g).to(dev)
    ind = torch.ones(a.rows, dtype=torch.int64, device=dev)
    bounds = D.batch_bounds(a.rows, a.batch)
    criterion = torch.nn.CrossEntropyLoss()

    def fresh():
        torch.manual_seed(11)
        m = M.smallcnn(a.classes, flat).to(dev).set_gemm_precision(a.precision).train()
        m.engine(x[:a.batch])
        return m, torch.optim.Adam(m.parameters(), lr=lr)

    ma, oa = fresh()
    mb, ob = fresh()
    mc, oc_ = fresh()
    bd_model, _ = fresh()                                   # the backdoored model the sweep re-initialises
    eb = mb._engine
    adam_b = T.AdamBinding(mb, ob)
    table = D.row_table(bd_model, "conv")
    rec = table[6:9]

    def evaluate(m, sets=3):
        """temp_test three times through the eval op (sides a and b)."""
        eng = m._engine
        accs = []
        for _ in range(sets):
            metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
            for s, e in bounds:
                torch.ops.abd.smallcnn_eval_metrics(x[s:e], eng.params, eng.running, eng.K, a.precision, y[s:e], None, metrics)
            w = T.read_metrics(metrics)
            accs.append(w[2] / w[1])
        m.train()
        return accs

    def unlearn_new():
        out = D.unlearn_epoch(ma, x, y, oa, batch_size=a.batch)
        return out[0], evaluate(ma)[0]

    def unlearn_composed():
        metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
        T.train_step(mb, x[:a.batch], y[:a.batch], None, None, metrics, do_update=False)
        eb.grads.neg_()
        norm = eb.grads[rec[0]:rec[0] + rec[1] * rec[2]].view(rec[1], rec[2]).abs().sum(-1)
        stack = torch.stack([norm], 0).float()
        stack.mean(dim=0), stack.var(dim=0)
        adam_b.step += 1
        torch.ops.abd.adam(eb.params, eb.grads, eb.exp_avg, eb.exp_avg_sq, adam_b.step, lr, 0.9, 0.999, 1e-8)
        return T.read_metrics(metrics)[0] / len(bounds), evaluate(mb)[0]

    def unlearn_reference():
        mc.train()
        oc_.zero_grad()
        out = mc(x[:a.batch])
        loss = criterion(out, y[:a.batch])
        hits = out.data.max(1)[1].eq(y[:a.batch]).sum()
        total = loss.item()
        (-loss).backward()
        norm = mc.conv3.weight.grad.view(32, -1).abs().sum(dim=-1)
        oc_.step()
        stack = torch.stack([norm], 0).float()
        stack.mean(dim=0), stack.var(dim=0)
        accs = []
        mc.eval()
        with torch.no_grad():
            for _ in range(3):
                tl, tc = 0.0, 0
                for s, e in bounds:
                    o = mc(x[s:e])
                    tl += criterion(o, y[s:e]).item()
                    tc += o.data.max(1)[1].eq(y[s:e]).sum()
                accs.append(float(tc) / a.rows)
        mc.train()
        return total / len(bounds) + 0 * float(hits), accs[0]

    # the sweep's inputs: a model a few unlearning steps away from bd_model
    mu, ou = fresh()
    for _ in range(3):
        D.unlearn_epoch(mu, x, y, ou, batch_size=a.batch)
    names, scores, absdiff = D.neuron_weight_change(mu, bd_model, "conv")
    ranked = D.rank_neurons((names, scores))
    n2w = D.absdiff_rows(bd_model, absdiff, "conv")
    twin = M.smallcnn(a.classes, flat).to(dev).set_gemm_precision(a.precision)
    twin.engine(x[:a.batch])

    def sweep_new():
        return D.reinit_sweep(bd_model, x, y, x, y, ind, ranked, absdiff, D.REINIT_RATIO, wratio, a.batch)[-1][:2]

    def eval_pair(m):
        m.eval()
        eng = m.engine(x[:a.batch])
        res = []
        for use_ind in (None, ind):
            metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
            for s, e in bounds:
                torch.ops.abd.smallcnn_eval_metrics(x[s:e], eng.params, eng.running, eng.K, a.precision, y[s:e],
                                                    use_ind[s:e] if use_ind is not None else None, metrics)
            res.append(T.read_metrics(metrics))
        return 100 * res[0][2] / res[0][1], 100 * res[1][4] / res[1][3]

    def sweep_composed():
        _, sel, ks, _ = D.reinit_selection(bd_model, ranked, D.REINIT_RATIO, wratio)
        rows = [(o + i * n, n) for o, r, n in zip(table[0::3], table[1::3], table[2::3]) for i in range(r)]
        at = [0]
        for _, n in rows[:-1]:
            at.append(at[-1] + n)
        base = bd_model._engine.params
        last = None
        for v in range(len(ks)):
            chosen = [i for i in range(len(rows)) if sel[v, i]]
            merged = torch.cat([absdiff[at[i]:at[i] + rows[i][1]] for i in chosen])
            thr = torch.topk(merged, ks[v]).values[-1]
            flat_p = base.clone()
            for i in chosen:
                s, n = rows[i]
                seg = flat_p[s:s + n]
                seg[absdiff[at[i]:at[i] + n] >= thr] = 0.0
            sd = bd_model.state_dict()
            offs = D.param_offsets(bd_model)
            for k, o in zip(M.PARAM_ORDER, offs):
                sd[k] = flat_p[o:o + sd[k].numel()].view(sd[k].shape)
            twin.load_state_dict(sd)
            last = eval_pair(twin)
        return last

    def sweep_reference():
        last = None
        for ratio in D.REINIT_RATIO:
            top_num = int(len(ranked) * ratio)
            net = copy.deepcopy(bd_model)
            sd = net.state_dict()
            merge = []
            for layer, idx, _ in ranked[:top_num]:
                merge += n2w[f"{layer}.{idx}"]
            reinit = sorted(merge, reverse=True)[:int(len(merge) * wratio)]
            lo = min(reinit)
            for layer, idx, _ in ranked[:top_num]:
                where = [i for i, v in enumerate(n2w[f"{layer}.{idx}"]) if v >= lo]
                sd[layer][int(idx)].view(-1)[where] = 0.0
            net.load_state_dict(sd)
            net.eval()
            with torch.no_grad():
                cc = sum(int((net(x[s:e]).max(1)[1] == y[s:e]).sum()) for s, e in bounds)
                for s, e in bounds:
                    criterion(net(x[s:e]), y[s:e]).item()
                ah = sum(int((net(x[s:e]).max(1)[1] == y[s:e]).sum()) for s, e in bounds)
                for s, e in bounds:
                    criterion(net(x[s:e]), y[s:e]).item()
            last = (100 * cc / a.rows, 100 * ah / a.rows)
        return last

    sides = {"unlearn": {"new": ("(a) unlearn_epoch + 3 evaluations", unlearn_new),
                         "composed": ("(b) composed from the earlier entry points", unlearn_composed),
                         "reference": ("(c) reference loop shape (autograd, torch Adam, .item() per batch)", unlearn_reference)},
             "sweep": {"new": ("(a) reinit_sweep, 11 ratios", sweep_new),
                       "composed": ("(b) torch threshold + load_state_dict per ratio", sweep_composed),
                       "reference": ("(c) reference loop shape (deepcopy, Python lists)", sweep_reference)}}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    lines = ["# TSBD: the unlearning epoch and the re-initialisation sweep three ways", "",
             f"Workload: {a.rows} rows of {a.H} x {a.W}, K = {a.classes}, batch {a.batch} ({len(bounds)} batches), "
             f"{a.precision}, Adam(lr {lr}), wratio {wratio}.  Device: {torch.cuda.get_device_name(0)}.  "
             f"`scripts/tsbd_ab.py`, {a.warmup} warm-up and {a.repeats} alternated timed runs of each side, HIP events "
             "around the whole run.  `unlearn` is one call of train_unlearning (its first batch) plus the three "
             "evaluations of the set that follow it; `sweep` is 11 ratios, each evaluated on a clean and a backdoor set.", ""]
    for what, group in sides.items():
        for _ in range(a.warmup):
            for _, fn in group.values():
                timed(fn)
        times = {k: [] for k in group}
        last = {}
        for _ in range(a.repeats):
            for k, (_, fn) in group.items():
                ms, last[k] = timed(fn)
                times[k].append(ms)
        med = {k: statistics.median(v) for k, v in times.items()}
        lines += [f"## {what}", "", "| side | median ms | min | max | last result |", "|---|---|---|---|---|"]
        for k, (label, _) in group.items():
            lines.append(f"| {label} | {med[k]:.2f} | {min(times[k]):.2f} | {max(times[k]):.2f} | "
                         f"{last[k][0]:.4f}, {last[k][1]:.4f} |")
        lines += [""] + [f"Measured {k} / new = {med[k] / med['new']:.2f}." for k in med if k != "new"] + [""]
    if a.out and a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
