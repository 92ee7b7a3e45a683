#!/usr/bin/env python3
"""DABA selection on the lstmwithattention and RNN victims: batched scores against a loop of batch-1 forwards.

    python scripts/daba_backbones_ab.py --mode ab --out DIR        # on the GPU: writes DIR/ab.json
    rocprofv3 --kernel-trace --stats -d DIR/kt -o kt -f csv -- \\
        python scripts/daba_backbones_ab.py --mode profile         # a run of its own, no counters
    python scripts/daba_backbones_ab.py --mode report --out DIR --stats DIR/kt/.../kt_kernel_stats.csv \\
        > profiles/daba_backbones/ab.md

Per backbone at (T, F) = (32, 40), 60 pool clips and 3000 ragged hosts (seeded noise, 0.5 .. 1 s at 16 kHz):
  batched  DabaSelector.certainty + DabaSelector.influence, wall time up to the scores on the host;
  loop     what the code before the per-utterance entry point offers for the same arithmetic: the same batched
           overlay + MFCC front end, then ONE batch-1 call per forward -- lstmwithattention.hip_forward(train=True)
           (abd_lstmattn_forward, train_mode 1) or torch.ops.abd.rnn_eval (abd_rnn_eval) -- and the same scoring
           kernels.  Timed on 60 pool clips + LOOP_HOSTS hosts; the host part is scaled to 3000.
The two alternate in one process, ROUNDS times each, after one warm-up of either.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T, F, K = 32, 40, 10
POOL, HOSTS, LOOP_HOSTS, ROUNDS, PROFILE_PASSES = 60, 3000, 300, 3, 3
FRONT = "front_per_utterance_kernel"
HBM_GBS = 8000.0   # MI355X peak HBM bandwidth, GB/s


def clips(n, seed):
    import numpy as np
    r = np.random.Generator(np.random.PCG64(seed))
    return [np.clip(r.normal(0, 4000, int(r.integers(8000, 16001))), -32768, 32767).astype(np.int16) for _ in range(n)]


def victim(kind, dev):
    import torch
    from abd_amd import daba as D
    torch.manual_seed(35)
    return D.load_victim_model(argparse.Namespace(model=kind, num_classes=K, n_mfcc=F)).to(dev)


def batched(sel, pool, hosts):
    import torch
    t0 = time.perf_counter()
    sel.certainty(pool)
    sel.influence(pool[0], hosts)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def loop(sel, kind, pool, hosts):
    """-> (seconds of the pool part, seconds of the host part)"""
    import torch
    from abd_amd import daba as D
    m = sel.sel.model

    def one_by_one(x):
        if kind == "RNN":
            eng = m.engine(x)
            return torch.cat([torch.ops.abd.rnn_eval(x[i:i + 1], eng.params, eng.K) for i in range(x.shape[0])])
        return torch.cat([m.hip_forward(x[i:i + 1], train=True) for i in range(x.shape[0])])

    t0 = time.perf_counter()
    D.softmax_entropy(one_by_one(sel.clip_inputs(pool)))[1].cpu()
    t1 = time.perf_counter()
    n = len(hosts)
    xt = sel.clip_inputs([pool[0]]).expand(n, -1, -1, -1)
    x = torch.cat([xt, sel.poisoned_inputs(pool[0], hosts)]).contiguous()
    probs, _ = D.softmax_entropy(one_by_one(x))
    D.pair_cross_entropy(probs[:n].contiguous(), probs[n:].contiguous()).cpu()
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t1


def run_ab(out):
    import torch
    import abd_amd
    from abd_amd import daba as D
    abd_amd.load_library()
    dev = torch.device("cuda", 0)
    pool, hosts = clips(POOL, 1), clips(HOSTS, 2)
    res = {"T": T, "F": F, "pool": POOL, "hosts": HOSTS, "loop_hosts": LOOP_HOSTS, "rounds": ROUNDS}
    for kind in ("lstmwithattention", "RNN"):
        sel = D.DabaSelector(victim(kind, dev), dev)
        batched(sel, pool, hosts)
        loop(sel, kind, pool[:4], hosts[:8])
        b, lp, lh = [], [], []
        for _ in range(ROUNDS):
            b.append(batched(sel, pool, hosts))
            p, h = loop(sel, kind, pool, hosts[:LOOP_HOSTS])
            lp.append(p)
            lh.append(h)
        res[kind] = {"batched_s": b, "loop_pool_s": lp, "loop_hosts_s": lh}
        print(kind, res[kind], flush=True)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "ab.json"), "w") as f:
        json.dump(res, f, indent=1)


def run_profile():
    import torch
    import abd_amd
    from abd_amd import daba as D
    abd_amd.load_library()
    dev = torch.device("cuda", 0)
    pool, hosts = clips(POOL, 1), clips(HOSTS, 2)
    sel = D.DabaSelector(victim("lstmwithattention", dev), dev)
    for _ in range(PROFILE_PASSES):
        batched(sel, pool, hosts)


def report(out, stats):
    with open(os.path.join(out, "ab.json")) as f:
        res = json.load(f)
    scale = res["hosts"] / res["loop_hosts"]
    print("# DABA selection on the LSTM backbones: batched scores against a loop of batch-1 forwards\n")
    print(f"MI355X, (T, F) = ({res['T']}, {res['F']}), {res['pool']} pool clips, {res['hosts']} hosts; "
          f"scripts/daba_backbones_ab.py, {res['rounds']} alternating rounds in one process after a warm-up of either. "
          f"The loop is timed on {res['pool']} pool clips + {res['loop_hosts']} hosts and its host part is scaled by "
          f"{scale:g} to {res['hosts']} hosts (scaled, not measured).\n")
    print("| victim | batched certainty + influence, s (each round) | median | loop, s (pool + scaled hosts, each round) "
          "| median | loop / batched |")
    print("|---|---|---|---|---|---|")
    for kind in ("lstmwithattention", "RNN"):
        r = res[kind]
        lo = [p + h * scale for p, h in zip(r["loop_pool_s"], r["loop_hosts_s"])]
        mb, ml = statistics.median(r["batched_s"]), statistics.median(lo)
        print(f"| {kind} | {', '.join(f'{v:.3f}' for v in r['batched_s'])} | {mb:.3f} | "
              f"{', '.join(f'{v:.2f}' for v in lo)} | {ml:.2f} | {ml / mb:.1f}x |")
    print("\nBoth columns include the clip packing, the overlay and the MFCC front end, which are the same work.\n")
    if not stats:
        print("Front kernel: not measured.")
        return
    with open(stats) as f:
        rows = [r for r in csv.DictReader(f) if FRONT in r["Name"]]
    calls = sum(int(r["Calls"]) for r in rows)
    ns = sum(int(r["TotalDurationNs"]) for r in rows)
    # per profiled pass: the pool's rows, then the 2 * hosts rows of influence in chunks
    passes = PROFILE_PASSES
    byts = passes * (res["pool"] + 2 * res["hosts"]) * 8 * res["T"] * res["F"]
    print(f"## {FRONT}\n")
    print(f"rocprofv3 --kernel-trace --stats (a run of its own, no counters), {passes} passes of certainty + influence: "
          f"{calls} launches, {ns / 1e3:.1f} us in all, {ns / calls / 1e3:.1f} us per launch on average. Its byte model is "
          f"8*T*F bytes per utterance (x read once, x0 written once): {byts / 1e6:.1f} MB over {ns / 1e3:.1f} us = "
          f"{byts / ns:.1f} GB/s achieved, {100.0 * byts / ns / HBM_GBS:.1f} % of the {HBM_GBS / 1000:g} TB/s HBM peak "
          f"(per element the kernel also spends 50 + 250 FMAs recomputing conv1 in passes 1 and 2).")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("ab", "profile", "report"), default="ab")
    ap.add_argument("--out", default="out/daba_backbones")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.mode == "ab":
        run_ab(a.out)
    elif a.mode == "profile":
        run_profile()
    else:
        report(a.out, a.stats)
