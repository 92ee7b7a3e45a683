#!/usr/bin/env python3
"""A/B timing of the largecnn train step on one GPU, one process.

A: abd_largecnn_train_step (forward + CE + backward + Adam, one C-ABI call).
B: PyTorch-ROCm's eager step of a reference-shaped module (torch.nn layers, autograd, torch.optim.Adam) on the
   same box, same data, same weights.
Run at B = 256, K = 10 on (100, 40) and (32, 13) inputs.  The two alternate in warmed blocks; per-block times are
HIP-event totals over the block.

A report, not a gate.  Usage: python scripts/ab_largecnn.py [--blocks 5] [--steps 3] [--out FILE]
Per-kernel shares of A come from a profiler run of its own (no counters mixed in):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/ab_largecnn.py --profile 3
and profiles/largecnn/ab.md is written from the timing text, the run's kernel statistics and its kernel trace
(each conv GEMM launch's time and the fraction of the fp32 matrix peak it reaches, FLOPs from its shape) with
    python scripts/ab_largecnn.py --profile 3 --times FILE --shares DIR/.../<pid>_kernel_stats.csv \
        --trace DIR/.../<pid>_kernel_trace.csv --out profiles/largecnn/ab.md
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import abd_amd  # noqa: E402
from abd_amd import training as T  # noqa: E402
from abd_amd.models_largecnn import CONVS, largecnn, linear_features  # noqa: E402

B, K = 256, 10
GEOMETRIES = ((100, 40), (32, 13))
WARM = 2
PEAK_TF = 157.3   # fp32 matrix peak


class Eager(nn.Module):
    """The reference's network from torch.nn layers (utils/models.py:68-119)."""

    def __init__(self, num_classes, lf):
        super().__init__()
        for (name, cin, cout) in CONVS:
            setattr(self, name, nn.Conv2d(cin, cout, kernel_size=(3, 3), stride=1, padding=1))
        self.pool1, self.pool2 = nn.MaxPool2d((2, 2)), nn.MaxPool2d((2, 2))
        self.pool3 = nn.MaxPool2d((3, 3), stride=(2, 2))
        self.fc1, self.fc2, self.fc3 = nn.Linear(lf, 256), nn.Linear(256, 128), nn.Linear(128, num_classes)
        self.dropout1, self.dropout2 = nn.Dropout(0.5), nn.Dropout(0.5)

    def forward(self, x):
        x = self.pool2(self.conv2(self.pool1(self.conv1(x))))
        x = torch.relu(self.conv5(torch.relu(self.conv4(torch.relu(self.conv3(x))))))
        x = self.pool3(x).flatten(1)
        x = self.dropout1(torch.relu(self.fc1(x)))
        x = self.dropout2(torch.relu(self.fc2(x)))
        return torch.log_softmax(self.fc3(x), dim=1)


def conv_gemm_flop(H, W):
    """FLOP of one step's conv GEMM launches from their shapes: forward and weight gradient of conv2..conv5,
    data gradient of conv2..conv5 (conv2's feeds conv1's weight gradient)."""
    px = {"conv2": B * (H // 2) * (W // 2)}
    for n in ("conv3", "conv4", "conv5"):
        px[n] = B * (H // 4) * (W // 4)
    return sum(3 * 2.0 * px[n] * 9 * cin * cout for n, cin, cout in CONVS[1:])


def shares(path, steps, H, W):
    import csv
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    name = next(k for k in rows[0] if k.lower() == "name")
    dur = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    calls = next(k for k in rows[0] if k.lower() == "calls")
    tot = sum(float(r[dur]) for r in rows)
    rows.sort(key=lambda r: -float(r[dur]))
    lines = ["| kernel | launches / step | us / step | share |", "|---|---|---|---|"]
    gemm = 0.0
    for r in rows:
        d = float(r[dur])
        if "conv_gemm_kernel" in r[name]:
            gemm += d
        short = r[name].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:60]
        lines.append(f"| `{short}` | {int(r[calls]) / steps:.1f} | {d / 1e3 / steps:.1f} | {100 * d / tot:.1f} % |")
    lines.append(f"| total | | {tot / 1e3 / steps:.1f} | 100 % |")
    if gemm:
        tf = conv_gemm_flop(H, W) / (gemm * 1e-9 / steps) / 1e12
        lines.append("")
        lines.append(f"conv_gemm_kernel launches together (conv2..conv5 forward, data and weight gradients, "
                     f"{conv_gemm_flop(H, W) / 1e12:.3f} TFLOP per step, and the fc head): {gemm / 1e6 / steps:.2f} ms "
                     f"per step, {tf:.1f} TFLOP/s = {100 * tf / PEAK_TF:.0f} % of the {PEAK_TF} TF fp32 matrix peak")
    return "\n".join(lines)


def gemm_launches(H, W):
    """The conv_gemm_kernel launches of one step in launch order: (what, FLOP)."""
    px = {"conv2": B * (H // 2) * (W // 2)}
    for n in ("conv3", "conv4", "conv5"):
        px[n] = B * (H // 4) * (W // 4)
    lf = linear_features(H, W)
    conv = {n: 2.0 * px[n] * 9 * cin * cout for n, cin, cout in CONVS[1:]}
    fc = {"fc1": 2.0 * B * lf * 256, "fc2": 2.0 * B * 256 * 128, "fc3": 2.0 * B * 128 * K}
    out = [(f"{n} forward", conv[n]) for n in ("conv2", "conv3", "conv4", "conv5")]
    out += [(f"{n} forward", fc[n]) for n in ("fc1", "fc2", "fc3")]
    for n in ("fc3", "fc2", "fc1"):
        out += [(f"{n} weight gradient", fc[n]), (f"{n} data gradient", fc[n])]
    for n in ("conv5", "conv4", "conv3", "conv2"):
        out += [(f"{n} weight gradient", conv[n]), (f"{n} data gradient", conv[n])]
    return out


def per_launch(path, steps, H, W):
    """Mean time of each conv_gemm_kernel launch of a step over the last `steps` steps of a rocprofv3 kernel trace,
    and the fraction of the fp32 matrix peak it reaches."""
    import csv
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    key = {k.lower(): k for k in rows[0]}
    name, t0, t1 = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    g = sorted((int(r[t0]), int(r[t1]) - int(r[t0]), r[name]) for r in rows if "conv_gemm_kernel" in r[name])
    plan = gemm_launches(H, W)
    assert len(g) % len(plan) == 0 and len(g) >= steps * len(plan), (len(g), len(plan))
    g = g[-steps * len(plan):]
    lines = ["| launch | tile | ms | TFLOP | TFLOP/s | of 157.3 TF |", "|---|---|---|---|---|---|"]
    for i, (what, flop) in enumerate(plan):
        mine = g[i::len(plan)]
        ns = sum(d for _, d, _ in mine) / len(mine)
        tile = "128" if "<2, 2>" in mine[0][2] else "64"
        tf = flop / (ns * 1e-9) / 1e12
        lines.append(f"| {what} | {tile} | {ns / 1e6:.3f} | {flop / 1e12:.4f} | {tf:.1f} | {100 * tf / PEAK_TF:.0f} % |")
    return "\n".join(lines)


def document(times, stats, trace, steps):
    H, W = GEOMETRIES[0]
    return f"""# largecnn train step: libabd against PyTorch-ROCm's eager step (one MI355X, one process)

Written by `scripts/ab_largecnn.py` (its docstring has the commands).  A is `abd_largecnn_train_step` (forward,
cross entropy, backward, Adam in one C-ABI call), B is PyTorch-ROCm's eager step of the same network from `torch.nn`
layers (autograd, `torch.optim.Adam`), same weights and data, fp32.  The two alternate in warmed blocks timed with
HIP events.  Where the ratio torch / abd is below 1, libabd is the slower one.

```
{times.strip()}
```

## Kernels of one libabd step at B = {B}, ({H}, {W})

One profiler run of {steps} steps after {WARM} of warm-up (`rocprofv3 --kernel-trace --stats`, no counters in that
run); all {steps + WARM} steps are counted in this table.

{shares(stats, steps + WARM, H, W)}

## Each conv_gemm_kernel launch of a step, in launch order

Mean over the last {steps} steps of the same run's kernel trace; FLOP from the launch's shape (2 M N K; a conv's
forward, data gradient and weight gradient are the same count).

{per_launch(trace, steps, H, W)}
"""


def setup(H, W, dev):
    torch.manual_seed(0)
    m = largecnn(K, linear_features(H, W)).to(dev).train()
    ref = Eager(K, linear_features(H, W))
    ref.load_state_dict(m.state_dict())
    ref.to(dev).train()
    r = np.random.Generator(np.random.PCG64(1))
    x = torch.tensor(r.normal(size=(B, 1, H, W)).astype(np.float32), device=dev)
    y = torch.tensor(r.integers(0, K, B), device=dev)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    eng = m.engine(x)
    adam = T.AdamBinding(m, opt)
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    crit = nn.CrossEntropyLoss()

    def step_a():
        T.largecnn_train_step(m, x, y, None, adam, None)

    def step_b():
        ropt.zero_grad(set_to_none=True)
        crit(ref(x), y).backward()
        ropt.step()

    return eng, step_a, step_b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=0, help="run only N libabd steps at (100, 40) (for a profiler)")
    ap.add_argument("--shares", default=None, help="a rocprofv3 kernel_stats.csv to summarise")
    ap.add_argument("--trace", default=None, help="the same run's kernel_trace.csv")
    ap.add_argument("--times", default=None, help="the text of a timing run (--out of a run without --profile)")
    a = ap.parse_args()
    if a.shares and a.trace and a.times:
        with open(a.times) as f:
            text = document(f.read(), a.shares, a.trace, a.profile or 3)
    elif a.shares:
        text = shares(a.shares, (a.profile or 3) + WARM, *GEOMETRIES[0])
    else:
        abd_amd.load_library()
        dev = torch.device("cuda", 0)
        if a.profile:
            _, step_a, _ = setup(*GEOMETRIES[0], dev)
            for _ in range(WARM + a.profile):
                step_a()
            torch.cuda.synchronize()
            return
        lines = []
        for H, W in GEOMETRIES:
            eng, step_a, step_b = setup(H, W, dev)
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
            ws = abd_amd.load_library().abd_largecnn_workspace_bytes(eng.h, B)
            lines.append(f"largecnn train step, B={B} ({H}, {W}) K={K}, {a.blocks} alternating blocks of {a.steps} "
                         f"steps, workspace {ws} bytes ({ws / 2**30:.2f} GiB)")
            for name, v in times.items():
                med = statistics.median(v)
                lines.append(f"  {name}: median {med:.3f} ms/step (min {min(v):.3f}, max {max(v):.3f}), "
                             f"{B / med * 1e3:.0f} utterances/s")
            lines.append(f"  ratio torch / abd: "
                         f"{statistics.median(times['torch']) / statistics.median(times['abd']):.2f}")
            del eng, step_a, step_b
            torch.cuda.empty_cache()
        text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
