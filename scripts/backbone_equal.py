#!/usr/bin/env python3
"""Byte equality of two libabd builds on the five flat-buffer backbones (RNN, largecnn, ResNet, lstmwithattention,
smalllstm).

    ABD_LIB=/path/libabd_parent.so timeout -k 10 120 python scripts/backbone_equal.py dump out/parent.npz
    ABD_LIB=/path/libabd.so        timeout -k 10 120 python scripts/backbone_equal.py dump out/new.npz
    python scripts/backbone_equal.py compare out/parent.npz out/new.npz

`dump` is one fresh process per library: from fixed seeds it runs the cases below and writes every output and every
mutated tensor (logits, metrics, parameters, gradients, Adam moments, running statistics, num_batches_tracked,
generated dropout masks) to the .npz.  `compare` checks two such files byte for byte and prints arrays, bytes and
differences; it exits 1 on any difference.

    RNN               eval forward, autograd forward + backward, two Adam train steps: `ragged_tiles` of
                      tests/rnn_cases.py, and B = 16, T = 32, F = 13 (M = 512 rows against N = 3072: exactly the 96
                      blocks at which the 128 tile is chosen, and two weight-gradient slices)
    largecnn          every case of tests/largecnn_cases.py at the default tile threshold and with
                      abd_largecnn_set_large_min_blocks(1): eval forward, an Adam step with given masks, a step
                      whose generated masks are written out
    ResNet            every case of tests/resnet_cases.py: eval forward, two Adam train steps
    lstmwithattention `tiny` and `ragged_tiles` of tests/lstm_attention_cases.py: eval forward, two Adam train steps
    smalllstm         every case of tests/smalllstm_cases.py: eval forward, an Adam step with the case's mask, a step
                      whose generated mask is written out under a fixed seed, eval forward on the updated running
                      statistics; the running statistics and num_batches_tracked after each step
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def dump(path):
    import torch

    import abd_amd  # noqa: F401
    from abd_amd import _lib as L, training as T
    from abd_amd.models_largecnn import largecnn
    from abd_amd.models_lstm import lstmwithattention
    from abd_amd.models_resnet import ResNet, ResidualBlock
    from abd_amd.models_rnn import RNN
    from abd_amd.models_smalllstm import smalllstm
    import largecnn_cases as lc
    import lstm_attention_cases as ac
    import resnet_cases as rc
    import rnn_cases as nc
    import smalllstm_cases as sc

    dev = torch.device("cuda")
    rec = {}

    def put(key, t):
        assert key not in rec, key
        rec[key] = t.detach().cpu().numpy().copy()

    def dev_t(*arrays):
        return [torch.tensor(a, device=dev) for a in arrays]

    def load(m, state):
        m.load_state_dict({k: torch.tensor(v) for k, v in state.items()})
        return m.to(dev)

    def engine_state(tag, m, names=("params", "grads", "exp_avg", "exp_avg_sq", "running", "nbt")):
        eng = m._engine
        for n in names:
            if getattr(eng, n, None) is not None:
                put(f"{tag}/{n}", getattr(eng, n))

    def steps(tag, m, x, y, ind, step, n=2):
        """n Adam steps through `step(adam, metrics, logits_out)`: the outputs and gradients of each, the whole
        engine state after the last."""
        adam = T.AdamBinding(m, torch.optim.Adam(m.parameters(), lr=1e-3))
        for i in range(n):
            mt = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
            lo = torch.zeros((x.shape[0], m._engine.K), dtype=torch.float32, device=dev)
            step(adam, mt, lo)
            put(f"{tag}/step{i}/logits", lo)
            put(f"{tag}/step{i}/metrics", mt)
            engine_state(f"{tag}/step{i}", m, ("grads",) if i < n - 1 else ())
        engine_state(f"{tag}/final", m)

    def eval_forward(tag, m, x):
        m.eval()
        with torch.no_grad():
            put(f"{tag}/eval", m(x))
        m.train()

    # ---------------------------------------------------------------- RNN
    nc.CASES["tile_threshold"] = (16, 32, 13, 10, 9)
    for name in ("ragged_tiles", "tile_threshold"):
        B, Tn, Fd, K, _ = nc.CASES[name]
        m = load(RNN(K, Fd), nc.make_state(name))
        x, y, ind = dev_t(*nc.make_inputs(name))
        tag = f"rnn/{name}"
        eval_forward(tag, m, x)
        out = m(x)
        g = torch.Generator().manual_seed(11)
        out.backward(torch.randn(out.shape, generator=g).to(dev))
        put(f"{tag}/train_logits", out)
        engine_state(f"{tag}/backward", m, ("grads",))
        steps(tag, m, x, y, ind, lambda adam, mt, lo: T.rnn_train_step(m, x, y, ind, adam, mt, logits_out=lo))
        del m
    # ---------------------------------------------------------------- largecnn
    for name, (B, H, W, K, _) in lc.CASES.items():
        for min_blocks in (None, 1):
            m = load(largecnn(K, lc.linear_features(H, W)), lc.make_state(name))
            x, y, ind, m1, m2 = dev_t(*lc.make_inputs(name))
            tag = f"largecnn/{name}/{'default' if min_blocks is None else 'large_tile'}"
            eng = m.engine(x)
            if min_blocks is not None:
                eng.call("set_large_min_blocks", min_blocks)
            eval_forward(tag, m, x)
            steps(tag, m, x, y, ind, lambda adam, mt, lo: T.largecnn_train_step(
                m, x, y, ind, adam, mt, masks=(m1, m2), logits_out=lo), n=1)
            mo = (torch.zeros_like(m1), torch.zeros_like(m2))
            lo = torch.zeros((B, K), dtype=torch.float32, device=dev)
            T.largecnn_train_step(m, x, y, ind, None, None, masks_out=mo, do_update=False, seed=77, logits_out=lo)
            put(f"{tag}/hash/logits", lo)
            put(f"{tag}/hash/mask1", mo[0])
            put(f"{tag}/hash/mask2", mo[1])
            engine_state(f"{tag}/hash", m, ("grads",))
            del m
    # ---------------------------------------------------------------- ResNet
    for name, (B, H, W, K, _) in rc.CASES.items():
        m = load(ResNet(ResidualBlock, [2, 2, 2], K, rc.linear_features(H, W)), rc.make_state(name))
        x, y, ind = dev_t(*rc.make_inputs(name))
        tag = f"resnet/{name}"
        eval_forward(tag, m, x)
        steps(tag, m, x, y, ind, lambda adam, mt, lo: T.resnet_train_step(m, x, y, ind, adam, mt, logits_out=lo))
        eval_forward(f"{tag}/after", m, x)
        del m
    # ---------------------------------------------------------------- lstmwithattention
    for name in ("tiny", "ragged_tiles"):
        B, Tn, Fd, K, _ = ac.geometry(name)
        m = load(lstmwithattention(K, Fd, Tn), ac.make_state(name))
        x, y, ind, mask = dev_t(*ac.make_inputs(name))
        tag = f"lstm/{name}"
        eval_forward(tag, m, x)
        steps(tag, m, x, y, ind, lambda adam, mt, lo: T.lstm_train_step(m, x, y, ind, adam, mt, mask=mask,
                                                                        logits_out=lo))
        del m
    # ---------------------------------------------------------------- smalllstm
    for name, (B, H, W, K, _) in sc.CASES.items():
        m = load(smalllstm(K, sc.rnn_features(H, W)), sc.make_state(name))
        x, y, ind, mask = dev_t(*sc.make_inputs(name))
        tag = f"smalllstm/{name}"
        eval_forward(tag, m, x)
        steps(tag, m, x, y, ind, lambda adam, mt, lo: T.smalllstm_train_step(m, x, y, ind, adam, mt, mask=mask,
                                                                             logits_out=lo), n=1)
        mo = torch.zeros_like(mask)
        lo = torch.zeros((B, K), dtype=torch.float32, device=dev)
        T.smalllstm_train_step(m, x, y, ind, None, None, mask_out=mo, do_update=False, seed=77, logits_out=lo)
        put(f"{tag}/hash/logits", lo)
        put(f"{tag}/hash/mask", mo)
        engine_state(f"{tag}/hash", m, ("grads", "running", "nbt"))
        eval_forward(f"{tag}/after", m, x)
        del m
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **rec)
    print(f"{L.LIB_PATH}: {len(rec)} arrays, {sum(a.nbytes for a in rec.values())} bytes -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    if sorted(a.files) != sorted(b.files):
        print(f"different arrays: {sorted(set(a.files) ^ set(b.files))}")
        return 1
    total = bad = 0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        total += x.nbytes
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad += 1
            n = int((x.view(np.uint8) != y.view(np.uint8)).sum()) if x.shape == y.shape and x.dtype == y.dtype else -1
            print(f"DIFFERS {k}: {x.dtype}{x.shape} vs {y.dtype}{y.shape}, {n} bytes")
    print(f"{len(a.files)} arrays, {total} bytes compared byte for byte, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
