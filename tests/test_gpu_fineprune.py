"""GPU: Fine-Pruning on the device (csrc/fineprune.hip, torch.ops.abd.smallcnn_hidden_sums / smallcnn_fcprune_eval /
smallcnn_pruned_finetune_step, abd_amd.defense.hidden_activation / fc_prune_sweep / fine_prune).

1. hidden sums: against the double column sum of the device's own d2 buffer (1e-12 relative), against the
   float64 restatement (fineprune_cases.hidden, RTOL = 1e-4 of the batch's largest activation), accumulation
2. the prune sweep: loss sums within RTOL per row of the restatement and of abd_smallcnn_eval on parameters with
   the variant's fc2.weight columns zeroed, correct counts exact; 1, 2 and one more variant than a pass holds,
   with the empty, the all-pruned and non-nested masks
3. the masked fine-tuning step: bit-equal over three steps to the step composed from the entry points that
   existed before it; log-probs and loss against the restatement with the golden's masks
4. defense.fine_prune against the reference's own run (tests/golden/fineprune_golden.npz)
Exact correct counts rest on the top-2 log-prob margin of the float64 restatement, asserted before the
comparison (above 1e-3, ten times RTOL of the largest log-prob magnitudes in play): a float32 result within
RTOL cannot change the arg-max.  Set ABD_PARITY_OUT to a file name to have the observed figures appended to it.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D, models as M, training as T
from golden_inputs import rng
from oracle import smallcnn as oc
import fineprune_cases as fc

pytestmark = pytest.mark.gpu
RTOL = 1e-4
MARGIN = 1e-3
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
SHAPES = [(32, 13, 10, 16), (32, 13, 10, 5), (32, 40, 35, 16), (32, 40, 35, 5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    from abd_amd import ops  # noqa: F401
    return torch.device("cuda", 0)


def note(line):
    print(line)
    out = os.environ.get("ABD_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def case(H, W, K, B, seed):
    """A test case whose logits spread over several units (fc2 scaled up, distinct biases 0.1 apart), so that
    arg-max margins are wide -- with every unit pruned the logits are the bias alone."""
    st, x, y = fc.case_inputs(H, W, K, B, seed)
    st["fc2.weight"] = (st["fc2.weight"] * 24.0).astype(np.float32)
    st["fc2.bias"] = (0.1 * rng(seed).permutation(K) - 0.05 * K).astype(np.float32)
    return st, x, y


def build(st, K, dev, prec="f32split"):
    m = M.smallcnn(K, st["fc1.weight"].shape[1])
    sd = {k: torch.tensor(v) for k, v in st.items()}
    for i in (1, 2, 3):                                                    # the golden's states carry no counters
        sd.setdefault(f"bn{i}.num_batches_tracked", torch.tensor(0))
    m.load_state_dict(sd)
    return m.to(dev).set_gemm_precision(prec).train()


def flat_state(st, dev):
    params = torch.cat([torch.tensor(st[k]).reshape(-1) for k in M.PARAM_ORDER]).to(dev)
    running = torch.cat([torch.tensor(st[f"{bn}.{s}"]) for bn, _ in M.RUNNING_ORDER
                         for s in ("running_mean", "running_var")]).to(dev)
    return params, running


def variant_masks(seed, V):
    """(V, 128) uint8: the empty mask, the all-pruned mask, then masks that are not nested in one another, from
    a few units to nearly all."""
    r = rng(seed)
    masks = np.zeros((V, 128), np.uint8)
    if V > 1:
        masks[1] = 1
    for v in range(2, V):
        masks[v] = r.random(128) < r.uniform(0.02, 0.98)
    return masks


# ------------------------------------------------------------------ 1. hidden sums
@pytest.mark.parametrize("prec", ["f32split", "f32"])
@pytest.mark.parametrize("H,W,K,B", SHAPES)
def test_hidden_sums(dev, H, W, K, B, prec):
    from abd_amd import ops
    st, x, _ = case(H, W, K, B, seed=300 + B + K)
    xd = torch.tensor(x, device=dev)
    params, running = flat_state(st, dev)
    h = ops._net(H, W, K, prec)
    lib = L.lib()
    need = lib.abd_smallcnn_workspace_bytes(h, B)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    sums = torch.zeros(128, dtype=torch.float64, device=dev)
    for i in range(2):
        L.check(lib.abd_smallcnn_hidden_sums(h, xd.data_ptr(), B, params.data_ptr(), running.data_ptr(), sums.data_ptr(),
                                             ws.data_ptr(), ws.numel(), L.stream_ptr(dev)), "abd_smallcnn_hidden_sums")
        if i == 0:
            once = sums.clone()
    torch.cuda.synchronize()
    off = lib.abd_smallcnn_workspace_offset(h, B, b"d2")
    d2 = ws[off:off + B * 128 * 4].view(torch.float32).reshape(B, 128).cpu().numpy()
    own = d2.astype(np.float64).sum(0)
    got = once.cpu().numpy()
    assert np.abs(got - own).max() <= 1e-12 * np.abs(own).max()
    assert torch.equal(sums, once + once)                                 # accumulates over calls
    ref = fc.hidden(oc.SmallCNN(st), x)
    err = np.abs(got - ref.sum(0)).max() / ref.max()
    note(f"| hidden_sums {H}x{W} K={K} B={B} {prec} | {err:.2e} |")
    assert (ref > 0).any() and err <= RTOL
    assert np.abs(d2 - ref).max() <= RTOL * ref.max()
    # the op, and the defense function with the reference's first-batch-only divisor
    s2 = torch.zeros(128, dtype=torch.float64, device=dev)
    torch.ops.abd.smallcnn_hidden_sums(xd, params, running, s2, K, prec)
    assert torch.equal(s2, once)
    if B == 16 and prec == "f32split":
        m = build(st, K, dev)
        both = torch.cat([xd, xd.flip(0)])
        act = D.hidden_activation(m, both, batch_size=B)
        assert act.dtype == torch.float32 and not act.is_cuda
        assert torch.equal(act, (once / 32.0).to(torch.float32).cpu())
        full = D.hidden_activation(m, both, batch_size=B, first_batch_only=False)
        np.testing.assert_allclose(full.numpy(), 2 * got / 32.0, rtol=1e-6)
        perm = np.arange(32)[::-1].copy()
        np.testing.assert_allclose(D.hidden_activation(m, both, batch_size=B, order=perm).numpy(), act.numpy(), rtol=1e-6)


# ------------------------------------------------------------------ 2. prune sweep
@pytest.mark.parametrize("prec", ["f32split", "f32"])
@pytest.mark.parametrize("V", [1, 2, L.FCPRUNE_PASS_VARIANTS + 1])
@pytest.mark.parametrize("H,W,K,B", SHAPES)
def test_fcprune_eval(dev, H, W, K, B, V, prec):
    # the seed whose inputs keep every (variant, row) margin of the restatement above MARGIN (asserted below)
    st, x, y = case(H, W, K, B, seed={(32, 13, 10, 16): 526}.get((H, W, K, B), 400 + B + K))
    masks = variant_masks(410 + V, V)
    m64 = oc.SmallCNN(st)
    ref_sum, ref_hit, margin = fc.sweep_batch(m64, x, y, masks)
    assert margin > MARGIN, f"test input: top-2 margin {margin:.2e}"
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    params, running = flat_state(st, dev)
    loss = torch.zeros(V, dtype=torch.float64, device=dev)
    hit = torch.zeros(V, dtype=torch.int64, device=dev)
    torch.ops.abd.smallcnn_fcprune_eval(xd, params, running, yd, torch.from_numpy(masks), loss, hit, K, prec)
    got, hits = loss.cpu().numpy(), hit.cpu().numpy()
    err = np.abs(got - ref_sum).max() / B
    assert err <= RTOL and np.array_equal(hits, ref_hit)
    if V > 1:
        # all units pruned: the logits are the bias
        out = oc.log_softmax(np.tile(st["fc2.bias"].astype(np.float64), (B, 1)))
        assert abs(got[1] - fc.row_losses(out, y).sum()) <= 1e-5 * B
    # per-variant abd_smallcnn_eval on parameters with the variant's columns zeroed
    w_off = D.param_offsets(M.smallcnn(K, st["fc1.weight"].shape[1]))[14]
    worst = 0.0
    for v in range(V):
        pv = params.clone()
        pv[w_off:w_off + K * 128].view(K, 128)[:, torch.from_numpy(masks[v] != 0).to(dev)] = 0.0
        metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
        torch.ops.abd.smallcnn_eval_metrics(xd, pv, running, K, prec, yd, None, metrics)
        mean, total, correct, _, _, _ = T.read_metrics(metrics)
        worst = max(worst, abs(got[v] / B - mean))
        assert total == B and correct == hits[v], v
        if v == 0:
            plain = mean                                                   # the empty mask is the plain eval
    assert worst <= RTOL and abs(got[0] / B - plain) <= RTOL
    note(f"| fcprune_eval {H}x{W} K={K} B={B} V={V} {prec} | {err:.2e} | {worst:.2e} | {margin:.2e} |")
    # accumulation over calls, and nothing launched for an empty batch / no variant
    torch.ops.abd.smallcnn_fcprune_eval(xd, params, running, yd, torch.from_numpy(masks), loss, hit, K, prec)
    torch.ops.abd.smallcnn_fcprune_eval(xd[:0], params, running, yd[:0], torch.from_numpy(masks), loss, hit, K, prec)
    torch.ops.abd.smallcnn_fcprune_eval(xd, params, running, yd, torch.from_numpy(masks[:0]), loss, hit, K, prec)
    assert torch.equal(hit.cpu(), torch.from_numpy(2 * hits)) and np.array_equal(loss.cpu().numpy(), got + got)


def test_fcprune_eval_bf16_equals_per_variant_eval(dev):
    """bf16: the public eval supports it unchanged, so the sweep does too; fc2 and the loss are fp32 in both."""
    H, W, K, B, V = 32, 13, 10, 16, 5
    st, x, y = case(H, W, K, B, seed=430)
    masks = variant_masks(431, V)
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    params, running = flat_state(st, dev)
    loss = torch.zeros(V, dtype=torch.float64, device=dev)
    hit = torch.zeros(V, dtype=torch.int64, device=dev)
    torch.ops.abd.smallcnn_fcprune_eval(xd, params, running, yd, torch.from_numpy(masks), loss, hit, K, "bf16")
    w_off = D.param_offsets(M.smallcnn(K, 224))[14]
    for v in range(V):
        pv = params.clone()
        pv[w_off:w_off + K * 128].view(K, 128)[:, torch.from_numpy(masks[v] != 0).to(dev)] = 0.0
        metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
        torch.ops.abd.smallcnn_eval_metrics(xd, pv, running, K, "bf16", yd, None, metrics)
        mean, _, correct, _, _, _ = T.read_metrics(metrics)
        assert abs(float(loss[v]) / B - mean) <= 1e-6 * max(1.0, mean) and correct == int(hit[v])


def test_fc_prune_sweep_batches_like_temp_test(dev):
    H, W, K, N, B = 32, 13, 10, 21, 16                                   # batches of 16 and 5
    st, x, y = case(H, W, K, N, seed=440)
    masks = variant_masks(441, 4)
    m64 = oc.SmallCNN(st)
    rloss, racc, margin = fc.sweep(m64, x, y, masks, B)
    assert margin > MARGIN
    m = build(st, K, dev)
    loss, acc = D.fc_prune_sweep(m, torch.tensor(x, device=dev), torch.tensor(y, device=dev), masks, batch_size=B)
    assert loss.dtype == torch.float64 and np.array_equal(acc.numpy(), racc)
    np.testing.assert_allclose(loss.numpy(), rloss, rtol=0, atol=RTOL)
    assert m._engine is None                                             # read, never bound or modified
    with pytest.raises(L.AbdError):
        torch.ops.abd.smallcnn_fcprune_eval(torch.tensor(x, device=dev), *flat_state(st, dev), torch.tensor(y, device=dev),
                                            torch.zeros((2, 127), dtype=torch.uint8),
                                            torch.zeros(2, dtype=torch.float64, device=dev),
                                            torch.zeros(2, dtype=torch.int64, device=dev), K)


# ------------------------------------------------------------------ 3. masked fine-tuning step
@pytest.mark.parametrize("prec", ["f32split", "f32", "bf16"])
@pytest.mark.parametrize("H,W,K,B", SHAPES)
def test_pruned_finetune_step_equals_composition(dev, H, W, K, B, prec):
    st, x, y = case(H, W, K, B, seed=500 + B + K)
    flat = st["fc1.weight"].shape[1]
    unit = variant_masks(501, 3)[2]
    pruned = torch.from_numpy(unit).to(dev)
    cols = pruned.ne(0)
    st["fc2.weight"][:, unit != 0] = 0.0                                  # the caller zeroes the columns once
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    ma, mb = build(st, K, dev, prec), build(st, K, dev, prec)
    ea, eb = ma.engine(xd), mb.engine(xd)
    ma_m, ma_v = torch.zeros_like(ea.params), torch.zeros_like(ea.params)
    mb_m, mb_v = torch.zeros_like(eb.params), torch.zeros_like(eb.params)
    meta, metb = (torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev) for _ in range(2))
    w0, w1 = ea.offsets[14], ea.offsets[15]
    r = rng(510 + B)
    p0 = ea.params.clone()
    for step in (1, 2, 3):
        k1 = (r.random((B, flat)) < 0.6).astype(np.uint8)
        k2 = (r.random((B, 128)) < 0.5).astype(np.uint8)
        m1, m2 = torch.tensor(k1, device=dev), torch.tensor(k2, device=dev)
        # the composition: no-update train step, torch zeroes the pruned columns' gradient, abd::adam
        T.train_step(mb, xd, yd, None, None, metb, mask1=m1, mask2=m2, do_update=False)
        eb.grads[w0:w1].view(K, 128)[:, cols] = 0.0
        torch.ops.abd.adam(eb.params, eb.grads, mb_m, mb_v, step, LR, B1, B2, EPS)
        lp = torch.ops.abd.smallcnn_pruned_finetune_step(xd, yd, ea.params, ea.grads, ma_m, ma_v, ea.running, ea.nbt, meta,
                                                         pruned, None, None, K, step, LR, B1, B2, EPS, 5, step, m1, m2, prec)
        torch.cuda.synchronize()
        for what, got, exp in (("params", ea.params, eb.params), ("exp_avg", ma_m, mb_m), ("exp_avg_sq", ma_v, mb_v),
                               ("running", ea.running, eb.running), ("nbt", ea.nbt, eb.nbt), ("metrics", meta, metb),
                               ("grads", ea.grads, eb.grads)):
            assert torch.equal(got, exp), (what, step)
        assert ea.nbt.tolist() == [step] * 3 and lp.shape == (B, K)
        w = ea.params[w0:w1].view(K, 128)
        assert not w[:, cols].any() and not ea.grads[w0:w1].view(K, 128)[:, cols].any()
        assert w[:, ~cols].ne(0).all() and ea.grads[w0:w1].view(K, 128)[:, ~cols].ne(0).any()
    assert not torch.equal(ea.params, p0)


def test_pruned_finetune_step_matches_restatement_on_golden(dev):
    f = fc.load_fixture()
    g, c = f["g"], f["c"]
    st = {k: v.copy() for k, v in f["state"].items()}
    unit = g["unit_mask"]
    tuner = fc.PrunedTuner(f["state"], unit, c["lr_ft"])
    st["fc2.weight"][:, unit != 0] = 0.0
    m = build(st, c["K"], dev)
    pruned = torch.from_numpy(unit).to(dev)
    eng = None
    ea = ev = None
    for step, ((x, y), (k1, k2)) in enumerate(zip(f["ft_batches"], f["ft_masks"]), 1):
        xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
        if eng is None:
            eng = m.engine(xd)
            ea, ev = torch.zeros_like(eng.params), torch.zeros_like(eng.params)
        metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
        m1, m2 = (torch.tensor(k.astype(np.uint8), device=dev) for k in (k1, k2))
        lp = torch.ops.abd.smallcnn_pruned_finetune_step(xd, yd, eng.params, eng.grads, ea, ev, eng.running, eng.nbt,
                                                         metrics, pruned, None, None, c["K"], step, c["lr_ft"], B1, B2,
                                                         EPS, 7, step, m1, m2)
        out, loss, hits = tuner.step(x, y, (k1, k2))
        got = lp.cpu().numpy()
        loss_sum, total, correct, _, _, _ = T.read_metrics(metrics)
        err = np.abs(got - out).max() / np.abs(out).max()
        note(f"| pruned_finetune_step golden batch {step} (B={len(y)}) | {err:.2e} | {abs(loss_sum / loss - 1):.2e} |")
        np.testing.assert_allclose(got, out, rtol=RTOL, atol=RTOL * np.abs(out).max())
        assert abs(loss_sum - loss) <= RTOL * abs(loss) and total == len(y)


# ------------------------------------------------------------------ 4. the whole defense against the reference's run
def test_fine_prune_reproduces_reference_fixture(dev):
    f = fc.load_fixture()
    g, c, d = f["g"], f["c"], f["d"]
    m = build(f["state"], c["K"], dev).eval()
    p_before = D._flat_params(m, dev).clone()
    t = lambda a: torch.tensor(a, device=dev)                             # noqa: E731
    n_val = len(f["val_x"])
    rest = [i for i in range(n_val) if i not in set(g["first_rows"].tolist())]
    val_order = np.concatenate([g["first_rows"], np.array(rest, np.int64)])   # only the first batch counts
    ft_masks = [(t(k1.astype(np.uint8)), t(k2.astype(np.uint8))) for k1, k2 in f["ft_masks"]]
    res = D.fine_prune(m, t(f["val_x"]), t(f["val_y"]), t(d["clean_x"]), t(d["clean_y"]), t(d["bd_x"]), t(d["bd_y"]),
                       t(d["bd_ind"]), once_prune_ratio=c["once_prune_ratio"], acc_ratio=c["acc_ratio"], lr_ft=c["lr_ft"],
                       batch_size=c["B"], val_order=val_order, ft_order=g["ft_rows"], ft_masks=ft_masks)
    ref = g["activation"]
    assert np.abs(res.activation.numpy() - ref).max() <= RTOL * ref.max()
    assert np.array_equal(res.seq_sort, g["seq_sort"])
    assert np.array_equal(np.array(res.pruning_rows), g["pruning_rows"])      # every CSV row, exactly
    assert res.stop_index == int(g["stop_index"]) and res.last_index == int(g["pruning_rows"][-2, 0])
    assert np.array_equal(res.unit_mask.numpy(), g["unit_mask"])
    row, rrow = res.ft_row, g["ft_row"]
    note(f"| fine_prune ft_data | {row} | {tuple(rrow)} |")
    assert row[0] == rrow[0] and row[1] == rrow[1]
    assert abs(row[2] - rrow[2]) <= RTOL * rrow[2] and abs(row[3] - rrow[3]) <= RTOL * rrow[3]
    pruned = torch.from_numpy(g["unit_mask"] != 0)
    w = res.model.fc2.weight.detach().cpu()
    assert not w[:, pruned].any() and w[:, ~pruned].ne(0).all()
    assert torch.equal(res.weight_orig.cpu()[:, pruned], torch.tensor(f["state"]["fc2.weight"])[:, pruned])
    assert torch.equal(res.weight_orig.cpu()[:, ~pruned], w[:, ~pruned])
    assert res.model is not m and torch.equal(D._flat_params(m, dev), p_before)   # the given model is untouched
    assert [int(v) for v in res.model._engine.nbt.tolist()] == [3, 3, 3]
    with pytest.raises(L.AbdError):
        D.pruned_finetune_epoch(res.model, t(f["val_x"]), t(f["val_y"]), torch.optim.SGD(res.model.parameters(), lr=0.01),
                                g["unit_mask"])
