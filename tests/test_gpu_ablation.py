"""GPU: the batched neuron-ablation sweep (abd_smallcnn_ablate_eval, torch.ops.abd.smallcnn_ablate_eval,
abd_amd.defense) against the float64 oracle on PATCHED parameters and the reference-pinned fixture
tests/golden/ablation_golden.npz -- never against the library's own eval.

Tolerance: the project's fp32 parity bound RTOL = 1e-4 (relative, per-variant mean loss); a loss
CHANGE is a difference of two such losses, so it is held to RTOL x |baseline loss| absolute.
Correct counts are exact: every case's seed was chosen on the CPU so that every (variant, row) has
a top-2 log-prob margin above 1e-3 (asserted on the oracle side first; no row is excluded).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D, models as M, training as T
from ablation_cases import (FIXTURE, SEEDS, case_inputs, ce_rows, fixture_variants, general_masks, oracle_case,
                            single_masks, top2_margin, OracleSweep)

pytestmark = pytest.mark.gpu
RTOL = 1e-4
GUARD = 8 << 20
PAT = 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ablation_golden.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    from abd_amd import ops  # noqa: F401
    return torch.device("cuda", 0)


def flat_state(st, dev):
    params = torch.cat([torch.tensor(st[k]).reshape(-1) for k in M.PARAM_ORDER]).to(dev)
    running = torch.cat([torch.tensor(st[f"{bn}.{s}"]) for bn, _ in M.RUNNING_ORDER
                         for s in ("running_mean", "running_var")]).to(dev)
    return params, running


def sweep(dev, st, x, y, masks, kind, vpp, prec, K, out=None):
    """One op call on one batch -> (loss_sum (V) float64, correct (V) int64) numpy."""
    params, running = flat_state(st, dev)
    V = len(masks)
    ls, co = out if out is not None else (torch.zeros(V, dtype=torch.float64, device=dev),
                                          torch.zeros(V, dtype=torch.int64, device=dev))
    torch.ops.abd.smallcnn_ablate_eval(torch.tensor(x, device=dev), params, running, torch.tensor(y, device=dev),
                                       torch.tensor(masks), L.ABLATE_KINDS[kind], vpp, ls, co, K, prec)
    torch.cuda.synchronize()
    return ls.cpu().numpy(), co.cpu().numpy()


@functools.lru_cache(maxsize=None)
def oracle_singles(H, W, K, B, kind):
    st, x, y = case_inputs(H, W, K, B, SEEDS[(H, W, K, B)])
    loss, pred, margin = oracle_case(st, x, y, single_masks(), kind)
    return st, x, y, loss, pred, margin


# ------------------------------------------------------------------ 1. fixture parity, 32 x 13
@pytest.mark.parametrize("prec", ["f32", "f32split"])
def test_fixture_parity(dev, prec):
    g = np.load(GOLDEN)
    c = FIXTURE
    assert list(g["case"]) == [c["H"], c["W"], c["K"], c["B"], c["seed"]]
    st, x, y = case_inputs(c["H"], c["W"], c["K"], c["B"], c["seed"])
    masks, kinds = g["masks"], g["kinds"]
    assert np.array_equal(masks, fixture_variants()[0])
    empty = np.zeros((1, 160), np.uint8)
    for kd, name in ((0, "conv"), (1, "bn")):
        sel = np.nonzero(kinds == kd)[0]
        ls, co = sweep(dev, st, x, y, np.concatenate([empty, masks[sel]]), name, 7, prec, c["K"])
        loss = ls / c["B"]
        print(f"{prec} {name}: baseline {loss[0]:.7f} (golden {float(g['base_loss']):.7f}), max rel err "
              f"{np.abs(loss[1:] / g['loss'][sel] - 1).max():.2e}, max loss-change err "
              f"{np.abs((loss[1:] - loss[0]) - (g['loss'][sel] - g['base_loss'])).max():.2e}")
        np.testing.assert_allclose(loss[0], g["base_loss"], rtol=RTOL)
        np.testing.assert_allclose(loss[1:], g["loss"][sel], rtol=RTOL)
        np.testing.assert_allclose(loss[1:] - loss[0], g["loss"][sel] - g["base_loss"], rtol=0,
                                   atol=RTOL * abs(float(g["base_loss"])))
        assert float(g["min_margin"]) > 1e-3
        assert np.array_equal(co[1:], (g["pred"][sel] == y[None]).sum(1))
        assert co[0] == (g["base_pred"] == y).sum()


# ------------------------------------------------------------------ 2. shapes + 5. accuracy
SHAPES = [(32, 40, 10), (101, 40, 35)]


@functools.lru_cache(maxsize=None)
def device_singles(H, W, K, B, kind, prec):
    st, x, y, _, _, _ = oracle_singles(H, W, K, B, kind)
    return sweep(torch.device("cuda", 0), st, x, y, single_masks(), kind, 7, prec, K)   # 22 passes + a tail of 6


@pytest.mark.parametrize("prec", ["f32", "f32split"])
@pytest.mark.parametrize("kind", ["conv", "bn"])
@pytest.mark.parametrize("B", [5, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_single_filter_losses(dev, shape, B, kind, prec):
    H, W, K = shape
    _, _, _, loss, _, _ = oracle_singles(H, W, K, B, kind)
    ls, _ = device_singles(H, W, K, B, kind, prec)
    ref = loss.sum(1)
    print(f"{shape} B={B} {kind} {prec}: max rel err {np.abs(ls / ref - 1).max():.2e}")
    np.testing.assert_allclose(ls / B, ref / B, rtol=RTOL)


@pytest.mark.parametrize("prec", ["f32", "f32split"])
@pytest.mark.parametrize("kind", ["conv", "bn"])
@pytest.mark.parametrize("B", [5, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_single_filter_accuracy(dev, shape, B, kind, prec):
    H, W, K = shape
    _, _, y, _, pred, margin = oracle_singles(H, W, K, B, kind)
    assert margin > 1e-3, f"case seed leaves a top-2 margin of {margin:.2e}"
    _, co = device_singles(H, W, K, B, kind, prec)
    assert np.array_equal(co, (pred == y[None]).sum(1))


# ------------------------------------------------------------------ 3. general masks
@pytest.mark.parametrize("prec", ["f32", "f32split"])
@pytest.mark.parametrize("kind", ["conv", "bn"])
def test_general_masks(dev, kind, prec):
    H, W, K, B = 32, 40, 10, 5
    st, x, y = case_inputs(H, W, K, B, SEEDS[(H, W, K, B)])
    masks = general_masks()
    loss, pred, margin = oracle_case(st, x, y, masks, kind)
    assert margin > 1e-3
    for vpp in (2, 5):   # mixed classes inside a pass and a tail of 1; everything in one pass
        ls, co = sweep(dev, st, x, y, masks, kind, vpp, prec, K)
        print(f"{kind} {prec} vpp={vpp}: rel err {np.abs(ls / loss.sum(1) - 1)}")
        np.testing.assert_allclose(ls / B, loss.sum(1) / B, rtol=RTOL)
        assert np.array_equal(co, (pred == y[None]).sum(1))


# ------------------------------------------------------------------ 4. accumulation
def test_two_calls_accumulate(dev):
    H, W, K = 32, 40, 10
    st, x, y = case_inputs(H, W, K, 8, SEEDS[(H, W, K, 5)])
    masks = np.concatenate([general_masks(), single_masks()[[1, 70, 150]]])
    out = (torch.zeros(len(masks), dtype=torch.float64, device=dev), torch.zeros(len(masks), dtype=torch.int64, device=dev))
    ref_l, ref_c = np.zeros(len(masks)), np.zeros(len(masks), np.int64)
    for s, e in ((0, 5), (5, 8)):
        ls, co = sweep(dev, st, x[s:e], y[s:e], masks, "conv", 3, "f32split", K, out=out)
        loss, pred, margin = oracle_case(st, x[s:e], y[s:e], masks, "conv")
        assert margin > 1e-3
        ref_l += loss.sum(1)
        ref_c += (pred == y[None, s:e]).sum(1)
    np.testing.assert_allclose(ls / 8, ref_l / 8, rtol=RTOL)
    assert np.array_equal(co, ref_c)
    # nothing to do: nothing launched, nothing changed
    sweep(dev, st, x[:0], y[:0], masks, "conv", 3, "f32split", K, out=out)
    sweep(dev, st, x[:5], y[:5], masks[:0], "conv", 3, "f32split", K, out=out)
    assert np.array_equal(out[0].cpu().numpy(), ls) and np.array_equal(out[1].cpu().numpy(), co)


# ------------------------------------------------------------------ 6. guards
@pytest.mark.parametrize("prec", ["f32", "f32split"])
@pytest.mark.parametrize("shape", [(100, 40, 35, 5), (32, 13, 10, 6)])
def test_stays_inside_workspace_and_outputs(dev, shape, prec):
    H, W, K, B = shape
    st, x, y = case_inputs(H, W, K, B, 3)
    params, running = flat_state(st, dev)
    lib = L.lib()
    h = C.c_void_p()
    L.check(lib.abd_smallcnn_create(H, W, K, 0, C.byref(h)), "create")
    L.check(lib.abd_smallcnn_set_precision(h, L.PRECISIONS[prec]), "precision")
    masks = np.ascontiguousarray(np.concatenate([general_masks(), single_masks()[::9]]))
    V, vpp = len(masks), 4
    need = lib.abd_smallcnn_ablate_workspace_bytes(h, B, vpp)
    assert need > 0
    ws = torch.full((need + GUARD,), PAT, dtype=torch.uint8, device=dev)
    ls = torch.full((V + 4,), -7.0, dtype=torch.float64, device=dev)
    co = torch.full((V + 4,), -7, dtype=torch.int64, device=dev)
    ls[:V] = 0
    co[:V] = 0
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)

    def call(vpp_, nbytes):
        return lib.abd_smallcnn_ablate_eval(h, xd.data_ptr(), B, params.data_ptr(), running.data_ptr(), yd.data_ptr(),
                                            masks.ctypes.data, V, 0, vpp_, ls.data_ptr(), co.data_ptr(), ws.data_ptr(),
                                            nbytes, L.stream_ptr(dev))
    try:
        assert call(vpp, need) == 0, lib.abd_last_error()
        torch.cuda.synchronize()
        bad = int((ws[need:] != PAT).sum().item())
        assert bad == 0, f"{bad} guard bytes written past the {need}-byte workspace"
        assert bool((ls[V:] == -7.0).all()) and bool((co[V:] == -7).all())
        assert bool((ls[:V] > 0).all()) and bool((co[:V] >= 0).all()) and bool((co[:V] <= B).all())
        before = (ls.clone(), co.clone())
        assert call(vpp, need - 1) == 1003 and b"workspace" in lib.abd_last_error()      # ABD_E_WORKSPACE
        assert call(1 << 24, need) == 1001 and b"int32" in lib.abd_last_error()          # ABD_E_INVALID
        assert call(0, need) == 1001
        torch.cuda.synchronize()
        assert torch.equal(ls, before[0]) and torch.equal(co, before[1])
    finally:
        lib.abd_smallcnn_destroy(h)


# ------------------------------------------------------------------ 7. opcheck
def test_opcheck_ablate_eval(dev):
    H, W, K, B = 32, 13, 10, 4
    st, x, y = case_inputs(H, W, K, B, 3)
    params, running = flat_state(st, dev)
    masks = torch.tensor(general_masks())
    ls = torch.zeros(5, dtype=torch.float64, device=dev)
    co = torch.zeros(5, dtype=torch.int64, device=dev)
    torch.library.opcheck(torch.ops.abd.smallcnn_ablate_eval.default,
                          (torch.tensor(x, device=dev), params, running, torch.tensor(y, device=dev), masks, 0, 2, ls,
                           co, K))
    with pytest.raises(L.AbdError):
        torch.ops.abd.smallcnn_ablate_eval(torch.tensor(x), params, running, torch.tensor(y, device=dev), masks, 0, 2,
                                           ls, co, K)


# ------------------------------------------------------------------ 8. defense API on a loaded checkpoint
def test_neuron_loss_change_on_loaded_checkpoint(dev, tmp_path):
    from conftest import load_dropin_checkpoint
    H, W, K, N = 32, 13, 10, 11
    st, x, y = case_inputs(H, W, K, N, 6)
    m = M.smallcnn(K, st["fc1.weight"].shape[1])
    m.load_state_dict({k: torch.tensor(v) for k, v in st.items()})
    path = str(tmp_path / "checkpoint.pt")
    T.save_reference_checkpoint(m.eval(), path)
    ck = load_dropin_checkpoint(path, map_location=dev)
    ck.train()   # the scan must not depend on, or change, the module's mode
    before = {k: v.detach().clone() for k, v in ck.state_dict().items()}
    xd, yd = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    bs = 4   # batches of 4, 4, 3: temp_test's mean of batch means with a short last batch
    sw = [(OracleSweep(st, x[s:e]), y[s:e]) for s, e in D.batch_bounds(N, bs)]

    def ref_loss(mask, kind):
        return float(np.mean([ce_rows(o.logp(mask, kind), yy).mean() for o, yy in sw]))
    for kind in ("conv", "bn"):
        names, change = D.neuron_loss_change(ck, xd, yd, layer_type=kind, batch_size=bs)
        assert names == D.neuron_names(None, kind) and names[64] == f"{kind}2.weight.0"
        base = ref_loss(np.zeros(160, np.uint8), kind)
        ref = np.array([ref_loss(mk, kind) - base for mk in single_masks()])
        print(f"{kind}: max loss-change err {np.abs(change - ref).max():.2e} (baseline {base:.5f})")
        np.testing.assert_allclose(change, ref, rtol=0, atol=RTOL * abs(base))
    after = ck.state_dict()
    assert ck.training and sorted(after) == sorted(before)
    for k in before:
        assert torch.equal(after[k], before[k]), k
    # the pruning ratio scan is the same sweep with growing masks
    ranked = [names[i] for i in np.argsort(-change)]
    loss, acc = D.pruned_eval(ck, xd, yd, ranked, [0.0, 0.05, 0.5], batch_size=bs)
    for r, lv in zip((0.0, 0.05, 0.5), loss):
        mk = D.pack_masks([ranked[:int(r * len(ranked))]])[0].numpy()[0]
        np.testing.assert_allclose(lv, ref_loss(mk, "bn"), rtol=RTOL)
    assert ((acc >= 0) & (acc <= 1)).all()
    with pytest.raises(L.AbdError):
        D.ablation_sweep(ck, torch.tensor(x), yd, np.zeros((1, 160), np.uint8))
