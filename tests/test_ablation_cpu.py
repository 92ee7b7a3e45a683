"""CPU: the neuron-ablation scan's reference chain and host logic.

The fixture tests/golden/ablation_golden.npz holds the reference smallcnn's own numbers on state dicts
patched as ft_reg.py:173-177 does; the float64 oracle on the same patched parameters must reproduce
them, and the tests' cached OracleSweep must equal that oracle.  Then abd_amd.defense's host side:
neuron names, mask packing, temp_test's mean-of-batch-means arithmetic.
"""
import os

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D
from ablation_cases import (FIXTURE, OracleSweep, case_inputs, ce_rows, fixture_variants, patched_state)
from oracle import smallcnn as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ablation_golden.npz")


def test_oracle_reproduces_reference_fixture():
    g = np.load(GOLDEN)
    c = FIXTURE
    assert list(g["case"]) == [c["H"], c["W"], c["K"], c["B"], c["seed"]]
    st, x, y = case_inputs(c["H"], c["W"], c["K"], c["B"], c["seed"])
    masks, kinds = fixture_variants()
    assert np.array_equal(g["masks"], masks) and np.array_equal(g["kinds"], kinds)
    assert len(masks) == 167 and (kinds == 1).sum() == 4 and (masks.sum(1) > 1).sum() == 3
    sw = OracleSweep(st, x)
    base = oc.SmallCNN(st).forward_eval(x)
    np.testing.assert_allclose(ce_rows(base, y).mean(), g["base_loss"], rtol=1e-9)
    assert np.array_equal(base.argmax(1), g["base_pred"])
    for v, (m, kd) in enumerate(zip(masks, kinds)):
        kind = "bn" if kd else "conv"
        lp = oc.SmallCNN(patched_state(st, m, kind)).forward_eval(x)
        np.testing.assert_allclose(ce_rows(lp, y).mean(), g["loss"][v], rtol=1e-9, err_msg=f"variant {v}")
        assert np.array_equal(lp.argmax(1), g["pred"][v]), v
        np.testing.assert_allclose(sw.logp(m, kind), lp, rtol=0, atol=1e-11)   # the GPU tests' cached oracle
    assert np.abs(g["loss"] - g["base_loss"]).max() > 1e-3                      # the variants do differ


def test_neuron_names_order():
    from abd_amd.models import smallcnn
    m = smallcnn(10, 224)
    for lt in ("conv", "bn"):
        names = D.neuron_names(m, lt)
        assert names == D.neuron_names(None, lt) and len(names) == 160
        assert names[0] == f"{lt}1.weight.0" and names[63] == f"{lt}1.weight.63" and names[64] == f"{lt}2.weight.0"
        assert names[128] == f"{lt}3.weight.0" and names[-1] == f"{lt}3.weight.31"
        assert [D.mask_column(n) for n in names] == [(lt, i) for i in range(160)]
    with pytest.raises(SystemError):
        D.neuron_names(m, "linear")


def test_mask_packing():
    masks, kind = D.pack_masks([[], ["conv1.weight.3", "conv2.weight.10", "conv3.weight.5"], ["conv3.weight.31"]])
    assert kind == "conv" and masks.dtype == torch.uint8 and tuple(masks.shape) == (3, L.ABLATE_CHANNELS)
    assert masks[0].sum() == 0 and masks[1].nonzero().flatten().tolist() == [3, 74, 133]
    assert masks[2].nonzero().flatten().tolist() == [159]
    assert D.pack_masks([["bn2.weight.0"]])[1] == "bn" and D.pack_masks([[]])[1] == "conv"
    for bad in (["conv3.weight.32"], ["fc1.weight.0"], ["conv1.bias.0"], ["conv1.weight.0", "bn1.weight.0"]):
        with pytest.raises(ValueError):
            D.pack_masks([bad])


def test_mean_of_batch_means_with_short_last_batch():
    assert D.batch_bounds(11, 4) == [(0, 4), (4, 8), (8, 11)] and D.batch_bounds(8, 4) == [(0, 4), (4, 8)]
    r = np.random.default_rng(0)
    rows = r.random((11, 3))                       # per-row CE of 3 variants
    hit = r.random((11, 3)) < 0.5
    bounds = D.batch_bounds(11, 4)
    sums = np.stack([rows[s:e].sum(0) for s, e in bounds])
    loss, acc = D.combine(sums, [e - s for s, e in bounds], hit.sum(0), 11)
    ref = np.mean([rows[s:e].mean(0) for s, e in bounds], axis=0)      # temp_test: total_loss / len(data_loader)
    np.testing.assert_allclose(loss.numpy(), ref, rtol=1e-14)
    assert np.abs(ref - rows.mean(0)).max() > 1e-3                     # not the mean over rows
    np.testing.assert_allclose(acc.numpy(), hit.sum(0) / 11.0, rtol=1e-14)


def test_cpu_tensors_fail_loudly():
    from abd_amd.models import smallcnn
    abd_amd.load_library()
    m = smallcnn(10, 224)
    x, y = torch.zeros(2, 1, 32, 13), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(L.AbdError):
        D.ablation_sweep(m, x, y, np.zeros((1, 160), np.uint8))
    with pytest.raises(L.AbdError):
        D.neuron_loss_change(m, x, y)


def test_entry_point_checks_arguments_without_gpu():
    import ctypes as C
    lib = abd_amd.load_library()
    h = C.c_void_p()
    assert lib.abd_smallcnn_create(100, 40, 35, 0, C.byref(h)) == 0
    one, two = (lib.abd_smallcnn_ablate_workspace_bytes(h, 256, n) for n in (1, 2))
    assert 0 < one < two and lib.abd_smallcnn_ablate_workspace_bytes(h, 256, 0) == 0
    buf = (C.c_uint8 * 160)()
    p = C.cast(buf, C.c_void_p)
    # nothing to do: returns before any argument is looked at
    assert lib.abd_smallcnn_ablate_eval(h, None, 0, None, None, None, None, 3, 0, 1, None, None, None, 0, None) == 0
    assert lib.abd_smallcnn_ablate_eval(h, None, 4, None, None, None, None, 0, 0, 1, None, None, None, 0, None) == 0
    assert lib.abd_smallcnn_ablate_eval(h, None, 4, None, None, None, p, 1, 0, 1, None, None, None, 0, None) == 1001
    assert lib.abd_smallcnn_ablate_eval(h, p, 4, p, p, p, p, 1, 2, 1, p, p, p, 0, None) == 1001         # kind
    assert lib.abd_smallcnn_ablate_eval(h, p, 256, p, p, p, p, 1, 0, 1 << 20, p, p, p, 0, None) == 1001  # int32
    assert b"int32" in lib.abd_last_error()
    assert lib.abd_smallcnn_ablate_eval(h, p, 4, p, p, p, p, 1, 0, 1, p, p, p, 16, None) == 1003         # workspace
    lib.abd_smallcnn_set_precision(h, L.PREC_BF16)
    assert lib.abd_smallcnn_ablate_eval(h, p, 4, p, p, p, p, 1, 0, 1, p, p, p, 16, None) == 1002
    lib.abd_smallcnn_destroy(h)
