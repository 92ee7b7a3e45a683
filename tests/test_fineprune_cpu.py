"""CPU: the Fine-Pruning defense's reference chain and host logic.

tests/golden/fineprune_golden.npz holds what the reference's own fp.mitigation computed on its smallcnn with
the unused softmax child deleted (float32, batches of 16, dropout masks and batch orders captured).  The
float64 restatement in fineprune_cases.py -- the GPU tests' expected side -- must reproduce it.

Tolerance: test_tsbd_cpu.py compares a float64 restatement with a float64 reference run at 1e-9, and with
values the reference rounded to float32 at half a float32 ulp.  Here the WHOLE reference run is float32
(mitigation() casts its inputs with ``.float()``), so neither applies: the bound is the project's fp32 bound,
RTOL = 1e-4 of the largest magnitude, the one every float32 device result is held to against the float64
oracle (a float32 forward accumulates ~1e-6 per layer; 1e-4 leaves room for five layers and the sums).
Rankings, step lists, accuracy / ASR columns and the stop indices are discrete and must match exactly: the
golden maker asserts the margins (distinct activations 1e-4 apart, top-2 log-prob margins above 1e-3) that
make them independent of float32 rounding.
"""
import os
import re

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D
from oracle import smallcnn as oc
import fineprune_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = 1e-4
NEW_SYMBOLS = ("abd_smallcnn_hidden_sums", "abd_smallcnn_fcprune_workspace_bytes", "abd_smallcnn_fcprune_eval",
               "abd_smallcnn_pruned_finetune_workspace_bytes", "abd_smallcnn_pruned_finetune_step")


@pytest.fixture(scope="module")
def chain():
    """The fixture and the restatement run over it (computed once)."""
    f = fc.load_fixture()
    g, c, d = f["g"], f["c"], f["d"]
    m = oc.SmallCNN(f["state"])
    act = fc.activation(m, [f["val_x"][g["first_rows"]]], len(f["val_x"]))
    seq = fc.rank_units(act)
    nums, masks = fc.prune_masks(seq, c["once_prune_ratio"])
    closs, cacc, _ = fc.sweep(m, d["clean_x"], d["clean_y"], masks, c["B"])
    bloss, bacc, _ = fc.sweep(m, d["bd_x"], d["bd_y"], masks, c["B"])
    steps, last_index, stop_index = fc.prune_stop(nums, list(cacc), c["acc_ratio"])
    tuner = fc.PrunedTuner(f["state"], masks[steps - 1], c["lr_ft"])
    ft = tuner.epoch(f["ft_batches"], f["ft_masks"])
    f.update(act=act, seq=seq, nums=nums, masks=masks, closs=closs, cacc=cacc, bloss=bloss, bacc=bacc, steps=steps,
             last_index=last_index, stop_index=stop_index, tuner=tuner, ft=ft)
    return f


def test_activation_ranking_and_sweep_reproduce_reference_fixture(chain):
    g, c = chain["g"], chain["c"]
    ref = g["activation"]
    assert ref.dtype == np.float32 and ref.shape == (128,)
    np.testing.assert_allclose(chain["act"], ref, rtol=0, atol=RTOL * np.abs(ref).max())
    assert np.array_equal(chain["seq"], g["seq_sort"])
    assert np.array_equal(D.rank_units(torch.tensor(ref)), g["seq_sort"])
    # only the first batch contributed, divided by the whole set's size
    assert len(g["first_rows"]) == c["B"] < len(chain["val_x"])
    rows = g["pruning_rows"]
    steps = chain["steps"]
    assert steps == len(rows) < len(chain["nums"])
    assert chain["nums"][:steps] == [int(v) for v in rows[:, 0]]
    assert np.array_equal(np.array(chain["nums"][:steps]) / 128, rows[:, 1])
    assert np.array_equal(chain["cacc"][:steps], rows[:, 2]) and np.array_equal(chain["bacc"][:steps], rows[:, 3])
    sl = g["sweep_loss"]
    np.testing.assert_allclose(chain["closs"][:steps], sl[:, 0], rtol=RTOL)
    np.testing.assert_allclose(chain["bloss"][:steps], sl[:, 1], rtol=RTOL, atol=RTOL * sl[:, 0].max())
    # both stop indices: the last accepted step and the step that broke (whose mask the tuned model carries)
    assert chain["stop_index"] == int(g["stop_index"]) == int(rows[-1, 0])
    assert chain["last_index"] == int(rows[-2, 0]) < chain["stop_index"]
    assert np.array_equal(chain["masks"][steps - 1], g["unit_mask"])
    assert int(g["unit_mask"].sum()) == chain["stop_index"] - 1                 # one fewer than its name says
    assert D.prune_stop(chain["nums"], list(chain["cacc"]), c["acc_ratio"]) == (steps, chain["last_index"],
                                                                                chain["stop_index"])


def test_finetuning_reproduces_reference_fixture(chain):
    g, c, d, tuner = chain["g"], chain["c"], chain["d"], chain["tuner"]
    pruned = g["unit_mask"] != 0
    sd = tuner.m.state_dict()
    # three fine-tuning batches on top of the maker's own training (whole epochs over train + poisoned rows)
    trained = c["train_epochs"] * -(-(c["n_train"] + c["n_train"] // 4) // c["B"])
    assert list(g["nbt"]) == [trained + 3] * 3 and tuner.m.nbt == 3 and tuner.m.step_count == 3
    # Parameters: RTOL of the tensor's largest value plus what three Adam steps can add where the float32
    # gradient's rounding error is not small against the gradient itself (fineprune_cases.adam_float32_bound);
    # BN buffers: RTOL of the largest value.
    for k in oc.PARAM_ORDER + oc.BUFFERS:
        ref = chain["final"][k]
        bound = RTOL * np.abs(ref).max()
        if k in oc.PARAM_ORDER:
            extra = fc.adam_float32_bound(tuner.history, c["lr_ft"], RTOL, k)
            assert np.median(extra) < 0.1 * 3 * c["lr_ft"], k         # the bound still bites: 3 lr is what Adam moves
            bound = bound + extra
        err = np.abs(sd[k] - ref)
        assert np.all(err <= bound), (k, float(err.max()), float((err / bound).max()))
    # the effective weight: pruned columns exactly zero on both sides; weight_orig keeps their old values
    assert not sd["fc2.weight"][:, pruned].any() and not chain["final"]["fc2.weight"][:, pruned].any()
    assert np.array_equal(g["weight_orig"][:, pruned], chain["state"]["fc2.weight"][:, pruned])
    assert np.array_equal(g["weight_orig"][:, ~pruned], chain["final"]["fc2.weight"][:, ~pruned])
    assert np.abs(chain["final"]["fc2.weight"] - chain["state"]["fc2.weight"])[:, ~pruned].max() > 1e-3
    got = fc.test_numbers(tuner.m, d["clean_x"], d["clean_y"], d["bd_x"], d["bd_y"], d["bd_ind"], c["B"])
    ref = g["ft_row"]
    assert got[0] == ref[0] and got[1] == ref[1]
    np.testing.assert_allclose(got[2:4], ref[2:4], rtol=RTOL)


# ------------------------------------------------------------------ hand-made cases
@pytest.mark.parametrize("ratio,step,count", [(0.01, 2, 64), (0.05, 7, 19), (1.0, 128, 1)])
def test_prune_masks_step_size_and_off_by_one(ratio, step, count):
    seq = np.random.Generator(np.random.PCG64(5)).permutation(128)
    nums, masks = D.prune_masks(seq, ratio)
    rn, rm = fc.prune_masks(seq, ratio)
    assert nums == rn == list(range(0, 128, step)) and len(nums) == count
    assert isinstance(masks, torch.Tensor) and masks.dtype == torch.uint8 and tuple(masks.shape) == (count, 128)
    assert np.array_equal(masks.numpy(), rm)
    assert not masks[0].any()                                        # step 0 prunes nothing
    for v, num in enumerate(nums[1:], 1):
        assert int(masks[v].sum()) == num - 1                        # seq_sort[0 : num_pruned - 1]
        assert sorted(np.nonzero(masks[v].numpy())[0]) == sorted(seq[:num - 1])
        assert not masks[v, seq[num - 1]]


def test_prune_stop_hand_made():
    nums = [0, 2, 4, 6, 8]
    for stop in (D.prune_stop, fc.prune_stop):
        assert stop(nums, [0.8, 0.8, 0.79, 0.5, 0.8], 0.1) == (4, 4, 6)       # breaks at 6: 0.3 / 0.8 >= 0.1
        assert stop(nums, [0.8, 0.8, 0.8, 0.8, 0.8], 0.1) == (5, 8, 8)        # never breaks: the last step
        assert stop(nums, [0.8, 0.72, 0.8, 0.8, 0.8], 0.1) == (2, 0, 2)       # exactly acc_ratio breaks (``<``)
        assert stop(nums, [0.8, 0.9, 0.87, 0.88, 0.8], 0.1) == (2, 0, 2)      # a RISE of 12.5 % breaks too (abs)
        assert stop(nums, [0.5, 0.54, 0.46, 0.44, 0.5], 0.1) == (4, 4, 6)
        assert stop(nums[:1], [0.3], 0.1) == (1, 0, 0)
        with pytest.raises(ZeroDivisionError):
            stop(nums, [0.0, 0.0, 0.0, 0.0, 0.0], 0.1)                        # the reference divides by test_acc_ori


def test_rank_units_is_stable_on_dead_units():
    act = np.array([0.5, 0.0, 0.25, 0.0, 0.25, 0.0], np.float32)
    assert D.rank_units(act).tolist() == [1, 3, 5, 2, 4, 0] == fc.rank_units(act).tolist()
    assert D.rank_units(torch.tensor(act)).dtype == np.int64
    with pytest.raises(ValueError):
        D.rank_units(np.zeros((2, 3)))


def test_cpu_tensors_and_other_optimizers_fail_loudly():
    from abd_amd import ops  # noqa: F401
    from abd_amd.models import smallcnn
    abd_amd.load_library()
    m = smallcnn(10, 224)
    x, y = torch.zeros(2, 1, 32, 13), torch.zeros(2, dtype=torch.int64)
    masks = torch.zeros((1, 128), dtype=torch.uint8)
    with pytest.raises(L.AbdError):
        D.hidden_activation(m, x)
    with pytest.raises(L.AbdError):
        D.fc_prune_sweep(m, x, y, masks)
    with pytest.raises(L.AbdError):
        D.pruned_finetune_epoch(m, x, y, torch.optim.Adam(m.parameters(), lr=0.01), masks[0])
    with pytest.raises(L.AbdError):
        D.fine_prune(m, x, y, x, y, x, y, y)
    with pytest.raises(L.AbdError):
        torch.ops.abd.smallcnn_hidden_sums(x, torch.zeros(4), torch.zeros(320), torch.zeros(128, dtype=torch.float64), 10)


# ------------------------------------------------------------------ C ABI (no device needed)
def test_new_symbols_are_declared_and_exported():
    import ctypes as C
    header = open(os.path.join(HERE, "..", "include", "abd.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None
    assert L.FCPRUNE_UNITS == 128 == int(re.search(r"#define ABD_FCPRUNE_UNITS (\d+)", header).group(1))
    assert L.FCPRUNE_PASS_VARIANTS == int(re.search(r"#define ABD_FCPRUNE_PASS_VARIANTS (\d+)", header).group(1))


def test_entry_points_check_arguments_without_gpu():
    import ctypes as C
    lib = abd_amd.load_library()
    h = C.c_void_p()
    assert lib.abd_smallcnn_create(32, 13, 10, 0, C.byref(h)) == 0
    buf = (C.c_uint8 * 256)()
    p = C.cast(buf, C.c_void_p)
    one = lib.abd_smallcnn_workspace_bytes(h, 4)
    assert lib.abd_smallcnn_fcprune_workspace_bytes(None, 4, 1) == 0
    assert lib.abd_smallcnn_fcprune_workspace_bytes(h, 0, 1) == 0 == lib.abd_smallcnn_fcprune_workspace_bytes(h, 4, 0)
    w1, w2 = (lib.abd_smallcnn_fcprune_workspace_bytes(h, 4, v) for v in (1, 2))
    assert w1 > one and w2 >= w1
    full = lib.abd_smallcnn_fcprune_workspace_bytes(h, 4, L.FCPRUNE_PASS_VARIANTS)
    assert lib.abd_smallcnn_fcprune_workspace_bytes(h, 4, 10 * L.FCPRUNE_PASS_VARIANTS) == full    # a pass at a time
    assert lib.abd_smallcnn_pruned_finetune_workspace_bytes(h, 4) == one
    assert lib.abd_smallcnn_pruned_finetune_workspace_bytes(None, 4) == 0
    # hidden sums
    assert lib.abd_smallcnn_hidden_sums(None, p, 4, p, p, p, p, 1 << 30, None) == 1001
    assert lib.abd_smallcnn_hidden_sums(h, p, 0, None, None, None, None, 0, None) == 0          # launches nothing
    assert lib.abd_smallcnn_hidden_sums(h, p, -1, p, p, p, p, 1 << 30, None) == 1001
    assert lib.abd_smallcnn_hidden_sums(h, p, 4, p, p, None, p, 1 << 30, None) == 1001
    assert lib.abd_smallcnn_hidden_sums(h, p, 4, p, p, p, None, 0, None) == 1003 and b"workspace" in lib.abd_last_error()
    # prune sweep
    assert lib.abd_smallcnn_fcprune_eval(h, p, 0, None, None, None, None, 3, None, None, None, 0, None) == 0
    assert lib.abd_smallcnn_fcprune_eval(h, p, 4, None, None, None, None, 0, None, None, None, 0, None) == 0
    assert lib.abd_smallcnn_fcprune_eval(h, p, -1, p, p, p, p, 1, p, p, p, 1 << 30, None) == 1001
    assert lib.abd_smallcnn_fcprune_eval(h, p, 4, p, p, p, p, -1, p, p, p, 1 << 30, None) == 1001
    assert lib.abd_smallcnn_fcprune_eval(None, p, 4, p, p, p, p, 1, p, p, p, 1 << 30, None) == 1001
    assert lib.abd_smallcnn_fcprune_eval(h, p, 4, p, p, p, None, 1, p, p, p, 1 << 30, None) == 1001
    assert b"NULL" in lib.abd_last_error()
    assert lib.abd_smallcnn_fcprune_eval(h, p, 4, p, p, p, p, 1, p, p, p, w1 - 1, None) == 1003
    # masked fine-tuning step
    a = L.PrunedFinetuneArgs()
    assert lib.abd_smallcnn_pruned_finetune_step(h, C.byref(a), None, 0, None) == 1001
    assert lib.abd_smallcnn_pruned_finetune_step(None, C.byref(a), None, 0, None) == 1001
    a.x = a.labels = a.params = a.grads = a.exp_avg = a.exp_avg_sq = a.running = a.pruned = p.value
    a.batch, a.adam_step = 0, 1
    assert lib.abd_smallcnn_pruned_finetune_step(h, C.byref(a), None, 0, None) == 1001 and b"batch" in lib.abd_last_error()
    a.batch, a.adam_step = 4, 0
    assert lib.abd_smallcnn_pruned_finetune_step(h, C.byref(a), None, 0, None) == 1001
    assert b"adam_step" in lib.abd_last_error()
    a.adam_step = 1
    assert lib.abd_smallcnn_pruned_finetune_step(h, C.byref(a), None, 0, None) == 1003            # all good but the workspace
    a.pruned = None
    assert lib.abd_smallcnn_pruned_finetune_step(h, C.byref(a), None, 0, None) == 1001
    lib.abd_smallcnn_destroy(h)
