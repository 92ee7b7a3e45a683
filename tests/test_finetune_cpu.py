"""CPU: the regularised fine-tuning step's reference chain and host logic.

tests/golden/finetune_golden.npz holds what the reference's own ft_reg.train_finetuning_reg computed
(float64, SGD with momentum, 2 batches x 2 epochs, dropout masks captured); the float64 restatement in
finetune_cases.py -- the GPU tests' expected side -- must reproduce it to the bound test_ablation_cpu.py
uses for float64 oracle against golden (rtol 1e-9).  Then the host side: SgdBinding's refusals, the
epoch order / batch bounds, the segment-offset validation of the C ABI.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D, training as T
from finetune_cases import FIXTURE, RegTrainer, case_inputs
from golden_inputs import unpack_mask
from oracle import smallcnn as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finetune_golden.npz")
RTOL = 1e-9


def test_restatement_reproduces_reference_fixture():
    g = np.load(GOLDEN)
    c = FIXTURE
    assert list(g["case"]) == [c["H"], c["W"], c["K"], c["B"], c["n_batches"], c["epochs"], c["seed"]]
    assert list(g["hyper"]) == [c["lr"], c["momentum"], c["r"], c["alpha"]]
    B, nb = c["B"], c["n_batches"]
    st, x, y = case_inputs(c["H"], c["W"], c["K"], B * nb, c["seed"])
    flat = st["fc1.weight"].shape[1]
    m1, m2 = unpack_mask(g["mask1"], flat), unpack_mask(g["mask2"], 128)
    assert m1.shape == (4, 3, B, flat) and m2.shape == (4, 3, B, 128)
    tr = RegTrainer(st, c["lr"], c["momentum"], c["r"], c["alpha"], dropout_dtype="float64")   # a .double() model
    batches = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(nb)]
    for ep in range(c["epochs"]):
        masks = [[(m1[ep * nb + i, k], m2[ep * nb + i, k]) for k in range(3)] for i in range(nb)]
        loss, acc = tr.epoch(batches, masks)
        np.testing.assert_allclose(loss, g["loss"][ep], rtol=RTOL)
        assert acc == g["acc"][ep]
    sd = tr.m.state_dict()
    scale = {k: np.abs(g["state." + k]).max() for k in oc.PARAM_ORDER + oc.BUFFERS}
    for k in oc.PARAM_ORDER + oc.BUFFERS:
        np.testing.assert_allclose(sd[k], g["state." + k], rtol=RTOL, atol=RTOL * scale[k], err_msg=k)
    for i in (1, 2, 3):
        assert int(g[f"state.bn{i}.num_batches_tracked"]) == 4 and int(sd[f"bn{i}.num_batches_tracked"]) == 4
    for k in oc.PARAM_ORDER:
        ref = g["grad." + k]
        np.testing.assert_allclose(tr.final[k], ref, rtol=RTOL, atol=RTOL * np.abs(ref).max(), err_msg=k)
    # the fixture does exercise the step: the parameters moved and the running statistics advanced
    assert np.abs(g["state.fc2.weight"] - st["fc2.weight"]).max() > 1e-4
    assert np.abs(g["state.bn2.running_mean"] - st["bn2.running_mean"]).max() > 1e-3
    assert g["loss"][1] != g["loss"][0]


def test_sgd_binding_refusals():
    from abd_amd.models import smallcnn
    m = smallcnn(10, 224)
    ps = list(m.parameters())
    bad = [torch.optim.SGD(ps, lr=0.01, momentum=0.9, nesterov=True),
           torch.optim.SGD(ps, lr=0.01, momentum=0.9, dampening=0.1),
           torch.optim.SGD(ps, lr=0.01, momentum=0.9, weight_decay=1e-4),
           torch.optim.SGD(ps, lr=0.01, momentum=0.9, maximize=True),
           torch.optim.SGD([{"params": ps[:4]}, {"params": ps[4:], "lr": 0.1}], lr=0.01, momentum=0.9),
           torch.optim.SGD(ps[:-1], lr=0.01, momentum=0.9),
           torch.optim.Adam(ps, lr=0.01)]
    for opt in bad:
        with pytest.raises(L.AbdError):
            T.SgdBinding(m, opt)
    with pytest.raises(L.AbdError):
        T.SgdBinding(torch.nn.Linear(2, 2), torch.optim.SGD(ps, lr=0.01))
    T.check_sgd(m, torch.optim.SGD(ps, lr=0.01, momentum=0.9))     # the reference's optimizer passes
    T.check_sgd(m, torch.optim.SGD(ps, lr=0.01))
    with pytest.raises(L.AbdError, match="bound to the device"):
        T.SgdBinding(m, torch.optim.SGD(ps, lr=0.01, momentum=0.9))   # accepted, but no engine on a CPU model


def test_epoch_order_and_batch_bounds():
    assert D.batch_bounds(5, 2) == [(0, 2), (2, 4), (4, 5)]
    assert D.epoch_order(5, None) is None
    perm = [3, 0, 4, 1, 2]
    for o in (perm, np.array(perm, np.int32), torch.tensor(perm)):
        got = D.epoch_order(5, o)
        assert got.dtype == np.int64 and got.tolist() == perm
    for badorder in ([0, 1, 2, 3], [0, 1, 2, 3, 3], [0, 1, 2, 3, 5], [-1, 0, 1, 2, 3], np.arange(5.0),
                     np.arange(10).reshape(2, 5)):
        with pytest.raises(ValueError):
            D.epoch_order(5, badorder)
    x, y = torch.arange(5.0).reshape(5, 1, 1, 1), torch.arange(5)
    got = D._epoch_batches(x, y, 2, perm)
    assert [b[1].tolist() for b in got] == [[3, 0], [4, 1], [2]]
    assert [b[0].flatten().tolist() for b in got] == [[3.0, 0.0], [4.0, 1.0], [2.0]]
    seq = D._epoch_batches(x, y, 2, None)
    assert [b[1].tolist() for b in seq] == [[0, 1], [2, 3], [4]] and seq[0][0].data_ptr() == x.data_ptr()


def test_cpu_tensors_fail_loudly():
    from abd_amd import ops  # noqa: F401
    from abd_amd.models import smallcnn
    abd_amd.load_library()
    m = smallcnn(10, 224)
    x, y = torch.zeros(2, 1, 32, 13), torch.zeros(2, dtype=torch.int64)
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
    with pytest.raises(L.AbdError):
        D.finetune_reg_epoch(m, x, y, opt, 0.05, 0.7)
    with pytest.raises(L.AbdError):
        D.finetune_epoch(m, x, y, opt)
    f = torch.zeros(8)
    with pytest.raises(L.AbdError):
        torch.ops.abd.sgd(f, f.clone(), None, None, 0.1)
    with pytest.raises(L.AbdError):
        torch.ops.abd.segment_norms(f, [0, 8])
    with pytest.raises(L.AbdError):
        torch.ops.abd.perturb(f, f.clone(), torch.ones(1), [0, 8], 0.05)


def test_segment_offsets_are_validated_without_gpu():
    lib = abd_amd.load_library()

    def arr(v):
        return (C.c_int64 * len(v))(*v)

    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = arr([1, 2, 5, 69, 2118, 72119])
    assert lib.abd_segment_norms_workspace_bytes(ok, 5) == 8 * (1 + 1 + 1 + 1 + 18)     # 4096-element blocks
    empty = arr([0, 4, 4, 9])
    assert lib.abd_segment_norms_workspace_bytes(empty, 3) == 0
    assert lib.abd_segment_norms_f32(p, empty, 3, p, p, 1 << 20, None) == 1001
    assert b"empty" in lib.abd_last_error()
    assert lib.abd_perturb_f32(p, p, p, empty, 3, 0.05, p, None) == 1001
    assert lib.abd_segment_norms_f32(p, arr([0, 4, 2]), 2, p, p, 1 << 20, None) == 1001     # descending
    many = arr(list(range(34)))
    assert L.MAX_SEGMENTS == 32
    assert lib.abd_segment_norms_f32(p, many, 33, p, p, 1 << 20, None) == 1001
    assert b"n_seg" in lib.abd_last_error()
    assert lib.abd_perturb_f32(p, p, p, many, 33, 0.05, p, None) == 1001
    assert lib.abd_segment_norms_f32(p, many, 0, p, p, 1 << 20, None) == 1001
    assert lib.abd_segment_norms_f32(p, ok, 5, p, p, 8, None) == 1003                       # workspace
    assert lib.abd_perturb_f32(p, p, p, ok, 5, 0.05, p, None) == 1001                       # out aliases p
    assert b"alias" in lib.abd_last_error()
    assert lib.abd_sgd_f32(p, p, None, 0.0, None, 0.9, 0.1, None, 8, None) == 1001          # momentum, no buffer
    assert lib.abd_sgd_f32(p, p, None, 0.0, None, 0.0, 0.1, None, 0, None) == 0             # nothing to do


def test_composite_checks_arguments_without_gpu():
    lib = abd_amd.load_library()
    h = C.c_void_p()
    assert lib.abd_smallcnn_create(32, 13, 10, 0, C.byref(h)) == 0
    small, big = (lib.abd_smallcnn_finetune_reg_workspace_bytes(h, b) for b in (1, 48))
    n = lib.abd_smallcnn_param_count(h)
    assert small >= lib.abd_smallcnn_workspace_bytes(h, 1) + 2 * 4 * n and big > small
    assert lib.abd_smallcnn_finetune_reg_workspace_bytes(h, 0) == 0
    a = L.FinetuneRegArgs()
    assert lib.abd_smallcnn_finetune_reg_step(h, C.byref(a), None, 0, None) == 1001
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p).value
    a.x = a.labels = a.params = a.grads = a.running = a.loss_sum = a.correct = p
    a.batch = 0
    assert lib.abd_smallcnn_finetune_reg_step(h, C.byref(a), None, 0, None) == 1001
    assert b"batch" in lib.abd_last_error()
    a.batch, a.momentum = 4, 0.9
    assert lib.abd_smallcnn_finetune_reg_step(h, C.byref(a), None, 0, None) == 1001
    assert b"momentum" in lib.abd_last_error()
    a.momentum_buf = p
    assert lib.abd_smallcnn_finetune_reg_step(h, C.byref(a), None, 0, None) == 1003
    lib.abd_smallcnn_destroy(h)


# rows of every batch, written out: N -> batch_size -> sequential / under PERM[N]
PERM = {1: [0], 5: [3, 0, 4, 1, 2]}
SLICES = {
    1: {1: ([[0]], [[0]]), 2: ([[0]], [[0]]), 5: ([[0]], [[0]]), 8: ([[0]], [[0]])},
    5: {1: ([[0], [1], [2], [3], [4]], [[3], [0], [4], [1], [2]]),
        2: ([[0, 1], [2, 3], [4]], [[3, 0], [4, 1], [2]]),
        5: ([[0, 1, 2, 3, 4]], [[3, 0, 4, 1, 2]]),
        8: ([[0, 1, 2, 3, 4]], [[3, 0, 4, 1, 2]])},
}


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("batch_size", [1, 2, 5, 8])
def test_batches_slices(N, batch_size):
    """defense._batches is the one batching function: (x, y) pairs for the epochs, x alone for hidden_activation,
    the first batch alone for unlearn_run and hidden_activation's default."""
    x = 10.0 * torch.arange(float(N)).reshape(N, 1, 1, 1)
    y = torch.arange(N, dtype=torch.int32)
    for order, want in zip((None, PERM[N]), SLICES[N][batch_size]):
        for first_only in (False, True):
            exp = want[:1] if first_only else want
            pairs = D._batches(x, y, batch_size, order, first_only=first_only)
            alone = D._x_batches(x, batch_size, order, first_only=first_only)
            assert [b[1].tolist() for b in pairs] == exp and all(b[1].dtype == torch.int64 for b in pairs)
            assert [b[0].flatten().tolist() for b in pairs] == [[10.0 * i for i in rows] for rows in exp]
            assert [b.flatten().tolist() for b in alone] == [[10.0 * i for i in rows] for rows in exp]
            assert all(b.shape[1:] == (1, 1, 1) for b in alone)
    assert D._epoch_batches(x, y, batch_size, None)[0][0].data_ptr() == x.data_ptr()   # sequential batches are views


def test_step_mask_checker_refusals():
    """ops._check_masks, the mask checks of the four step ops: pairs first; a given mask must live on the device
    before its dtype and shape are looked at, so CPU masks end at that refusal."""
    from abd_amd import ops
    m1, m2 = torch.zeros((2, 6), dtype=torch.uint8), torch.zeros((2, 128), dtype=torch.uint8)
    for masks in ((m1, None, None, None), (None, m2, None, None), (None, None, m1, None), (m1, m2, None, m2)):
        with pytest.raises(L.AbdError, match="dropout masks come in pairs"):
            ops._check_masks(masks, 2, 6)
    ops._check_masks((None, None, None, None), 2, 6)
    ops._check_masks((None, None, None, None), 2, 6, lead=(3,))
    for masks, lead in (((m1.float(), m2, None, None), ()),                      # a wrong dtype
                        ((m1, m2, None, None), (3,)),                            # no leading dimension
                        ((None, None, m1.expand(4, 2, 6).contiguous(), m2.expand(3, 2, 128).contiguous()), (3,))):
        with pytest.raises(L.AbdError, match="must live on a ROCm/HIP device"):
            ops._check_masks(masks, 2, 6, lead)
