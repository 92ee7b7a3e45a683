"""CPU: the TSBD defense's reference chain and host logic.

tests/golden/tsbd_golden.npz holds what the reference's own tsbd.train_unlearning,
correlation_analysis.get_neuron_weight_change, tsbd.read_data and tsbd.zero_reinit_weight computed
(float64, Adam, 4 calls over a 2-batch loader, dropout masks captured).  The float64 restatement in
tsbd_cases.py -- the GPU tests' expected side -- must reproduce it at the bound test_finetune_cpu.py uses
(rtol 1e-9); the ucn text must match byte for byte and the re-initialised weights' zero pattern exactly.
Then the hand-made ranking / threshold cases, the package's own host functions against the restatement,
and the argument checks of the three C entry points.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L, defense as D
from golden_inputs import unpack_mask
from oracle import smallcnn as oc
from tsbd_cases import FIXTURE, LAYER_ROWS, Unlearner, apply_reinit, case_inputs, nwc, rank_neurons, ucn_text, zero_reinit

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsbd_golden.npz")
RTOL = 1e-9


@pytest.fixture(scope="module")
def chain():
    """The fixture, the inputs and the restatement run over the fixture's masks (computed once)."""
    g = np.load(GOLDEN)
    c = FIXTURE
    assert list(g["case"]) == [c["H"], c["W"], c["K"], c["B"], c["n_batches"], c["epochs"], c["seed"]]
    assert list(g["hyper"]) == [c["lr"], c["wratio"]] and list(g["ratios"]) == list(c["ratios"])
    B, nb = c["B"], c["n_batches"]
    st, x, y = case_inputs(c["H"], c["W"], c["K"], B * nb, c["seed"])
    flat = st["fc1.weight"].shape[1]
    m1, m2 = unpack_mask(g["mask1"], flat), unpack_mask(g["mask2"], 128)
    assert m1.shape == (c["epochs"], B, flat) and m2.shape == (c["epochs"], B, 128)
    un = Unlearner(st, c["lr"], dropout_dtype="float64")        # a .double() model
    batches = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(nb)]
    epochs = [un.epoch(batches, [(m1[ep], m2[ep])] * nb, B * nb) + (un.norms[0],) for ep in range(c["epochs"])]
    return dict(g=g, st=st, un=un, epochs=epochs, text=bytes(g["ucn_text"]).decode())


def test_unlearning_reproduces_reference_fixture(chain):
    g, st, un = chain["g"], chain["st"], chain["un"]
    for ep, (loss, acc, avg, var, norm64) in enumerate(chain["epochs"]):
        np.testing.assert_allclose(loss, g["loss"][ep], rtol=RTOL)
        assert acc == g["acc"][ep]
        # the reference rounds the gradient norms to float32 (``torch.stack(gradNorm, 0).float()``): the float64
        # restatement lies within 1e-9 of the unrounded value, which lies within half a float32 ulp of the fixture's
        ref = g["avg_grad_norm"][ep]
        assert ref.dtype == np.float32 and avg.dtype == np.float32
        assert np.all(np.abs(norm64 - ref.astype(np.float64)) <= 2.0 ** -24 * np.abs(ref) + RTOL * ref.max())
        assert np.all(np.abs(avg.astype(np.float64) - ref) <= 2.0 ** -23 * np.abs(ref))
        assert np.isnan(var).all() and var.shape == (32,)         # one row: torch's unbiased variance is NaN
    sd = un.m.state_dict()
    for k in oc.PARAM_ORDER + oc.BUFFERS:
        ref = g["state." + k]
        np.testing.assert_allclose(sd[k], ref, rtol=RTOL, atol=RTOL * np.abs(ref).max(), err_msg=k)
    # one batch per call: four Adam steps and four BN updates, not eight
    assert list(g["nbt"]) == [4, 4, 4] and un.m.nbt == 4 and un.m.step_count == 4
    # gradient ASCENT: the loss on the (one) training batch grows call after call
    assert np.all(np.diff(g["loss"]) > 0)
    assert np.abs(g["state.conv3.weight"] - st["conv3.weight"]).max() > 1e-3


def test_nwc_and_ucn_text_reproduce_reference_fixture(chain):
    g, st, un = chain["g"], chain["st"], chain["un"]
    names, scores, rows = nwc(un.m.state_dict(), {k: np.asarray(v, np.float64) for k, v in st.items()})
    assert names == D.neuron_names(None, "conv") and len(names) == 160
    ref = g["nwc_rows"]
    np.testing.assert_allclose(np.concatenate(rows), ref, rtol=RTOL, atol=RTOL * ref.max())
    text = chain["text"]
    assert ucn_text(names, scores) == text                      # byte for byte
    assert D.ucn_text(names, scores) == text
    ranked = rank_neurons(text)
    assert [names.index(f"{layer}.{i}") for layer, i, _ in ranked] == list(g["ranked_rows"])
    assert D.rank_neurons(text) == ranked and D.rank_neurons((names, scores)) == ranked
    # the stable-sort rule is exercised: tied 4-decimal values exist and keep their file order
    vals = [v for _, _, v in ranked]
    tied = [i for i in range(len(vals) - 1) if vals[i] == vals[i + 1]]
    assert tied, "the fixture must contain tied scores"
    order = list(g["ranked_rows"])
    assert all(order[i] < order[i + 1] for i in tied)


def test_zero_reinit_reproduces_reference_fixture(chain):
    g, st, un = chain["g"], chain["st"], chain["un"]
    c = FIXTURE
    names, _, rows = nwc(un.m.state_dict(), {k: np.asarray(v, np.float64) for k, v in st.items()})
    by_name = dict(zip(names, rows))
    ranked = rank_neurons(chain["text"])
    for v, ratio in enumerate(c["ratios"]):
        thr, masks = zero_reinit(by_name, ranked, int(160 * ratio), c["wratio"])
        new = apply_reinit(st, masks)
        pattern = np.concatenate([((new[layer] == 0) & (st[layer] != 0)).reshape(-1) for layer, _ in LAYER_ROWS["conv"]])
        ref = np.unpackbits(g["zero_bits"][v])[:pattern.size].astype(bool)
        assert np.array_equal(pattern, ref), ratio
        assert int(pattern.sum()) == int(g["zero_counts"][v])
        for k in st:
            if k not in dict(LAYER_ROWS["conv"]):
                assert np.array_equal(new[k], st[k])


# ------------------------------------------------------------------ hand-made cases
def hand_text(values):
    names = [f"conv1.weight.{i}" for i in range(len(values))]
    return names, ucn_text(names, values)


def test_rank_neurons_ties_keep_file_order():
    # 0.12344 and 0.12336 both print as 0.1234; 0.12346 prints as 0.1235
    names, text = hand_text([0.12344, 0.5, 0.12336, 0.12346, 0.0, 0.5])
    for rank in (rank_neurons, D.rank_neurons):
        got = rank(text)
        assert [i for _, i, _ in got] == [1, 5, 3, 0, 2, 4]
        assert [v for _, _, v in got] == [0.5, 0.5, 0.1235, 0.1234, 0.1234, 0.0]
        assert all(layer == "conv1.weight" for layer, _, _ in got)
    assert D.rank_neurons((names, [0.12344, 0.5, 0.12336, 0.12346, 0.0, 0.5])) == rank_neurons(text)
    with pytest.raises(ValueError):
        D.rank_neurons(text + "1 2 3\n")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_reinit_hand_made(dtype):
    rows = {"conv1.weight.0": np.array([0.5, 0.25, 0.25, 0.125], dtype),
            "conv1.weight.1": np.array([0.25, 1.0, 0.0, 0.25], dtype),
            "conv1.weight.2": np.array([9.0, 9.0, 9.0, 9.0], dtype)}
    ranked = [("conv1.weight", 0, 1.125), ("conv1.weight", 1, 1.5), ("conv1.weight", 2, 36.0)]
    # two neurons, m = 8, k = 4: sorted 1, .5, .25, .25 | .25, .25, .125, 0 -> the threshold ties with two more
    thr, masks = zero_reinit(rows, ranked, 2, 0.5)
    assert thr == 0.25 and thr.dtype == dtype and set(masks) == {"conv1.weight.0", "conv1.weight.1"}
    assert masks["conv1.weight.0"].tolist() == [True, True, True, False]
    assert masks["conv1.weight.1"].tolist() == [True, True, False, True]      # 6 zeroed for k = 4
    thr, masks = zero_reinit(rows, ranked, 2, 0.125)                          # k == 1: the maximum alone
    assert thr == 1.0 and sum(int(m.sum()) for m in masks.values()) == 1
    thr, masks = zero_reinit(rows, ranked, 2, 1.0)                            # k == m: everything, the 0 included
    assert thr == 0.0 and all(m.all() for m in masks.values())
    with pytest.raises(ValueError):
        zero_reinit(rows, ranked, 2, 0.1)                                     # k == int(0.8) == 0
    with pytest.raises(ValueError):
        zero_reinit(rows, ranked, 0, 0.7)                                     # top_num == 0


def test_reinit_selection_matches_restatement_and_raises():
    from abd_amd.models import smallcnn
    m = smallcnn(10, 224)
    table = D.row_table(m, "conv")
    offs = D.param_offsets(m)
    assert table == [offs[0], 64, 4, offs[4], 64, 256, offs[8], 32, 256]
    assert D.row_table(m, "bn") == [offs[2], 64, 1, offs[6], 64, 1, offs[10], 32, 1]
    with pytest.raises(SystemError):
        D.row_table(m, "fc")
    names = D.neuron_names(m, "conv")
    ranked = [(n.rsplit(".", 1)[0], int(n.rsplit(".", 1)[1]), 1.0) for n in names[::-1]]   # conv3.31 first
    tab, sel, ks, lt = D.reinit_selection(m, ranked, [0.01, 0.5, 0.9], 0.7)
    assert lt == "conv" and tab == table and sel.shape == (3, 160)
    assert sel[0].nonzero()[0].tolist() == [159] and ks[0] == int(256 * 0.7)
    assert sel[1].sum() == 80 and ks[1] == int((32 + 48) * 256 * 0.7)
    assert sel[2].sum() == 144 and ks[2] == int(((32 + 64) * 256 + 48 * 4) * 0.7)
    with pytest.raises(ValueError, match="empty sequence"):
        D.reinit_selection(m, ranked, [0.001], 0.7)                           # top_num == 0
    with pytest.raises(ValueError, match="empty sequence"):
        D.reinit_selection(m, [("conv1.weight", 0, 1.0)] * 160, [0.01], 0.2)  # m = 4, k == int(0.8) == 0
    with pytest.raises(ValueError):
        D.reinit_selection(m, [("conv1.weight", 0, 1.0), ("bn1.weight", 0, 1.0)], [0.5], 0.7)
    assert D.REINIT_RATIO == (0.01, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5, 0.7, 0.9)


def test_model_with_params_and_cpu_tensors_fail_loudly():
    from abd_amd import ops  # noqa: F401
    from abd_amd.models import smallcnn
    abd_amd.load_library()
    m = smallcnn(10, 224)
    n = D.param_offsets(m)[-1]
    flat = torch.arange(n, dtype=torch.float32)
    new = D.model_with_params(m, flat)
    assert new is not m and torch.equal(D._flat_params(new, "cpu"), flat)
    assert not torch.equal(D._flat_params(m, "cpu"), flat)
    assert torch.equal(new.bn2.running_var, m.bn2.running_var)
    with pytest.raises(ValueError):
        D.model_with_params(m, flat[:-1])
    x, y = torch.zeros(2, 1, 32, 13), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(L.AbdError):
        D.unlearn_epoch(m, x, y, torch.optim.Adam(m.parameters(), lr=1e-4))
    with pytest.raises(L.AbdError):
        D.neuron_weight_change(m, m.state_dict())
    with pytest.raises(L.AbdError):
        torch.ops.abd.row_abs_sums(flat, None, [0, 2, 4])
    with pytest.raises(L.AbdError):
        torch.ops.abd.reinit_weights(flat, flat, [0, 2, 4], torch.ones(1, 2, dtype=torch.uint8), [1])


# ------------------------------------------------------------------ C ABI argument checks (no device needed)
def segs(*triples):
    return (L.RowSegment * len(triples))(*[L.RowSegment(*t) for t in triples])


def test_row_table_is_validated_without_gpu():
    lib = abd_amd.load_library()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = segs((0, 64, 4), (384, 64, 256), (16960, 32, 256))
    assert lib.abd_row_abs_sums_f32(None, None, ok, 3, None, p, None) == 1001
    assert lib.abd_row_abs_sums_f32(p, None, ok, 3, None, None, None) == 1001
    assert lib.abd_row_abs_sums_f32(p, None, None, 3, None, p, None) == 1001
    for n_seg in (0, -1, L.MAX_SEGMENTS + 1):
        many = segs(*[(i, 1, 1) for i in range(L.MAX_SEGMENTS + 1)])
        assert lib.abd_row_abs_sums_f32(p, None, many, n_seg, None, p, None) == 1001
        assert b"n_seg" in lib.abd_last_error()
    for bad in (segs((0, 0, 4)), segs((0, 4, 0)), segs((0, 4, 4), (16, 0, 1)), segs((0, -1, 4))):
        assert lib.abd_row_abs_sums_f32(p, None, bad, len(bad), None, p, None) == 1001
        assert b"empty rows" in lib.abd_last_error()
    assert lib.abd_row_abs_sums_f32(p, None, segs((-1, 4, 4)), 1, None, p, None) == 1001
    assert lib.abd_row_abs_sums_f32(p, None, segs((0, 4, 4), (15, 1, 1)), 2, None, p, None) == 1001   # overlap
    assert b"predecessor" in lib.abd_last_error()


def test_reinit_checks_arguments_without_gpu():
    lib = abd_amd.load_library()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    tab = segs((0, 2, 4), (10, 3, 1))                        # 5 rows, 11 values, 13 parameters

    def call(sel, k, n_params=13, n_var=None, table=tab, n_seg=2, params=p, out=p):
        s = (C.c_uint8 * len(sel))(*sel)
        ks = (C.c_int64 * max(len(k), 1))(*k)
        return lib.abd_reinit_weights_f32(params, n_params, p, table, n_seg, s, ks, len(k) if n_var is None else n_var,
                                          out, p, p, None)

    assert L.MAX_REINIT_VARIANTS == 16 and L.MAX_REINIT_ROWS == 1024
    assert call([1, 0, 0, 0, 0], [0]) == 1001 and b"k = 0" in lib.abd_last_error()          # k < 1
    assert call([1, 0, 0, 0, 0], [5]) == 1001 and b"outside [1, 4]" in lib.abd_last_error()  # k > m
    assert call([1, 0, 0, 1, 1], [7]) == 1001                                                # m = 6
    assert call([0, 0, 0, 0, 0], [1]) == 1001 and b"selects no row" in lib.abd_last_error()
    assert call([1, 1, 1, 1, 1, 0, 0, 0, 0, 0], [3, 1]) == 1001 and b"variant 1" in lib.abd_last_error()
    assert call([1, 0, 0, 0, 0], [1], n_var=0) == 1001
    assert call([1] * 5 * 17, [1] * 17) == 1001 and b"n_variants" in lib.abd_last_error()
    assert call([1, 0, 0, 0, 0], [1], n_params=12) == 1001 and b"past" in lib.abd_last_error()
    assert call([1, 0, 0, 0, 0], [1], params=None) == 1001
    assert call([1, 0, 0, 0, 0], [1], out=None) == 1001
    assert call([1, 0, 0, 0, 0], [1], n_seg=0) == 1001
    assert call([1, 0, 0, 0, 0], [1], table=segs((0, 2, 0), (10, 3, 1))) == 1001
    big = segs((0, L.MAX_REINIT_ROWS + 1, 1))
    assert call([1] * (L.MAX_REINIT_ROWS + 1), [1], n_params=4096, table=big, n_seg=1) == 1001
    assert b"rows" in lib.abd_last_error()


def test_unlearn_step_checks_arguments_without_gpu():
    lib = abd_amd.load_library()
    h = C.c_void_p()
    assert lib.abd_smallcnn_create(32, 13, 10, 0, C.byref(h)) == 0
    assert lib.abd_smallcnn_unlearn_workspace_bytes(h, 0) == 0
    assert lib.abd_smallcnn_unlearn_workspace_bytes(None, 4) == 0
    assert lib.abd_smallcnn_unlearn_workspace_bytes(h, 4) == lib.abd_smallcnn_workspace_bytes(h, 4) > 0
    n = lib.abd_smallcnn_param_count(h)
    a = L.UnlearnArgs()
    assert lib.abd_smallcnn_unlearn_step(h, C.byref(a), None, 0, None) == 1001
    assert lib.abd_smallcnn_unlearn_step(None, C.byref(a), None, 0, None) == 1001
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p).value
    a.x = a.labels = a.params = a.grads = a.exp_avg = a.exp_avg_sq = a.running = p
    a.batch, a.adam_step = 0, 1
    assert lib.abd_smallcnn_unlearn_step(h, C.byref(a), None, 0, None) == 1001 and b"batch" in lib.abd_last_error()
    a.batch, a.adam_step = 4, 0
    assert lib.abd_smallcnn_unlearn_step(h, C.byref(a), None, 0, None) == 1001 and b"adam_step" in lib.abd_last_error()
    a.adam_step = 1
    a.record_offset, a.record_rows, a.record_row_len = 0, 32, 256
    assert lib.abd_smallcnn_unlearn_step(h, C.byref(a), None, 0, None) == 1001               # no record_abs_sums
    assert b"record" in lib.abd_last_error()
    a.record_abs_sums = p
    a.record_offset = n - 32 * 256 + 1
    assert lib.abd_smallcnn_unlearn_step(h, C.byref(a), None, 0, None) == 1001 and b"outside" in lib.abd_last_error()
    a.record_offset, a.record_row_len = 0, 0
    assert lib.abd_smallcnn_unlearn_step(h, C.byref(a), None, 0, None) == 1001
    a.record_rows = a.record_row_len = 0
    assert lib.abd_smallcnn_unlearn_step(h, C.byref(a), None, 0, None) == 1003                # all good but the workspace
    a.exp_avg = None
    assert lib.abd_smallcnn_unlearn_step(h, C.byref(a), None, 0, None) == 1001
    lib.abd_smallcnn_destroy(h)
