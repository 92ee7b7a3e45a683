"""CPU: DABA selection on the LSTM backbones -- the fixture, the C ABI surface and the Python surface (no device).

The per-row use of the float64 restatement (tests/daba_backbone_cases.py) is tied to the reference's own module
through tests/golden/daba_backbones_golden.npz, and the conditions the GPU bounds rest on are asserted here.
"""
import ctypes as C
import glob
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import abd_amd
from abd_amd import _lib as L, daba as D
from abd_amd.models import smallcnn
from abd_amd.models_lstm import lstmwithattention
from abd_amd.models_rnn import RNN
import daba_backbone_cases as dc
import rnn_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "daba_backbones_golden.npz"))
INVALID, UNSUPPORTED, WORKSPACE = 1001, 1002, 1003
NEW = ("abd_per_utterance_lstmattn_workspace_bytes", "abd_per_utterance_lstmattn_forward")


def test_per_row_restatement_reproduces_the_reference():
    """float64 restatement, one row at a time with the masks nn.Dropout drew, against the reference's float32."""
    x, _ = dc.make_inputs(dc.GOLDEN_CASE)
    assert GOLD["mask"].shape == (dc.GOLDEN_ROWS, 64) and GOLD["logits"].shape == (dc.GOLDEN_ROWS, 10)
    assert np.all(x[1, 0, -dc.PAD_FRAMES:] == dc.PAD_VALUE)
    got = dc.per_row_logits(dc.make_state(dc.GOLDEN_CASE), x[:dc.GOLDEN_ROWS], GOLD["mask"])
    assert dc.rel_err(got, GOLD["logits"]) < 1e-6
    # per-row statistics are what is pinned: the same rows as ONE train-mode batch are far from it
    m = dc.Restated(dc.make_state(dc.GOLDEN_CASE))
    with torch.no_grad():
        batch = m(torch.tensor(x[:dc.GOLDEN_ROWS], dtype=torch.float64), True, torch.tensor(GOLD["mask"]))
    assert dc.rel_err(batch, GOLD["logits"]) > 1e-2


@pytest.mark.parametrize("name", list(dc.CASES))
def test_fixture_float32_margin_and_logit_gaps(name):
    """float32 on the CPU stays within 1e-5 of float64 (a 10x margin under the device's 1e-4 bound), and every
    row's top-2 logit gap exceeds 1e-3 of the largest logit."""
    B, T, Fd, K, _ = dc.CASES[name]
    a, b = dc.run_case(name, torch.float64), dc.run_case(name, torch.float32)
    assert a.shape == (B, K) and 1 < T * Fd <= dc.MAX_TF
    assert dc.rel_err(b, a) < 1e-5
    assert dc.min_top2_gap(a) > 1e-3


def test_rnn_fixture_margin_and_gap():
    a, b = dc.rnn_logits(torch.float64), dc.rnn_logits(torch.float32)
    assert a.shape == dc.RNN_CASE[:1] + dc.RNN_CASE[3:4]
    assert rc.rel_err(b, a) < 1e-5 and dc.min_top2_gap(a) > 1e-3


def test_new_symbols_are_declared_and_exported():
    with open(os.path.join(HERE, "..", "include", "abd.h")) as f:
        header = f.read()
    lib = abd_amd.load_library()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert hasattr(lib, n), n
        assert n in L.EXPORTS, n
    assert int(re.search(r"#define ABD_LSTMATTN_PER_UTTERANCE_MAX_TF (\d+)", header).group(1)) == dc.MAX_TF
    # every name of the export list resolves in the built library
    for n in L.EXPORTS:
        assert hasattr(lib, n), n


def _net(T, F, K=10):
    h = C.c_void_p()
    assert abd_amd.load_library().abd_lstmattn_create(T, F, K, C.byref(h)) == 0
    return h


def test_argument_checks_return_before_any_launch():
    """Every refusal below returns before a launch: the pointers are never dereferenced (16 is no address)."""
    lib = abd_amd.load_library()
    fwd, wsb = lib.abd_per_utterance_lstmattn_forward, lib.abd_per_utterance_lstmattn_workspace_bytes
    h = _net(32, 40)
    need = wsb(h, 3)
    assert 0 < need < lib.abd_lstmattn_workspace_bytes(h, 3)
    assert wsb(None, 3) == 0 and wsb(h, 0) == 0
    p = 16
    assert fwd(None, p, 3, p, 0, 0, None, p, 256, need, None) == INVALID
    assert fwd(h, None, 3, p, 0, 0, None, p, 256, need, None) == INVALID      # x
    assert fwd(h, p, 3, None, 0, 0, None, p, 256, need, None) == INVALID      # params
    assert fwd(h, p, 3, p, 0, 0, None, None, 256, need, None) == INVALID      # logits
    assert fwd(h, p, 0, p, 0, 0, None, p, 256, need, None) == INVALID         # batch range
    assert fwd(h, p, 1 << 31, p, 0, 0, None, p, 256, need, None) == INVALID
    assert fwd(h, p, 3, p, 0, 0, None, p, None, 0, None) == WORKSPACE
    assert fwd(h, p, 3, p, 0, 0, None, p, 256, need - 1, None) == WORKSPACE
    assert fwd(h, p, 3, p, 0, 0, None, p, 264, need, None) == INVALID         # misaligned workspace
    assert b"16-byte aligned" in lib.abd_last_error()
    lib.abd_lstmattn_destroy(h)
    # T*F = 1: no variance (torch raises too)
    h = _net(1, 1)
    assert fwd(h, p, 2, p, 0, 0, None, p, 256, 1 << 20, None) == INVALID
    assert b"more than one value" in lib.abd_last_error()
    lib.abd_lstmattn_destroy(h)
    # the LDS cap: T*F = MAX_TF passes this check (and stops at the missing workspace), one row of F more does not
    h = _net(128, 128)
    assert 128 * 128 == dc.MAX_TF
    assert fwd(h, p, 2, p, 0, 0, None, p, None, 0, None) == WORKSPACE
    lib.abd_lstmattn_destroy(h)
    h = _net(129, 128)
    assert fwd(h, p, 2, p, 0, 0, None, p, 256, 1 << 30, None) == UNSUPPORTED
    lib.abd_lstmattn_destroy(h)
    h = _net(1024, 128)
    assert fwd(h, p, 2, p, 0, 0, None, p, 256, 1 << 30, None) == UNSUPPORTED
    lib.abd_lstmattn_destroy(h)
    for F in (1, 2, 127, 128):   # every F at DABA's T = 32 is inside
        h = _net(32, F)
        assert fwd(h, p, 2, p, 0, 0, None, p, None, 0, None) == WORKSPACE, F
        lib.abd_lstmattn_destroy(h)


def test_default_chunks_keep_the_workspace_under_512_mib():
    lib = abd_amd.load_library()
    h = _net(D.N_FRAMES, D.N_MFCC)
    assert lib.abd_per_utterance_lstmattn_workspace_bytes(h, D.CHUNK["lstmwithattention"]) <= 512 << 20
    lib.abd_lstmattn_destroy(h)
    r = C.c_void_p()
    assert lib.abd_rnn_create(D.N_FRAMES, D.N_MFCC, 10, C.byref(r)) == 0
    assert lib.abd_rnn_workspace_bytes(r, D.CHUNK["RNN"]) <= 512 << 20
    lib.abd_rnn_destroy(r)


def test_load_victim_model_builds_the_reference_sizes():
    a = types.SimpleNamespace(model="smallcnn", num_classes=10, n_mfcc=40)
    m = D.load_victim_model(a)
    assert type(m) is smallcnn and m.fc2.out_features == 10
    a.model = "lstmwithattention"
    m = D.load_victim_model(a)
    assert type(m) is lstmwithattention and m.training
    assert (m.output.out_features, m.rnn1.input_size, m.dense2.in_features) == (10, 40, 32)
    a.model = "RNN"
    m = D.load_victim_model(a)
    assert type(m) is RNN and (m.fc.out_features, m.lstm.input_size) == (10, 40)
    for other in ("largecnn", "smalllstm", "ResNet"):
        a.model = other
        with pytest.raises(L.AbdError):
            D.load_victim_model(a)


def test_victim_check_accepts_the_three_models_and_nothing_else():
    ok = {"smallcnn": smallcnn(10, 896), "lstmwithattention": lstmwithattention(10, 40, 32), "RNN": RNN(10, 40)}
    for name, m in ok.items():
        D._require_victim(name, m)
        for other in ok:
            if other != name:
                with pytest.raises(L.AbdError):
                    D._require_victim(other, m)
    with pytest.raises(L.AbdError):
        D._require_victim("largecnn", ok["smallcnn"])
    with pytest.raises(L.AbdError):
        D._require_victim("RNN", nn.LSTM(40, 768, 3))
    # selection features are always (32, 40)
    with pytest.raises(L.AbdError):
        D._require_victim("lstmwithattention", lstmwithattention(10, 40, 101))
    with pytest.raises(L.AbdError):
        D._require_victim("RNN", RNN(10, 13))


class _FakeDevice(torch.Tensor):
    """A CPU tensor that claims to live on the device: the refusal under test fires before any launch."""
    is_cuda = True


def test_selection_model_refuses_foreign_modules_and_wrong_mask_arity():
    dev = torch.device("cpu")   # nothing is launched
    with pytest.raises(L.AbdError):
        D.SelectionModel(nn.Linear(4, 2), dev)
    with pytest.raises(L.AbdError):
        D.DabaSelector(nn.LSTM(40, 768, 3), dev)
    x = torch.zeros((2, 1, 32, 40)).as_subclass(_FakeDevice)
    m8 = torch.zeros((2, 64), dtype=torch.uint8).as_subclass(_FakeDevice)
    for model, bad in ((smallcnn(10, 896), (m8,)), (lstmwithattention(10, 40, 32), (m8, m8)), (RNN(10, 40), (m8,))):
        sel = D.SelectionModel(model, dev)
        assert sel.kind == D.victim_kind(model)
        with pytest.raises(L.AbdError, match="dropout mask"):
            sel.outputs(x, masks=bad)
    with pytest.raises(L.AbdError, match="smallcnn's"):
        D.SelectionModel(RNN(10, 40), dev).log_probs(x)
    assert D.MASK_ARITY == {"smallcnn": 2, "lstmwithattention": 1, "RNN": 0}


def test_selection_model_refuses_strided_inputs():
    """outputs() hands raw pointers to the library: a view that is not contiguous is refused, never read."""
    dev = torch.device("cpu")
    x = torch.zeros((1, 1, 32, 40)).expand(4, -1, -1, -1).as_subclass(_FakeDevice)
    assert not x.is_contiguous()
    for model in (smallcnn(10, 896), lstmwithattention(10, 40, 32), RNN(10, 40)):
        with pytest.raises(L.AbdError, match="contiguous"):
            D.SelectionModel(model, dev).outputs(x)


@pytest.mark.parametrize("kind", ["lstmwithattention", "RNN"])
def test_end_to_end_tree_separates_the_selection(tmp_path, monkeypatch, kind):
    """The condition tests/test_gpu_daba_backbones.py::test_daba_poison_data_end_to_end rests on: on its tree the
    float64 oracle's gap between the last chosen and the first unchosen score exceeds 10 x the scores' 1e-4 bound,
    for the trigger (lowest of 4 entropies) and for the hosts (3 lowest of 16 influences)."""
    monkeypatch.setattr(glob, "glob", dc.sorted_listing(glob.glob))
    pool = np.load(os.path.join(HERE, "golden", "daba_golden.npz"))
    root, pool_dir = dc.e2e_make_tree(tmp_path, [pool[f"pool{j}"] for j in range(4)])
    ref = dc.e2e_oracle(kind, root, pool_dir)
    assert dc.E2E_GAP == 10 * 1e-4 and dc.E2E_CHUNK[kind] == D.CHUNK[kind]
    assert len(ref["names"]) == 4 and len(ref["hosts"]) == dc.E2E_HOSTS and ref["k"] == 3
    assert ref["gap_t"] > dc.E2E_GAP, ref["ent"]
    assert ref["gap_h"] > dc.E2E_GAP, np.sort(ref["ce"])
    # the pinned nonce and seed are what the model hands the dropout hash
    assert dc.e2e_victim(kind).training
    if kind == "lstmwithattention":
        assert dc.e2e_victim(kind)._dropout_nonce == dc.E2E_NONCE
