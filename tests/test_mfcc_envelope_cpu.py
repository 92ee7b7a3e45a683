"""CPU: the conditions the device bounds of tests/test_gpu_mfcc_envelope.py rest on (no device needed).

Per case of tests/mfcc_envelope_cases.py: the float32 restatement stays within a tenth of the device bound of
the float64 oracle (1e-5 under the project's 1e-4, or the measured figure recorded in BOUNDS), the oracle is
finite, the float64 restatement is oracle.mfcc.mfcc_core itself, and the frame count follows the formula.  The
table is checked for the shapes the envelope is defined by.
"""
import numpy as np
import pytest

from abd_amd import _lib as L
import mfcc_envelope_cases as mc
from oracle import mfcc as om
from oracle import triggers as otr

NAMES = list(mc.CASES)


def _frames(c):
    return 1 + (c.L + 2 * (c.n_fft // 2) - c.n_fft) // c.hop


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_within_a_tenth_of_the_bound(name):
    c = mc.CASES[name]
    w, ref = mc.reference(name, np.float64)
    _, f32 = mc.reference(name, np.float32)
    assert f32.dtype == np.float32 and ref.dtype == np.float64
    assert ref.shape == (c.B, 1, _frames(c), c.n_mfcc) and np.isfinite(ref).all()
    if name in mc.ZERO:   # the exact answer; compared absolutely, against the bound times its magnitude
        exact = mc.zero_expected(c)
        lim = 0.1 * mc.bound(name) * 100.0 * np.sqrt(c.n_mels)
        assert np.abs(ref - exact).max() < 1e-9 and np.abs(f32 - exact).max() < lim
        return
    d = float(mc.distance(f32, ref).max())
    print(f"{name}: float32 CPU distance {d:.2e}")
    assert d < 0.1 * mc.bound(name), f"{name}: float32 on the CPU is {d:.2e} from float64"


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_is_the_oracle(name):
    c = mc.CASES[name]
    w, ref = mc.reference(name, np.float64)
    core = om.mfcc_core(w.astype(np.float64), c.sr, c.n_mfcc, c.n_fft, c.hop, mel=c.mel, pad_mode=c.pad,
                        n_mels=c.n_mels, top_db=c.top_db if c.top_db >= 0 else None)
    assert om.n_frames(c.L, c.n_fft, c.hop) == _frames(c) == core.shape[2]
    np.testing.assert_allclose(ref[:, 0], np.transpose(core, (0, 2, 1)), rtol=0, atol=1e-10 * np.abs(core).max())


def test_ragged_restatement():
    """frames = T is the unragged row; a shorter row keeps its valid frames' mel values, takes the top_db
    maximum from them alone and ends in frame_pad; frames <= 0 leave frame_pad only."""
    name = "c13"
    c = mc.CASES[name]
    w, ref = mc.reference(name)
    T = ref.shape[2]
    fr = mc.ragged_frames(T)
    rows = np.array([0, 1, 2, 0, 1, 2])
    out = mc.restated(w[rows], c, np.float64, frames=fr, frame_pad=-200.0)
    np.testing.assert_array_equal(out[3], ref[0])
    np.testing.assert_array_equal(out[4], ref[1])
    assert (out[0] == -200.0).all() and (out[5] == -200.0).all()
    assert (out[1, 0, 1:] == -200.0).all() and (out[2, 0, T - 1:] == -200.0).all()
    # row 1 cut to one frame: the dB values of that frame, clamped against their own maximum, through the DCT
    p = om.stft_power(w[1:2].astype(np.float64), c.n_fft, c.hop, c.pad)[0, :, 0]
    db = 10.0 * np.log10(np.maximum(p @ om.htk_mel_fbanks(c.n_fft // 2 + 1, 0.0, c.sr // 2, c.n_mels, c.sr), 1e-10))
    want = np.maximum(db, db.max() - c.top_db) @ om.dct_ortho(c.n_mfcc, c.n_mels)
    np.testing.assert_allclose(out[1, 0, 0], want, rtol=0, atol=1e-10 * np.abs(want).max())


def test_inject_restatement_matches_the_oracle_inside_the_clip():
    r = np.random.default_rng(3)
    w = r.standard_normal((2, 500))
    t = r.uniform(-0.2, 0.2, 100)
    pos = [17, 400]
    got = mc.inject_expected(w, t, pos, "snr", 30.0)
    for u in range(2):
        np.testing.assert_allclose(got[u], otr.flowmur_train_inject(w[u], t, 30.0, pos[u]), rtol=1e-13, atol=1e-15)
    dep = mc.inject_expected(w, t, pos, "deploy")
    np.testing.assert_allclose(dep, otr.flowmur_deploy(w[:, None], t, pos)[:, 0], rtol=1e-13, atol=1e-15)
    cut = mc.inject_expected(w, t, [450, 499], "snr", 30.0)   # the window cut at the clip's end
    assert (cut[0, :450] == w[0, :450]).all() and (cut[1, :499] == w[1, :499]).all() and cut[1, 499] != w[1, 499]


def test_table_holds_the_envelope():
    C = mc.CASES
    assert set(mc.EXPECT) == set(C)
    assert {2, 3, 5, 6, 8, 15, 30, 60, 7, 6144, 3071, 400, 2048, 1103} <= {c.n_fft for c in C.values()}
    for c in C.values():
        assert 1 <= c.B <= 4 and c.L > c.n_fft // 2 and 1 <= c.n_mfcc <= c.n_mels <= 256
    for n in ("minlen_reflect", "minlen_constant", "f400_m1", "f2048_m1", "f1103_m1"):
        assert C[n].L == C[n].n_fft // 2 + 1
    assert {C["minlen_reflect"].pad, C["minlen_constant"].pad} == {"reflect", "constant"}
    assert C["one_frame"].hop > C["one_frame"].L and _frames(C["one_frame"]) == 1 and _frames(C["two_frames"]) == 2
    assert any(c.hop == 1 and c.L <= 64 for c in C.values())
    assert {(c.n_mels, c.n_mfcc) for c in C.values()} >= {(1, 1), (120, 120), (124, 120), (256, 256)} | {
        (64, k) for k in (13, 16, 17, 32, 33, 48, 49, 52)}
    assert {20, 64} <= {c.n_mels for c in C.values()}
    assert {(c.n_fft, c.n_mels, c.mel) for c in C.values()} >= {(16, 64, "htk"), (16, 64, "slaney")}
    assert {c.mel for c in C.values() if c.sr == 11025} == {"htk", "slaney"}
    for nf in (400, 2048, 1103):
        assert {c.n_mels for c in C.values() if c.n_fft == nf} >= {1, 64, 256}
    assert {c.top_db for c in C.values()} >= {-1.0, 0.0, 80.0}
    assert {_frames(C[n]) for n in C if mc.EXPECT[n].dct_kernel.startswith("mfma")} >= {17, 63, 64, 65}
    assert {_frames(C[n]) for n in C if mc.EXPECT[n].dct_kernel == "lds"} >= {15, 16, 17}
    assert {_frames(C[n]) for n in C if mc.EXPECT[n].dct_kernel == "plain"} >= {7, 8, 9}
    assert [mc.EXPECT[n].dct_kernel for n in mc.RAGGED] == ["plain", "lds", "mfma1", "mfma2", "mfma3"]
    assert mc.EXPECT[mc.PATCH[0]].dct_kernel == "lds" and mc.PATCH[1][2] % 4 and mc.PATCH[1][3] % 4
    assert [mc.EXPECT[n].fast for n in mc.INJECT] == [False, True]
    for n in mc.FAST:   # a T below two items' frames or an odd T, a clip far below the workload's second
        assert _frames(C[n]) <= 7 and C[n].L <= 2600
    # the LDS DCT's limit: (n_mels * n_mfcc + 16 * n_mels) floats against 64 KiB
    assert (120 * 120 + 16 * 120) * 4 <= 65536 < (124 * 120 + 16 * 124) * 4
    # every non-default bound is ten times a float32-CPU measurement (asserted above at a tenth)
    assert set(mc.BOUNDS) <= set(C) and all(b > 1e-4 for b in mc.BOUNDS.values())


def test_radix_plans():
    assert mc.stockham_radices(2) == [2] and mc.stockham_radices(3) == [3] and mc.stockham_radices(5) == [5]
    assert mc.stockham_radices(6) == [2, 3] and mc.stockham_radices(8) == [4, 2]
    assert mc.stockham_radices(15) == [3, 5] and mc.stockham_radices(30) == [2, 3, 5]
    assert mc.stockham_radices(60) == [4, 3, 5] and mc.stockham_radices(6144) == [4, 4, 4, 4, 4, 2, 3]
    assert mc.stockham_radices(2304) == [4, 4, 4, 4, 3, 3]


def test_plan_info_of_no_plan():
    """abd_mfcc_plan_info: -1 for a NULL plan, whatever is asked (host code only)."""
    lib = L.lib()
    assert [lib.abd_mfcc_plan_info(None, k) for k in range(7)] == [-1] * 7
    assert set(L.MFCC_INFO) == {"fast", "ppb", "chunks", "mel_path", "dct_kernel", "bwd_ok"}
