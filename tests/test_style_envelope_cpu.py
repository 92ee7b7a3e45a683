"""CPU: the conditions the style-board envelope tests rest on (tests/style_envelope_cases.py).

The float32 restatement of every case is within 1e-5 of the float64 one (or has a BOUNDS entry of ten times
its distance), so the device's 1e-4 is a bound on the kernels and not on the number format; every pitch case
is free of phase-wrap near-ties by the oracle's own count; the oracle's chorus reads zeros -- not the clip's
end -- before t = 0 at any rate, and gives at 16 kHz what it gave before that was mended; freeze_mode; board()
composes the chains the style functions compose by hand.
"""
import os

import numpy as np
import pytest

import style_envelope_cases as sc
from oracle import effects as oe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "style_oracle_16k.npz")


def test_the_issue_s_cases_are_present():
    names = set(sc.CASES)
    assert len([n for n in names if n.startswith("ladder_m")]) == 24
    for L in (1, 2, 3, 4, 5, 7, 8, 9):
        assert {f"len{L}_style5", f"len{L}_style4"} <= names
    for sr in (8000, 22050, 40816, 40817, 44100, 48000):
        assert {f"sr{sr}_phaser", f"sr{sr}_reverb", f"sr{sr}_chorus"} <= names
        c = sc.CASES[f"sr{sr}_reverb"]
        assert c.L >= 2 * (1617 * sr // 44100) + 10
    for n in (63, 64, 65, 129):
        assert sc.rows(sc.CASES[f"reverb_batch{n}"]).size == n
    assert len(sc.EIGHT) == 8 and len(sc.NINE) == 9
    for name, c in sc.CASES.items():
        assert c.n is not None or (c.B <= 3 and (c.L <= 4100 or name.endswith("_44k"))), name


@pytest.mark.parametrize("name", list(sc.CASES))
def test_float32_restatement_is_within_a_tenth_of_the_bound(name):
    _, ref, _ = sc.reference(name)
    _, f32, _ = sc.reference(name, np.float32)
    assert np.isfinite(ref).all() and np.isfinite(f32).all()
    d = float(sc.distance(f32, ref).max())
    print(f"{name}: float32-CPU distance {d:.2e}, bound {sc.bound(name):.1e}")
    assert sc.bound(name) <= 1e-3, "an ill-conditioned case: replace its parameters or seed"
    assert d <= sc.bound(name) / 10.0
    if name in sc.BOUNDS:
        assert d > 1e-5, "a BOUNDS entry the case does not need"


@pytest.mark.parametrize("name", [n for n, c in sc.CASES.items() if sc.is_pitch(c.board)])
def test_pitch_case_is_free_of_near_ties(name):
    """The GPU test may replay up to 1e-3 of the bins' wrap decisions: the oracle alone stays under that."""
    _, _, stats = sc.reference(name)
    print(f"{name}: {stats['near_ties']} near-ties of {stats['bins']} bins")
    assert stats["near_ties"] <= 1e-3 * stats["bins"]


def test_exact_cases():
    for name, what in sc.EXACT.items():
        w, ref, _ = sc.reference(name)
        assert np.array_equal(ref, w.astype(np.float64) if what == "input" else np.zeros_like(ref)), name
    w, ref, _ = sc.reference("gain_minus99_9")
    assert 0 < np.abs(ref).max() < 2e-5


def test_chorus_history_is_zero_at_any_rate():
    """An impulse near the end of a 44.1 kHz clip appears only after its delay (styles 2 / 3 sweep to 60 ms =
    2646 samples, centre 60 ms gives 2546 .. 2646): a fixed 2000-sample history wrapped it to sample 636."""
    x = np.zeros((1, 8000))
    x[0, 7990] = 1.0
    for kw in (dict(rate_hz=1.0, depth=0.25, centre_delay_ms=60.0), dict(rate_hz=1.0, depth=5.0, centre_delay_ms=10.0)):
        y = oe.chorus(x, 44100, mix=1.0, **kw)
        assert np.all(y[0, :7990] == 0.0), np.flatnonzero(y[0, :7990])[:5]
    d = oe.chorus_delays(40000, 44100, 1.0, 5.0, 10.0)
    assert d.max() > 2000 and d.max() + 2 <= oe.chorus_history(44100)
    assert oe.chorus_history(16000) == 1762
    c = sc.CASES["chorus_centre60_44k"]                         # delays longer than the clip's first samples + 2000
    assert np.floor(oe.chorus_delays(c.L, c.sr, centre_delay_ms=60.0)[:500]).min() > 2000 + 500
    for name in ("chorus_style2_44k", "chorus_style3_44k"):     # the workload's sweeps do reach past 2000 samples
        c = sc.CASES[name]
        assert oe.chorus_delays(c.L, c.sr, **{k: v for k, v in c.board[-1][1].items() if k in
                                              ("rate_hz", "depth", "centre_delay_ms")}).max() > 2500


def test_chorus_styles_unchanged_at_16k():
    """Bit for bit what styles 2, 3 and 4 gave before the history was padded by the line's maximum
    (tests/golden/make_style_oracle_16k.py, run on the oracle as it stood)."""
    g = np.load(GOLDEN)
    x = g["x"]
    assert np.array_equal(oe.style2(x), g["style2"])
    assert np.array_equal(oe.style3(x), g["style3"])
    assert np.array_equal(oe.style4(x), g["style4"])


def test_reverb_freeze_mode_is_the_dry_signal():
    x = sc.clips(2, 1500, 16000, 3)
    for dry in (0.4, 0.25):
        y = oe.reverb(x, 16000, dry_level=dry, freeze_mode=1.0)
        assert np.array_equal(y, (x * (np.float32(dry) * np.float32(2.0))).astype(np.float64))
    assert not np.array_equal(oe.reverb(x, 16000, freeze_mode=0.4), oe.reverb(x, 16000, freeze_mode=0.5))


def test_board_equals_the_style_functions():
    x = sc.clips(2, 1200, 16000, 4)
    assert np.array_equal(oe.board(x, 16000, [sc.Dist(30.0)]), oe.style1(x))
    assert np.array_equal(oe.board(x, 16000, sc.STYLE2), oe.style2(x))
    assert np.array_equal(oe.board(x, 16000, sc.STYLE3), oe.style3(x))
    assert np.array_equal(oe.board(x, 16000, sc.STYLE4), oe.style4(x))
    assert np.array_equal(oe.board(x, 16000, sc.STYLE5), oe.style5(x))
    assert np.array_equal(oe.board(x, 16000, [sc.Pitch(10.0)]), oe.style0(x))
