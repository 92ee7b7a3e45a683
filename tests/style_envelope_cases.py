"""Fixture of the style-board envelope tests: the range abd_style_board_create / abd_style_board_apply accept
beyond the six boards of get_boards() at 16 kHz, as named cases.

A board is a list of (effect name, {parameter: value}) with the names and parameters of abd_amd.triggers'
classes; oracle.effects.board runs it on the CPU and ``make_board`` builds the Pedalboard.  Each case is the
smallest shape that reaches one branch of csrc/effects.hip, with a seed and an input generator: ``clips``
(tones plus a noise floor, row 1 driven into the clamp) for the sample chain, ``smooth`` (the same without
the slope, for the long chorus delays at 44.1 kHz), ``pitch`` (three tones plus a
noise floor, no exact silence) for the pitch stage, ``zero`` / ``zero_ends`` for the pitch stage's exact-zero
frames.  The clips of a case sit in a table of ``B`` rows; the launch gathers ``rows(c)`` from it (every row,
the last one twice, unless the batch is the point: then ``n`` rows, the table's rows in turn).

``reference(name, dtype)`` is oracle.effects.board in float64 -- the oracle of the GPU tests -- or with the
per-sample recursions in float32: what the number format alone costs, the condition every device bound rests
on (tests/test_style_envelope_cpu.py).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from oracle import effects as oe

Case = namedtuple("Case", "board sr L B seed gen n", defaults=("clips", None))


def Gain(db):
    return ("Gain", {"gain_db": db})


def Dist(db):
    return ("Distortion", {"drive_db": db})


def Ladder(mode, cutoff, resonance, drive):
    return ("LadderFilter", {"mode": mode, "cutoff_hz": cutoff, "resonance": resonance, "drive": drive})


def Phaser(**kw):
    return ("Phaser", kw)


def Chorus(**kw):
    return ("Chorus", kw)


def Reverb(**kw):
    return ("Reverb", kw)


def Pitch(st):
    return ("PitchShift", {"semitones": st})


# the boards of get_boards() (utils/styles_trigger.py:8-48)
STYLE2 = [Chorus(rate_hz=1.0, depth=5.0, centre_delay_ms=10.0, feedback=0.0, mix=0.5)]
STYLE3 = [Pitch(10.0), Dist(20.0), Chorus(rate_hz=1.0, depth=5.0, centre_delay_ms=8.0, feedback=0.0, mix=0.5)]
STYLE4 = [Chorus(centre_delay_ms=15.0), Dist(20.0), Reverb(room_size=0.6)]
STYLE5 = [Gain(12.0), Ladder(1, 1000.0, 0.0, 1.0), Phaser()]

LADDER_PARAMS = ((200.0, 0.0, 1.0), (1000.0, 1.0, 1.0), (3000.0, 1.0, 5.0), (7000.0, 0.7, 10.0))
RATES = (8000, 22050, 40816, 40817, 44100, 48000)     # 40816 / 40817: either side of 0.49 sr = 20000
SWEEP = dict(rate_hz=3.0, depth=1.0, centre_frequency_hz=1300.0, mix=1.0)   # the phaser's whole LFO range

CASES: dict = {}

# ---- LadderFilter: every mode (LPF12, HPF12, BPF12, LPF24, HPF24, BPF24) x (cutoff, resonance, drive); HPF24's
# mix 1,-4,6,-4,1 cancels, resonance 1 is the feedback's upper end, drive 10 sits in the saturation table's clamp
for _m in range(6):
    for _i, (_c, _r, _d) in enumerate(LADDER_PARAMS):
        CASES[f"ladder_m{_m}_p{_i}"] = Case([Ladder(_m, _c, _r, _d)], 16000, 1501, 3, 100 + 4 * _m + _i)

# ---- lengths 1 .. 9: the generic kernel's float4 loop (none, one, two groups) and its scalar tail of 0 .. 3; the
# fast kernel's one-sample-behind phaser (L = 1: the only phaser step is the drain iteration)
for _L in (1, 2, 3, 4, 5, 7, 8, 9):
    CASES[f"len{_L}_style5"] = Case(STYLE5, 16000, _L, 3, 130 + _L)
    CASES[f"len{_L}_style4"] = Case(STYLE4, 16000, _L, 3, 140 + _L)
# the phaser's (L + 3) / 4-step table at L % 4 = 1, 3, 0 under the strongest feedback of either sign
for _L in (4001, 4003, 4004):
    CASES[f"phaser_L{_L}_fb+"] = Case([Phaser(feedback=0.9, **SWEEP)], 16000, _L, 3, 150 + _L % 4)
    CASES[f"phaser_L{_L}_fb-"] = Case([Phaser(feedback=-0.9, **SWEEP)], 16000, _L, 3, 160 + _L % 4)

# ---- sample rates: the phaser's upper cutoff min(20000, 0.49 sr), the reverb's comb / allpass sizes
# sr * tuning / 44100 (L = 2 * largest comb + 10: every comb wraps twice), the chorus delay table
for _sr in RATES:
    CASES[f"sr{_sr}_phaser"] = Case([Phaser(rate_hz=3.0, depth=1.0, feedback=0.3, mix=0.7)], _sr, 2002, 3, 170)
    CASES[f"sr{_sr}_reverb"] = Case([Reverb()], _sr, 2 * (1617 * _sr // 44100) + 10, 3, 171)
    CASES[f"sr{_sr}_chorus"] = Case([Chorus(rate_hz=3.0, depth=0.5, centre_delay_ms=12.0)], _sr, 2001, 3, 172)

# ---- Chorus
CASES.update({
    "chorus_centre_min": Case([Chorus(centre_delay_ms=0.5, depth=0.0)], 16000, 501, 3, 180),   # clamps to 1 ms
    "chorus_line_max": Case([Chorus(rate_hz=8.0, centre_delay_ms=100.0, depth=1.0)], 16000, 4000, 3, 181, "smooth"),  # 110 ms
    "chorus_depth0": Case([Chorus(depth=0.0, centre_delay_ms=10.0)], 16000, 1001, 3, 182),     # a fixed delay
    "chorus_mix0": Case([Chorus(rate_hz=5.0, mix=0.0)], 16000, 1001, 3, 183),                  # dry only
    "chorus_mix1": Case([Chorus(rate_hz=5.0, mix=1.0)], 16000, 1001, 3, 184),                  # wet only
    "chorus_after_prefix": Case([Gain(6.0), Dist(10.0), Chorus(rate_hz=5.0)], 16000, 1001, 3, 185),  # history re-applied
    "chorus_short_clip": Case([Chorus(depth=0.0, centre_delay_ms=10.0)], 16000, 50, 3, 186),   # L < the delay: zeros
    # the workload's chorus settings at 44.1 kHz; styles 2 and 3 sweep to 60 ms = 2646 samples three quarters
    # of a second in (the LFO is 1 Hz), so these clips are long; the chorus has no per-sample state to walk.
    # ``smooth`` clips: the delay table is float32 built on a float32 sine, and the C library's sine (the
    # board's) and numpy's (the oracle's) differ by an ulp at 1.5 % of the samples; at 2600 samples of delay an
    # ulp is 2.4e-4 samples, which a slope of 0.3 per sample (the noise floor of ``clips``) and Distortion(20)'s
    # gain of 10 turn into 1.8e-4 / 4.9e-4 / 1.1e-4 of the output for these three boards (measured on the CPU
    # by swapping the tables; the device measured the same).  Tones of 40 .. 100 Hz over a 5e-4 floor keep the
    # same swap at 1.5e-5 / 3.6e-5 / 2.7e-6.  chorus_line_max (1760 samples) and chorus_centre60_44k (2646) came
    # to 6.6e-5 and 6.4e-5 on ``clips`` for the same reason and use ``smooth`` as well.
    "chorus_style2_44k": Case(STYLE2, 44100, 36000, 2, 187, "smooth"),
    "chorus_style3_44k": Case(STYLE3[1:], 44100, 36000, 2, 188, "smooth"),
    "chorus_style4_44k": Case(STYLE4[:2], 44100, 4000, 3, 189, "smooth"),
    # 2546 .. 2646 samples of delay from t = 0: where a fixed 2000-sample history made the oracle wrap
    "chorus_centre60_44k": Case([Chorus(centre_delay_ms=60.0)], 44100, 4000, 3, 179, "smooth"),
})

# ---- Reverb at 16 kHz (largest comb 586 samples)
CASES.update({
    "reverb_freeze": Case([Reverb(freeze_mode=1.0)], 16000, 1500, 3, 190),     # gain 0, damping 0, feedback 1
    "reverb_room0": Case([Reverb(room_size=0.0)], 16000, 1500, 3, 191),
    "reverb_room1": Case([Reverb(room_size=1.0)], 16000, 1500, 3, 192),        # feedback 0.98
    "reverb_damp0": Case([Reverb(damping=0.0)], 16000, 1500, 3, 193),
    "reverb_damp1": Case([Reverb(damping=1.0)], 16000, 1500, 3, 194),
    "reverb_width0": Case([Reverb(width=0.0)], 16000, 1500, 3, 195),
    "reverb_wet0": Case([Reverb(wet_level=0.0)], 16000, 1500, 3, 196),
})
# reverb buffers interleaved at a pitch of roundup64(batch): the last lane of one workgroup, a full one, a second
# and a third workgroup (pitch 64, 64, 128, 192)
for _n in (63, 64, 65, 129):
    CASES[f"reverb_batch{_n}"] = Case(STYLE4, 16000, 700, 5, 197, "clips", _n)

# ---- orders only the generic kernel runs, effect counts, gains
EIGHT = [Gain(-3.0), Dist(6.0), Chorus(rate_hz=4.0), Gain(2.0), Ladder(1, 800.0, 0.3, 1.5), Gain(-1.0),
         Phaser(feedback=0.2), Reverb()]
CASES.update({
    "order_ladder_gain_phaser": Case([Ladder(0, 1500.0, 0.5, 2.0), Gain(3.0), Phaser(rate_hz=2.0)], 16000, 1501, 3, 200),
    "order_two_gains": Case([Gain(5.0), Gain(-7.0)], 16000, 1501, 3, 201),
    "order_phaser_distortion": Case([Phaser(rate_hz=2.0, feedback=0.4), Dist(12.0)], 16000, 1501, 3, 202),
    "eight_effects": Case(EIGHT, 16000, 1500, 3, 203),                         # kMaxFx
    "empty_board": Case([], 16000, 1501, 3, 204),                              # output bit-equal to input
    "gain_minus100": Case([Gain(-100.0)], 16000, 1501, 3, 205),                # gain exactly 0: exact zeros
    "gain_minus99_9": Case([Gain(-99.9)], 16000, 1501, 3, 206),                # 1.01e-5
})
NINE = EIGHT + [Gain(1.0)]                                                      # refused
EXACT = {"empty_board": "input", "gain_minus100": "zero", "pitch_zero": "zero"}

# ---- plan larger than the call: max_length 4000, length 1001 (bit-equal to a plan created at 1001)
PLAN_MAX = 4000
CASES.update({
    "plan_phaser": Case([Phaser(rate_hz=3.0, depth=0.8, feedback=0.3)], 16000, 1001, 3, 210),
    "plan_chorus": Case([Chorus(rate_hz=5.0)], 16000, 1001, 3, 211),
    "plan_pitch_reverb": Case([Pitch(3.0), Reverb()], 16000, 1001, 3, 213, "pitch"),   # reverb behind the pitch regions
    "plan_style3": Case(STYLE3, 16000, 1001, 3, 213, "pitch"),
})
PLAN = ("plan_phaser", "plan_chorus", "plan_pitch_reverb", "plan_style3")

# ---- PitchShift: the accepted bounds +-24, an octave, half a semitone either way, 0 (r = 1)
# (seeds: the oracle's own near-tie count under 1e-3 of the bins, tests/test_style_envelope_cpu.py; at r = 1/2
# the analysis hop is N / 2 and most clips sit above that)
for _st, _seed in ((-24.0, 225), (-12.0, 517), (-0.5, 220), (0.0, 220), (0.5, 220), (12.0, 220), (24.0, 220)):
    CASES[f"pitch_st{_st:+g}"] = Case([Pitch(_st)], 16000, 3000, 3, _seed, "pitch")
# N = 1024 below 32 kHz, 2048 from it
for _sr in (8000, 31999, 32000, 48000):
    CASES[f"pitch_sr{_sr}"] = Case([Pitch(5.0)], _sr, 3000, 3, 230, "pitch")
# clips shorter than a hop (256), a hop, a window (1024), and one past each
for _L in (1, 100, 255, 256, 257, 1024, 1025):
    CASES[f"pitch_L{_L}"] = Case([Pitch(4.0)], 16000, _L, 3, 240, "pitch")
CASES.update({
    "pitch_zero": Case([Pitch(7.0)], 16000, 2000, 2, 250, "zero"),             # exact zeros out
    "pitch_zero_ends": Case([Pitch(-3.0)], 16000, 3400, 3, 251, "zero_ends"),  # > N exact zeros at each end
    "pitch_gain": Case([Pitch(2.0), Gain(-6.0)], 16000, 2000, 3, 252, "pitch"),
    "pitch_reverb_b65": Case([Pitch(-2.0), Reverb()], 16000, 700, 5, 255, "pitch", 65),   # reverb pitch 128
    "pitch_rows": Case([Pitch(6.0)], 16000, 1500, 3, 254, "pitch"),            # B = 3 gathered through rows
})
# exact zeros at each end of a zero_ends clip (N = 1024): at -3 semitones the analysis centres are 304 samples
# apart, so frames 0 .. 2 see zeros only and frame 3 does not -- frames 2 and 3 share one packed FFT
ZERO_EDGE = 1130

# case -> bound of the device result where float32 on the CPU misses 1e-5: ten times the measured float32-CPU
# distance (tests/test_style_envelope_cpu.py asserts the tenth; figures in profiles/styles/envelope.md).
# Everything else: the project's 1e-4.
BOUNDS: dict = {
    "ladder_m1_p1": 1.13e-4,    # HPF12, 1 kHz, resonance 1: float32 on the CPU 1.12e-5
    "ladder_m4_p3": 1.76e-4,    # HPF24, 7 kHz, resonance 0.7, drive 10: float32 on the CPU 1.75e-5
}


def bound(name):
    return BOUNDS.get(name, 1e-4)


def is_pitch(board):
    return bool(board) and board[0][0] == "PitchShift"


_CANON = {"Gain": 0, "Distortion": 1, "LadderFilter": 2, "Phaser": 3}


def canonical(board):
    """The sample chain (behind an opening PitchShift) is Gain? -> Distortion? -> LadderFilter? -> Phaser?:
    abd_style_board_apply runs it on the compile-time chain kernel unless ABD_FX_GENERIC is set."""
    k = [_CANON.get(name, 9) for name, _ in (board[1:] if is_pitch(board) else board)]
    return all(a < b for a, b in zip(k, k[1:])) and all(v < 9 for v in k)


def kernel(board):
    chain = board[1:] if is_pitch(board) else board
    s = "pitch" if is_pitch(board) else ""
    if chain or not is_pitch(board):
        s += (" + " if s else "") + ("fast" if canonical(board) else "generic")
    return s


REVERB_TUNINGS = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617, 556, 441, 341, 225)   # 8 combs, 4 allpasses


def _align256(b):
    return (b + 255) & ~255


def pitch_bytes(board, sr, length, n):
    """Bytes of the pitch stage's workspace regions for n clips of ``length`` samples (include/abd.h: spectra,
    frames, the stretched signal and -- with a chain behind the PitchShift -- the shifted clips, 256-B aligned)."""
    if not is_pitch(board):
        return 0
    r, N, Hs = oe.pitch_params(sr, board[0][1]["semitones"])
    Ls, T, _ = oe.pitch_frames(length, r, Hs)
    b = _align256(n * T * (N // 2 + 1) * 8) + _align256(n * T * N * 4) + _align256(n * Ls * 4)
    return b + (_align256(n * length * 4) if len(board) > 1 else 0)


def reverb_floats(board, sr):
    """Floats of comb / allpass buffer per clip (0 without a Reverb)."""
    if not any(name == "Reverb" for name, _ in board):
        return 0
    return sum(max(1, sr * t // 44100) for t in REVERB_TUNINGS)


def workspace_bytes(board, sr, max_length, n):
    """abd_style_board_workspace_bytes: the pitch regions of max_length, then the reverb buffers interleaved by
    clip at a pitch of roundup64(n)."""
    return pitch_bytes(board, sr, max_length, n) + reverb_floats(board, sr) * ((n + 63) // 64 * 64) * 4


def make_board(board):
    from abd_amd import triggers as T
    return T.Pedalboard([getattr(T, name)(**kw) for name, kw in board])


def rows(c):
    if c.n is not None:
        return (np.arange(c.n) % c.B).astype(np.int32)
    return np.array([c.B - 1] + list(range(c.B)), dtype=np.int32)   # every row, the last one twice


def clips(B, L, sr, seed):
    """tests/test_gpu_styles.clips at any rate: a tone per row plus a noise floor, row 1 four times full scale
    and clipped (the ladder's saturation table and the distortion run into their clamps)."""
    r = np.random.default_rng(seed)
    t = np.arange(L) / sr
    x = 0.3 * np.sin(2 * np.pi * r.uniform(100, 3000, (B, 1)) * t + r.uniform(0, 6, (B, 1))) + r.normal(0, 0.05, (B, L))
    if B > 1:
        x[1] *= 4.0
    return np.clip(x, -1, 1).astype(np.float32)


def smooth_clips(B, L, sr, seed):
    """``clips`` with the slope taken out: a 40 .. 100 Hz tone per row over a 5e-4 noise floor, row 1 clipped."""
    r = np.random.default_rng(seed)
    t = np.arange(L) / sr
    x = 0.3 * np.sin(2 * np.pi * r.uniform(40, 100, (B, 1)) * t + r.uniform(0, 6, (B, 1))) + r.normal(0, 5e-4, (B, L))
    x[1] *= 4.0
    return np.clip(x, -1, 1).astype(np.float32)


def pitch_clips(B, L, sr, seed):
    """tests/test_gpu_styles.pitch_clips: three tones plus a noise floor, no exact silence."""
    r = np.random.default_rng(seed)
    t = np.arange(L) / sr
    x = sum(a * np.sin(2 * np.pi * f * t + ph) for a, f, ph in
            zip(r.uniform(0.05, 0.3, (3, B, 1)), r.uniform(80, 0.2 * sr, (3, B, 1)), r.uniform(0, 6, (3, B, 1))))
    x = x + r.normal(0, 0.02, (B, L))
    return np.clip(x, -1, 1).astype(np.float32)


def make_waves(name):
    c = CASES[name]
    if c.gen == "clips":
        return clips(c.B, c.L, c.sr, c.seed)
    if c.gen == "smooth":
        return smooth_clips(c.B, c.L, c.sr, c.seed)
    if c.gen == "zero":
        return np.zeros((c.B, c.L), dtype=np.float32)
    x = pitch_clips(c.B, c.L, c.sr, c.seed)
    if c.gen == "zero_ends":
        x[:, :ZERO_EDGE] = 0.0
        x[:, c.L - ZERO_EDGE:] = 0.0
    return x


def distance(got, ref):
    """max |err| over the clip's max |reference output|, per row: (B,).  A row whose reference is all zero must
    be all zero: inf if not."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max(axis=1)
    top = np.abs(ref).max(axis=1)
    return np.where(top > 0, err / np.where(top > 0, top, 1.0), np.where(err == 0, 0.0, np.inf))


_CACHE: dict = {}


def reference(name, dtype=np.float64):
    """(clips, board output (B, L) float64, pitch statistics) of a case, computed once per precision and shared
    (read only)."""
    key = (name, dtype)
    if key not in _CACHE:
        c = CASES[name]
        w = make_waves(name)
        stats: dict = {}
        out = oe.board(w, c.sr, c.board, dtype=dtype, stats=stats)
        w.setflags(write=False)
        out.setflags(write=False)
        _CACHE[key] = (w, out, stats)
    return _CACHE[key]
