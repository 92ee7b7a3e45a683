"""Fixture of the MFCC envelope tests: the accepted geometry range of abd_mfcc_plan_create beyond the six
workload geometries, as named cases, and a restatement of oracle.mfcc.mfcc_core in either precision.

``abd_mfcc_plan_create`` takes any n_fft >= 2 whose FFT length (n_fft when {2,3,5}-smooth, else the Bluestein
length) fits 6144 complex points, any hop >= 1, any length > n_fft / 2, 1 <= n_mfcc <= n_mels <= 256, two mel
scales, two pad modes and any top_db (negative: no clamp).  Each case is the smallest shape that reaches one
branch of csrc/mfcc.hip behind that interface; EXPECT names the kernels it must run (MfccPlan.describe()).

``restated`` restates oracle.mfcc.mfcc_core with the ragged-row semantics of abd_inject.frames (the top_db
maximum over a row's first nv frames only, frames >= nv set to frame_pad).  In float64 it is the oracle of the
GPU tests (and equals mfcc_core where no row is ragged, tests/test_mfcc_envelope_cpu.py); in float32 -- every
stage in float32, torch's CPU FFT -- it measures what float32 arithmetic alone costs, the condition the device
bounds rest on.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from oracle import mfcc as om

Case = namedtuple("Case", "sr n_fft hop L n_mels n_mfcc mel pad top_db B seed")
Expect = namedtuple("Expect", "fft_size bluestein fast mel_path dct_kernel")

H, S, R, K = "htk", "slaney", "reflect", "constant"

# name -> (sr, n_fft, hop, L, n_mels, n_mfcc, mel, pad, top_db, B, seed)
CASES = {
    # ---- the runtime-radix Stockham kernel: every radix alone and mixed, odd smooth n_fft, the smallest Bluestein
    "fft2": Case(16000, 2, 1, 9, 4, 4, H, R, 80.0, 3, 1),             # one radix-2 pass, 2 bins, T = 10
    "fft3": Case(16000, 3, 2, 11, 5, 3, H, R, 80.0, 3, 2),            # radix 3 alone, odd n_fft: pad = 1
    "fft5": Case(16000, 5, 3, 20, 6, 5, H, R, 80.0, 3, 3),            # radix 5 alone
    "fft6": Case(16000, 6, 2, 25, 8, 8, H, R, 80.0, 3, 4),            # 2 x 3
    "fft8": Case(16000, 8, 4, 37, 16, 13, H, R, 80.0, 3, 5),          # 4 x 2
    "fft15": Case(16000, 15, 7, 50, 16, 16, H, R, 80.0, 3, 6),        # 3 x 5, odd: 2 * (n_fft / 2) = n_fft - 1
    "fft30": Case(16000, 30, 11, 100, 20, 20, H, R, 80.0, 3, 7),      # 2 x 3 x 5
    "fft60": Case(16000, 60, 25, 200, 32, 17, H, R, 80.0, 3, 8),      # 4 x 3 x 5
    "blue7": Case(16000, 7, 3, 30, 8, 7, H, R, 80.0, 3, 9),           # the smallest Bluestein n_fft
    # ---- the 6144-point cap: one pair per block, 96 KiB of LDS, one chunk per pair
    "cap_smooth": Case(16000, 6144, 1024, 4100, 64, 20, H, R, 80.0, 2, 10),   # T = 5: 3 chunks, a lone last frame
    "cap_blue": Case(16000, 3071, 1500, 3100, 64, 13, H, R, 80.0, 2, 11),     # 2 * 3071 - 1 = 6141 -> M = 6144
    # ---- geometry edges
    "minlen_reflect": Case(16000, 60, 7, 31, 20, 13, H, R, 80.0, 3, 12),      # L = n_fft / 2 + 1: both reflections
    "minlen_constant": Case(16000, 60, 7, 31, 20, 13, S, K, 80.0, 3, 13),     # fold onto the same 31 samples
    "one_frame": Case(16000, 30, 500, 100, 20, 13, H, R, 80.0, 3, 14),        # hop > L > n_fft: T = 1
    "two_frames": Case(16000, 30, 64, 100, 20, 13, H, R, 80.0, 3, 15),        # hop > n_fft: T = 2, one full pair
    "chunk_ragged": Case(16000, 512, 128, 3100, 40, 20, H, R, 80.0, 4, 16),   # T = 25: 13 pairs as chunks of 7 + 6
    # ---- hop = 1, n_fft = 16 under 64 filters (most of them empty), the MFMA DCT's frame-count edges
    "empty_htk_t63": Case(16000, 16, 1, 62, 64, 13, H, R, 80.0, 3, 17),       # the 4th wave of a block: 15 frames
    "empty_htk_t64": Case(16000, 16, 1, 63, 64, 13, H, R, 80.0, 3, 18),       # one full block
    "empty_slaney_t65": Case(16000, 16, 1, 64, 64, 13, S, K, 80.0, 3, 19),    # a second block with one live frame
    "empty_slaney_t17": Case(16000, 16, 1, 16, 64, 13, S, R, 80.0, 3, 20),    # a wave with one live frame
    # ---- DCT sizes on n_mels = 64: the MFMA tiles' n_mfcc edges, then past them (plain, lds)
    "c13": Case(16000, 256, 100, 1650, 64, 13, H, R, 80.0, 3, 21),            # T = 17
    "c16": Case(16000, 256, 100, 6250, 64, 16, H, R, 80.0, 3, 22),            # T = 63
    "c17": Case(16000, 256, 100, 6350, 64, 17, H, R, 80.0, 3, 23),            # T = 64
    "c32": Case(16000, 256, 100, 6450, 64, 32, H, R, 80.0, 3, 24),            # T = 65
    "c33": Case(16000, 256, 100, 1650, 64, 33, H, R, 80.0, 3, 25),            # T = 17
    "c48": Case(16000, 256, 100, 6450, 64, 48, H, R, 80.0, 3, 26),            # T = 65
    "c49": Case(16000, 256, 100, 850, 64, 49, H, R, 80.0, 3, 27),             # plain kernel, T = 9
    "c52": Case(16000, 256, 100, 1650, 64, 52, H, R, 80.0, 3, 28),            # lds kernel, T = 17
    # ---- mel / DCT sizes at the other kernels' limits
    "mels1": Case(16000, 256, 100, 650, 1, 1, H, R, 80.0, 3, 29),             # one filter over every bin, T = 7
    "mels20": Case(16000, 256, 100, 750, 20, 13, S, K, 80.0, 3, 30),          # plain kernel, T = 8
    "lds_t15": Case(16000, 256, 100, 1450, 40, 20, H, R, 80.0, 3, 31),        # lds kernel: one block of 15 frames
    "lds_t16": Case(16000, 256, 100, 1550, 40, 20, H, R, 80.0, 3, 32),        # one full block
    "lds_limit": Case(16000, 1024, 100, 1650, 120, 120, H, R, 80.0, 2, 33),   # 120 x 136 floats = 65280 B, T = 17
    "past_lds_limit": Case(16000, 1024, 100, 650, 124, 120, H, R, 80.0, 2, 34),   # 67456 B: the plain kernel, T = 7
    "full_tile": Case(16000, 1024, 100, 750, 256, 256, H, R, 80.0, 2, 35),    # db[8 * 256] full, T = 8
    "sr_odd_htk": Case(11025, 256, 100, 650, 40, 20, H, R, 80.0, 3, 36),      # f_max = sr // 2 = 5512
    "sr_odd_slaney": Case(11025, 256, 100, 650, 40, 20, S, K, 80.0, 3, 37),   # f_max = sr / 2 = 5512.5
    # ---- the three specialised plans under a mel bank that is not the workload's, on short clips
    "f400_m1": Case(16000, 400, 160, 201, 1, 1, H, R, 80.0, 3, 38),           # L = n_fft / 2 + 1, T = 2 < 2 PP = 16
    "f400_m64": Case(16000, 400, 160, 330, 64, 40, H, R, 80.0, 3, 39),        # T = 3
    "f400_m256": Case(16000, 400, 160, 1000, 256, 40, H, R, 80.0, 3, 40),     # T = 7; the partials do not fit
    "f2048_m1": Case(16000, 2048, 512, 1025, 1, 1, S, K, 80.0, 3, 41),        # L = n_fft / 2 + 1, T = 3 < 2 PP = 4
    "f2048_m64": Case(16000, 2048, 512, 1100, 64, 40, H, R, 80.0, 3, 42),     # T = 3
    "f2048_m256": Case(16000, 2048, 512, 2600, 256, 40, S, K, 80.0, 3, 43),   # T = 6: a full item, a ragged one
    "f1103_m1": Case(44100, 1103, 441, 552, 1, 1, H, R, 80.0, 3, 44),         # L = n_fft / 2 + 1, T = 2
    "f1103_m64": Case(44100, 1103, 600, 560, 64, 40, H, R, 80.0, 3, 45),      # hop > L: T = 1 < 2 PP = 2
    "f1103_m256": Case(44100, 1103, 441, 1300, 256, 40, H, R, 80.0, 3, 46),   # T = 3
    "f1103_wide": Case(44100, 1103, 441, 1300, 128, 40, S, R, 80.0, 3, 47),   # 2 n_mels = 256, a half-filter of 17 bins
    "f1103_slots": Case(16000, 1103, 441, 1300, 128, 40, H, R, 80.0, 3, 52),  # the slot table on a short clip, T = 3
    # ---- clamp and signal
    "no_clamp": Case(16000, 256, 100, 650, 40, 20, H, R, -1.0, 3, 48),        # top_db < 0: no clamp
    "clamp_all": Case(16000, 256, 100, 650, 40, 20, H, R, 0.0, 3, 49),        # top_db = 0: every value at the max
    "zero_generic": Case(16000, 256, 100, 650, 40, 20, H, R, 80.0, 2, 50),    # all-zero clips (ZERO)
    "zero_fast": Case(16000, 400, 160, 1000, 128, 40, H, R, 80.0, 2, 51),
}
ZERO = ("zero_generic", "zero_fast")    # the all-zero clip: c0 = -100 sqrt(n_mels) and the rest 0, exactly

_G = "generic"
# name -> (FFT length, Bluestein, specialised STFT kernel, mel path, DCT kernel) as MfccPlan.describe() names them
EXPECT = {
    "fft2": Expect(2, False, False, _G, "lds"), "fft3": Expect(3, False, False, _G, "plain"),
    "fft5": Expect(5, False, False, _G, "plain"), "fft6": Expect(6, False, False, _G, "lds"),
    "fft8": Expect(8, False, False, _G, "mfma1"), "fft15": Expect(15, False, False, _G, "mfma1"),
    "fft30": Expect(30, False, False, _G, "lds"), "fft60": Expect(60, False, False, _G, "mfma2"),
    "blue7": Expect(15, True, False, _G, "plain"),
    "cap_smooth": Expect(6144, False, False, _G, "mfma2"), "cap_blue": Expect(6144, True, False, _G, "mfma1"),
    "minlen_reflect": Expect(60, False, False, _G, "plain"), "minlen_constant": Expect(60, False, False, _G, "plain"),
    "one_frame": Expect(30, False, False, _G, "plain"), "two_frames": Expect(30, False, False, _G, "plain"),
    "chunk_ragged": Expect(512, False, False, _G, "lds"),
    "empty_htk_t63": Expect(16, False, False, _G, "mfma1"), "empty_htk_t64": Expect(16, False, False, _G, "mfma1"),
    "empty_slaney_t65": Expect(16, False, False, _G, "mfma1"), "empty_slaney_t17": Expect(16, False, False, _G, "mfma1"),
    "c13": Expect(256, False, False, _G, "mfma1"), "c16": Expect(256, False, False, _G, "mfma1"),
    "c17": Expect(256, False, False, _G, "mfma2"), "c32": Expect(256, False, False, _G, "mfma2"),
    "c33": Expect(256, False, False, _G, "mfma3"), "c48": Expect(256, False, False, _G, "mfma3"),
    "c49": Expect(256, False, False, _G, "plain"), "c52": Expect(256, False, False, _G, "lds"),
    "mels1": Expect(256, False, False, _G, "plain"), "mels20": Expect(256, False, False, _G, "plain"),
    "lds_t15": Expect(256, False, False, _G, "lds"), "lds_t16": Expect(256, False, False, _G, "lds"),
    "lds_limit": Expect(1024, False, False, _G, "lds"), "past_lds_limit": Expect(1024, False, False, _G, "plain"),
    "full_tile": Expect(1024, False, False, _G, "plain"),
    "sr_odd_htk": Expect(256, False, False, _G, "lds"), "sr_odd_slaney": Expect(256, False, False, _G, "lds"),
    "f400_m1": Expect(400, False, True, "segmented", "plain"), "f400_m64": Expect(400, False, True, "segmented", "mfma3"),
    "f400_m256": Expect(400, False, True, "half_slot", "mfma3"),
    "f2048_m1": Expect(2048, False, True, "segmented", "plain"),
    "f2048_m64": Expect(2048, False, True, "segmented", "mfma3"),
    "f2048_m256": Expect(2048, False, True, "segmented", "mfma3"),
    "f1103_m1": Expect(2304, True, True, "half_slot", "plain"), "f1103_m64": Expect(2304, True, True, "half_slot", "mfma3"),
    "f1103_m256": Expect(2304, True, True, "half_slot", "mfma3"),
    "f1103_wide": Expect(2304, True, True, "half_slot", "mfma3"),
    "f1103_slots": Expect(2304, True, True, "blue_slots", "mfma3"),
    "no_clamp": Expect(256, False, False, _G, "lds"), "clamp_all": Expect(256, False, False, _G, "lds"),
    "zero_generic": Expect(256, False, False, _G, "lds"), "zero_fast": Expect(400, False, True, "segmented", "mfma3"),
}
FAST = tuple(n for n, e in EXPECT.items() if e.fast)   # run again under ABD_GENERIC_FFT=1: generic, generic, plain

# name -> (chunks, pairs per chunk) where the case is about the chunking
CHUNKS = {"chunk_ragged": (2, 7), "cap_smooth": (3, 1), "cap_blue": (2, 1), "f2048_m256": (2, 2), "f400_m256": (1, 8)}

# geometries abd_mfcc_plan_create refuses: name -> (Case, piece of the error message)
REFUSED = {
    "blue_3073": (Case(16000, 3073, 512, 4000, 64, 13, H, R, 80.0, 1, 0), "too large"),    # 2 * 3073 - 1 > 6144
    "smooth_6250": (Case(16000, 6250, 512, 4000, 64, 13, H, R, 80.0, 1, 0), "too large"),  # 2 * 5^5 > 6144
    "len_half": (Case(16000, 60, 7, 30, 20, 13, H, R, 80.0, 1, 0), "too short"),           # L = n_fft / 2
    "mels_257": (Case(16000, 1024, 100, 750, 257, 13, H, R, 80.0, 1, 0), "n_mels > 256"),
    "mfcc_over_mels": (Case(16000, 256, 100, 650, 20, 21, H, R, 80.0, 1, 0), "bad MFCC geometry"),
    "fft_one": (Case(16000, 1, 1, 8, 1, 1, H, R, 80.0, 1, 0), "bad MFCC geometry"),
    "hop_zero": (Case(16000, 256, 0, 650, 20, 13, H, R, 80.0, 1, 0), "bad MFCC geometry"),
}

# one case per DCT kernel for the ragged rows (abd_inject.frames); frames of the six batch rows from T
RAGGED = ("c49", "c52", "c13", "c17", "c48")            # plain, lds, mfma1, mfma2, mfma3


def ragged_frames(T):
    return np.array([0, 1, T - 1, T, T + 5, -3], dtype=np.int32)


PATCH = ("c52", (3, 11, 5, 23, -200.0))                 # lds kernel: the coefficient window starts and ends off a 4
INJECT = ("chunk_ragged", "f400_m256")                  # one generic and one specialised plan
TRIG_LEN = 300

# case -> bound of the device result where float32 on the CPU misses 1e-5: ten times the measured float32-CPU
# distance (tests/test_mfcc_envelope_cpu.py asserts the tenth).  Everything else: the project's 1e-4.
BOUNDS: dict = {}


def bound(name):
    return BOUNDS.get(name, 1e-4)


def stockham_radices(M):
    """The runtime-radix plan of a {2,3,5}-smooth M: 4s, then a 2, then 3s, then 5s."""
    r = []
    for f, stop in ((4, 4), (2, 2), (3, 3), (5, 5)):
        while M % stop == 0:
            r.append(f)
            M //= f
    assert M == 1
    return r


def signal(B, L, sr, seed):
    """(B, L) float32: broadband noise plus two tones per row, rows at falling levels (1, 0.3, 0.05, 0.01),
    the second half of row 1 another 100 dB down so the top_db clamp is active there.  Noise in every bin
    keeps the un-clamped low-energy values well conditioned."""
    r = np.random.Generator(np.random.PCG64(7000 + seed))
    t = np.arange(L) / sr
    w = 0.25 * r.standard_normal((B, L))
    f1 = r.uniform(200.0, sr / 4, B)
    f2 = r.uniform(sr / 4, sr / 2.2, B)
    ph = r.uniform(0, 2 * math.pi, B)
    w += 0.2 * np.sin(2 * math.pi * f1[:, None] * t + ph[:, None]) + 0.1 * np.sin(2 * math.pi * f2[:, None] * t)
    w *= np.array([1.0, 0.3, 0.05, 0.01])[:B, None]
    if B > 1:
        w[1, L // 2:] *= 1e-5
    return w.astype(np.float32)


def make_waves(name):
    """The clips of a case: signal(), or zeros for the ZERO cases."""
    c = CASES[name]
    if name in ZERO:
        return np.zeros((c.B, c.L), dtype=np.float32)
    return signal(c.B, c.L, c.sr, c.seed)


def _power(wave, c, dtype):
    """|STFT|^2 (B, n_freqs, T): oracle.mfcc.stft_power in float64; the same steps in float32 on torch's CPU FFT."""
    if dtype == np.float64:
        return om.stft_power(wave.astype(np.float64), c.n_fft, c.hop, c.pad)
    pad = c.n_fft // 2
    xp = np.pad(wave.astype(np.float32), ((0, 0), (pad, pad)), mode=c.pad)
    T = om.n_frames(wave.shape[1], c.n_fft, c.hop)
    idx = np.arange(T)[:, None] * c.hop + np.arange(c.n_fft)[None, :]
    frames = xp[:, idx] * om.hann_periodic(c.n_fft).astype(np.float32)[None, None, :]
    spec = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(frames)), dim=-1)
    assert spec.dtype == torch.complex64
    p = (spec.real ** 2 + spec.imag ** 2).numpy()
    return np.transpose(p, (0, 2, 1))


def restated(wave, c, dtype=np.float64, frames=None, frame_pad=-200.0):
    """wave (B, L) -> the model input (B, 1, T, n_mfcc) in ``dtype``; frames (B,) = valid frames per row
    (clamped to [0, T]) or None."""
    p = _power(wave, c, dtype)
    nfreq = c.n_fft // 2 + 1
    if c.mel == "htk":
        fb = om.htk_mel_fbanks(nfreq, 0.0, float(c.sr // 2), c.n_mels, c.sr)
    else:
        fb = om.slaney_mel_fbanks(c.sr, c.n_fft, c.n_mels)
    mel = np.einsum("bft,fm->bmt", p, fb.astype(dtype))
    db = (10.0 * np.log10(np.maximum(mel, dtype(1e-10)))).astype(dtype)
    B, _, T = db.shape
    nv = np.full(B, T) if frames is None else np.clip(np.asarray(frames), 0, T)
    if c.top_db >= 0:
        for u in range(B):
            if nv[u] > 0:
                db[u] = np.maximum(db[u], db[u, :, :nv[u]].max() - dtype(c.top_db))
    out = np.einsum("bmt,mc->btc", db, om.dct_ortho(c.n_mfcc, c.n_mels).astype(dtype))
    assert out.dtype == dtype
    for u in range(B):
        out[u, nv[u]:] = frame_pad
    return out[:, None]


def distance(got, ref, frames=None):
    """max |err| of every (utterance, frame) over the utterance's max |MFCC| (its valid frames), as
    tests/test_gpu_mfcc_scale.py measures it: (B, T).  Frames past a ragged row's end must be equal: inf if not."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    B, _, T, _ = ref.shape
    nv = np.full(B, T) if frames is None else np.clip(np.asarray(frames), 0, T)
    err = np.abs(got - ref)[:, 0].max(axis=2)
    rel = np.zeros((B, T))
    for u in range(B):
        if nv[u] > 0:
            rel[u, :nv[u]] = err[u, :nv[u]] / np.abs(ref[u, 0, :nv[u]]).max()
        rel[u, nv[u]:] = np.where(err[u, nv[u]:] == 0.0, 0.0, np.inf)
    return rel


def zero_expected(c):
    """The all-zero clip: every mel value at amin, 10 log10 = -100 dB, so c0 = -100 sqrt(n_mels), the rest 0."""
    T = om.n_frames(c.L, c.n_fft, c.hop)
    out = np.zeros((c.B, 1, T, c.n_mfcc))
    out[..., 0] = -100.0 * math.sqrt(c.n_mels)
    return out


def inject_expected(wave, trig, pos, mode, snr_db=30.0):
    """float64 waveform after abd_inject's windowed modes, the window cut at the clip's end: SNR_WINDOW
    x[p:p+Lt] += sqrt(|x|^2 / |t|^2 * 10^(-snr/10)) t (flowmur.py:77-85); DEPLOY s = 10^(30/20) |t| / |x|,
    (s x + t) / (s + 1) inside, s x / (s + 1) outside (utils/flowmur_generate_trigger.py:49-62).  The norms are
    the whole clip's and the whole trigger's."""
    w = np.asarray(wave, np.float64).copy()
    t = np.asarray(trig, np.float64)
    L = w.shape[1]
    tin = np.zeros_like(w)
    for u, p in enumerate(pos):
        n = max(0, min(t.size, L - int(p)))
        tin[u, int(p):int(p) + n] = t[:n]
    wn2, tn2 = (w * w).sum(axis=1), float(t @ t)
    if mode == "snr":
        return w + np.sqrt(wn2 / tn2 * 10.0 ** (-snr_db / 10.0))[:, None] * tin
    s = (10.0 ** (30.0 / 20.0) * math.sqrt(tn2) / np.sqrt(wn2))[:, None]
    return (s * w + tin) / (s + 1.0)


_CACHE: dict = {}


def reference(name, dtype=np.float64):
    """(waves, restated output) of a case, computed once per precision and shared (read only)."""
    key = (name, dtype)
    if key not in _CACHE:
        w = make_waves(name)
        out = restated(w, CASES[name], dtype)
        w.setflags(write=False)
        out.setflags(write=False)
        _CACHE[key] = (w, out)
    return _CACHE[key]
