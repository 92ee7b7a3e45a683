"""GPU: the JingleBack style boards across the range abd_style_board_create / abd_style_board_apply accept
(tests/style_envelope_cases.py) against oracle.effects.board in float64.

Per case, through the C entry: the clips sit in a table whose rows are longer than the clip with NaN behind
it, gathered through ``rows`` with a repeat; the output rows are longer than the clip with NaN canaries behind
every row and two NaN rows behind the batch; the workspace is filled with a pattern (nothing may read it
before writing it) and has guard bytes behind it.  Every row is within bound(case) of the oracle (max |err|
over the row's max |output|); a second launch is bit-equal; a canonical chain runs again on the generic kernel
(ABD_FX_GENERIC=1) and the two agree to 1e-6.  Pitch boards: the device's phase-wrap decisions at genuine
near-ties are replayed into the oracle, as tests/test_gpu_styles.py does, at most 1e-3 of the bins.  Row
strides of L + 4 and L + 5 and bases 4 bytes off a 16-byte boundary, a plan made for a longer clip, the refused
boards and tensors.

Figures at HEAD on one MI355X: profiles/styles/envelope.md.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import triggers as T
from abd_amd import _lib as L
import style_envelope_cases as sc
from oracle import effects as oe

pytestmark = pytest.mark.gpu
GUARD = 1 << 16
PAT = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    return torch.device("cuda", 0)


def _pad(Ln):
    """NaN floats behind a clip so that rows are a multiple of 4 floats apart (the generic kernel's float4 rows)."""
    return 4 + (-Ln) % 4


def _table(w, dev, tail, lead=0):
    """The clips in rows of lead + L + tail floats, NaN around them; returns (buffer, view of the clips)."""
    t = np.full((w.shape[0], lead + w.shape[1] + tail), np.nan, dtype=np.float32)
    t[:, lead:lead + w.shape[1]] = w
    buf = torch.tensor(t, device=dev)
    return buf, buf[:, lead:lead + w.shape[1]]


def _launch(pb, c, view, rows, dev, plan_len=None, otail=None, olead=0):
    """One guarded launch of ``pb`` through abd_style_board_apply: (n, L) numpy and the workspace."""
    lib = L.lib()
    n, Ln = rows.numel(), c.L
    otail = _pad(Ln) if otail is None else otail
    h = pb._plan(c.sr, Ln if plan_len is None else plan_len, dev)
    need = lib.abd_style_board_workspace_bytes(h, n)
    assert need == sc.workspace_bytes(c.board, c.sr, Ln if plan_len is None else plan_len, n)
    ws = torch.full((need + GUARD,), PAT, dtype=torch.uint8, device=dev)
    obuf = torch.full((n + 2, olead + Ln + otail), float("nan"), device=dev)
    out = obuf[:, olead:olead + Ln]
    L.check(lib.abd_style_board_apply(h, view.data_ptr(), view.stride(0), rows.data_ptr(), n, Ln, out.data_ptr(),
                                      out.stride(0), ws.data_ptr(), need, L.stream_ptr(dev)), "abd_style_board_apply")
    torch.cuda.synchronize()
    assert int((ws[need:] != PAT).sum().item()) == 0, "guard bytes written behind the workspace"
    assert bool(torch.isnan(obuf[n:]).all()), "rows behind the batch written"
    assert bool(torch.isnan(obuf[:n, olead + Ln:]).all()) and bool(torch.isnan(obuf[:n, :olead]).all()), \
        "canaries around an output row written"
    _check_layout(c, ws[:need], n, Ln if plan_len is None else plan_len)
    return out[:n].cpu().numpy(), ws[:need]


def _check_layout(c, ws, n, max_length):
    """Where the launch wrote in the workspace: the pitch regions are laid out by the call's length and the gap
    up to the regions of max_length stays untouched; the reverb buffers sit behind the regions of max_length,
    [buffer word][clip] at a pitch of roundup64(n) -- every word of the n clips written (reset per clip), the
    columns of the padding lanes untouched."""
    used, off = sc.pitch_bytes(c.board, c.sr, c.L, n), sc.pitch_bytes(c.board, c.sr, max_length, n)
    assert int((ws[used:off] != PAT).sum().item()) == 0, "workspace between the pitch regions and the reverb written"
    rf = sc.reverb_floats(c.board, c.sr)
    if rf:
        pitch = (n + 63) // 64 * 64
        words = ws[off:].view(torch.int32).reshape(rf, pitch)
        blank = int.from_bytes(bytes([PAT] * 4), "little", signed=True)
        assert bool((words[:, n:] == blank).all()), "reverb buffer words of the padding lanes written"
        assert bool((words[:, :n] != blank).all()), "reverb buffer words of a clip not written"


def _spectra(ws, c, n):
    """The pitch stage's synthesized spectra Y (n, T, K) complex: workspace offset 0, [clip][frame][bin] float2."""
    r, N, Hs = oe.pitch_params(c.sr, c.board[0][1]["semitones"])
    _, Tf, _ = oe.pitch_frames(c.L, r, Hs)
    K = N // 2 + 1
    y = ws[:n * Tf * K * 8].view(torch.float32).cpu().numpy().reshape(n, Tf, K, 2)
    return y[..., 0] + 1j * y[..., 1]


def _reference(name, rows, ws):
    """(oracle output of the launched rows, replayed decisions, bins)."""
    c = sc.CASES[name]
    w, ref, _ = sc.reference(name)
    if not sc.is_pitch(c.board):
        return ref[rows], 0, 0
    Y = _spectra(ws, c, rows.size)
    if c.gen in ("zero", "zero_ends"):
        # a frame whose window holds exact zeros only has an exactly zero spectrum, also where it shares its FFT
        # with a live frame (the analysis kernel packs frames 2 j and 2 j + 1 into one complex transform)
        r, N, Hs = oe.pitch_params(c.sr, c.board[0][1]["semitones"])
        _, Tf, ia = oe.pitch_frames(c.L, r, Hs)
        live = np.array([[np.any(w[u, max(0, a - N // 2):max(0, min(c.L, a + N // 2))] != 0) for a in ia] for u in rows])
        assert (~live).any() and (c.gen == "zero" or any(live[0, t] != live[0, t + 1] for t in range(0, Tf - 1, 2)))
        assert np.all(Y[~live] == 0), "the spectrum of an all-zero frame is not exactly zero"
    out, nrep = oe.board(w[rows], c.sr, c.board, replay=Y)
    return out, nrep, Y.size


def _check(name, got, ref, what):
    assert got.shape == ref.shape and np.isfinite(got).all(), f"{what}: shape or non-finite output"
    d = float(sc.distance(got, ref).max())
    assert d < sc.bound(name), f"{what}: distance {d:.2e} over {sc.bound(name):.1e}"
    return d


def _run_case(name, dev, monkeypatch):
    c = sc.CASES[name]
    w, _, _ = sc.reference(name)
    rows_np = sc.rows(c)
    rows = torch.tensor(rows_np, device=dev)
    pb = sc.make_board(c.board)
    _, view = _table(w, dev, _pad(c.L))
    got, ws = _launch(pb, c, view, rows, dev)
    ref, nrep, bins = _reference(name, rows_np, ws)
    d = _check(name, got, ref, name)
    line = f"ENVELOPE {name} | {sc.kernel(c.board)} | {d:.2e}"
    if bins:
        assert nrep <= 1e-3 * bins, f"{nrep} replayed decisions of {bins}"
        line += f" | {nrep} of {bins}"
    if name in sc.EXACT:
        assert np.array_equal(got, w[rows_np] if sc.EXACT[name] == "input" else np.zeros_like(got))
    again, _ = _launch(pb, c, view, rows, dev)
    assert np.array_equal(got, again), "two launches differ"
    if c.n is None:
        assert np.array_equal(got[0], got[-1]), "the repeated row differs from itself"
    if sc.canonical(c.board):       # the same chain on the runtime-dispatch kernel
        monkeypatch.setenv("ABD_FX_GENERIC", "1")
        slow, ws2 = _launch(pb, c, view, rows, dev)
        monkeypatch.delenv("ABD_FX_GENERIC")
        d2 = _check(name, slow, ref, f"{name} on the generic kernel")
        gap = float(np.abs(got - slow).max())
        assert gap <= 1e-6 * float(np.abs(slow).max()), f"fast and generic kernels differ by {gap:.2e}"
        line += f" | generic {d2:.2e}"
    print(line)
    return got


@pytest.mark.parametrize("name", list(sc.CASES))
def test_envelope_case(dev, monkeypatch, name):
    _run_case(name, dev, monkeypatch)


VIEWS = ("len8_style5", "plan_phaser", "reverb_room0", "reverb_batch65", "pitch_gain", "plan_pitch_reverb")


@pytest.mark.parametrize("tail", [4, 5])
@pytest.mark.parametrize("name", VIEWS)
def test_row_strides(dev, monkeypatch, name, tail):
    """Rows L + 4 and L + 5 floats apart on both sides (float4 rows where L + 4 is a multiple of 4, scalar rows
    otherwise), on the fast kernel, the generic kernel with a reverb and pitch boards: bit for bit the result of
    the case's own launch, NaN behind every clip unread, the canaries behind every output row untouched."""
    c = sc.CASES[name]
    w, _, _ = sc.reference(name)
    rows = torch.tensor(sc.rows(c), device=dev)
    pb = sc.make_board(c.board)
    base, _ = _launch(pb, c, _table(w, dev, _pad(c.L))[1], rows, dev)
    got, _ = _launch(pb, c, _table(w, dev, tail)[1], rows, dev, otail=tail)
    assert np.array_equal(got, base)
    assert np.isfinite(got).all()


@pytest.mark.parametrize("lead_in,lead_out", [(1, 0), (0, 1), (1, 1), (3, 2)])
def test_rows_off_the_16_byte_grid(dev, monkeypatch, lead_in, lead_out):
    """x[:, 1:] of a padded table: both row strides are multiples of 4 floats and the row pointers are 4 bytes
    off a 16-byte boundary (input, output, both).  board_kernel takes its float4 rows only where the pointers
    allow it; the result is that of the aligned launch."""
    name = "reverb_room0"
    c = sc.CASES[name]
    assert c.L % 4 == 0 and not sc.canonical(c.board)
    w, ref, _ = sc.reference(name)
    rows_np = sc.rows(c)
    rows = torch.tensor(rows_np, device=dev)
    pb = sc.make_board(c.board)
    base, _ = _launch(pb, c, _table(w, dev, 4)[1], rows, dev, otail=4)
    buf, view = _table(w, dev, 4 - lead_in, lead=lead_in)
    assert buf.shape[1] == c.L + 4 and view.stride(0) % 4 == 0 and view.data_ptr() % 16 == 4 * lead_in
    got, _ = _launch(pb, c, view, rows, dev, otail=4 - lead_out, olead=lead_out)
    _check(name, got, ref[rows_np], f"{name} lead {lead_in}/{lead_out}")
    assert np.array_equal(got, base)


@pytest.mark.parametrize("name", sc.PLAN)
def test_plan_larger_than_the_call(dev, monkeypatch, name):
    """max_length 4000 called with L = 1001: the pitch regions are laid out by the call's length, the reverb
    buffers sit behind the regions of max_length.  Bit for bit what a plan created at 1001 gives."""
    c = sc.CASES[name]
    w, _, _ = sc.reference(name)
    rows = torch.tensor(sc.rows(c), device=dev)
    _, view = _table(w, dev, _pad(c.L))
    small, _ = _launch(sc.make_board(c.board), c, view, rows, dev)
    big, _ = _launch(sc.make_board(c.board), c, view, rows, dev, plan_len=sc.PLAN_MAX)
    assert np.array_equal(small, big)
    with pytest.raises(L.AbdError, match="max_length"):
        _launch(sc.make_board(c.board), c, view, rows, dev, plan_len=c.L - 1)


def _create(fx, sr=16000, length=64):
    arr = (L.Effect * max(len(fx), 1))()
    for i, (kind, p) in enumerate(fx):
        arr[i].kind = kind
        for j, v in enumerate(p):
            arr[i].p[j] = v
    h = C.c_void_p()
    rc = L.lib().abd_style_board_create(arr, len(fx), sr, length, C.byref(h))
    return rc, h


NAN, INF = float("nan"), float("inf")
# (effect kind, parameters) abd_style_board_create refuses, piece of the message, the nearest accepted parameters
REFUSED_FX = {
    "ladder_drive_zero": ((L.FX_LADDER, [1, 1000.0, 0.5, 0.0]), b"LadderFilter", [1, 1000.0, 0.5, 1e-3]),
    "ladder_drive_negative": ((L.FX_LADDER, [1, 1000.0, 0.5, -1.0]), b"LadderFilter", [1, 1000.0, 0.5, 1e-3]),
    "ladder_cutoff_nan": ((L.FX_LADDER, [1, NAN, 0.5, 1.0]), b"LadderFilter", [1, 0.0, 0.5, 1.0]),
    "ladder_resonance_inf": ((L.FX_LADDER, [1, 1000.0, INF, 1.0]), b"LadderFilter", [1, 1000.0, 1.5, 1.0]),
    "gain_nan": ((L.FX_GAIN, [NAN]), b"Gain", [-120.0]),
    "gain_inf": ((L.FX_GAIN, [INF]), b"Gain", [300.0]),
    "gain_overflow": ((L.FX_GAIN, [800.0]), b"Gain", [760.0]),            # 10^40 is past float
    "distortion_nan": ((L.FX_DISTORTION, [NAN]), b"Distortion", [60.0]),
    "phaser_centre_nan": ((L.FX_PHASER, [1.0, 0.5, NAN, 0.0, 0.5]), b"Phaser", [1.0, 0.5, 0.0, 0.0, 0.5]),
    # a huge finite rate: the LFO's phase reduction must end (fmod, not a subtraction that no longer moves a float)
    "phaser_rate_inf": ((L.FX_PHASER, [INF, 0.5, 1300.0, 0.0, 0.5]), b"Phaser", [1e30, 0.5, 1300.0, 0.0, 0.5]),
    "chorus_rate_inf": ((L.FX_CHORUS, [INF, 0.25, 7.0, 0.0, 0.5]), b"Chorus", [1e30, 0.25, 7.0, 0.0, 0.5]),
    "phaser_mix_nan": ((L.FX_PHASER, [1.0, 0.5, 1300.0, 0.0, NAN]), b"Phaser", [1.0, 0.5, -5.0, 0.0, 1.5]),
    "chorus_depth_inf": ((L.FX_CHORUS, [1.0, INF, 7.0, 0.0, 0.5]), b"Chorus", [1.0, 5.0, 7.0, 0.0, 0.5]),
    "chorus_centre_nan": ((L.FX_CHORUS, [1.0, 0.25, NAN, 0.0, 0.5]), b"Chorus", [1.0, 0.25, 1e6, 0.0, 0.5]),
    "reverb_room_nan": ((L.FX_REVERB, [NAN, 0.5, 0.33, 0.4, 1.0, 0.0]), b"Reverb", [2.0, 0.5, 0.33, 0.4, 1.0, 0.0]),
    "reverb_freeze_nan": ((L.FX_REVERB, [0.5, 0.5, 0.33, 0.4, 1.0, NAN]), b"Reverb", [0.5, 0.5, 0.33, 0.4, 1.0, 0.49]),
    "pitch_nan": ((L.FX_PITCHSHIFT, [NAN]), b"PitchShift", [24.0]),
    "pitch_past_24": ((L.FX_PITCHSHIFT, [24.001]), b"PitchShift", [-24.0]),
}


@pytest.mark.parametrize("name", list(REFUSED_FX))
def test_refused_parameters_and_their_accepted_neighbours(dev, name):
    """A parameter that is not finite, or that makes a coefficient or a table entry not finite, is refused with
    ABD_E_INVALID naming the effect and no board comes back; the nearest accepted value creates a board and runs
    to a finite result (finite values outside JUCE's debug assertions are accepted, as JUCE's release build does)."""
    (kind, bad), msg, good = REFUSED_FX[name]
    with torch.cuda.device(dev):
        rc, h = _create([(kind, bad)])
        assert rc == 1001 and h.value is None, (rc, L.lib().abd_last_error())
        assert msg in L.lib().abd_last_error(), L.lib().abd_last_error()
        rc, h = _create([(kind, good)])
        assert rc == 0 and h.value is not None, L.lib().abd_last_error()
        lib = L.lib()
        try:
            x = torch.tensor(sc.clips(2, 64, 16000, 5) * 0.1, device=dev)
            need = lib.abd_style_board_workspace_bytes(h, 2)
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            out = torch.full((2, 64), float("nan"), device=dev)
            rc = lib.abd_style_board_apply(h, x.data_ptr(), 64, None, 2, 64, out.data_ptr(), 64, ws.data_ptr(), need,
                                           L.stream_ptr(dev))
            torch.cuda.synchronize()
        finally:
            lib.abd_style_board_destroy(h)
    assert rc == 0 and bool(torch.isfinite(out).all())


def test_effect_counts(dev, monkeypatch):
    """Eight effects run (case eight_effects); nine are refused; an empty board copies."""
    x = torch.tensor(sc.clips(2, 100, 16000, 6), device=dev)
    with pytest.raises(L.AbdError, match="bad board parameters"):
        sc.make_board(sc.NINE).apply_device(x, 16000)
    assert torch.equal(sc.make_board([]).apply_device(x, 16000), x)
    assert len(sc.CASES["eight_effects"].board) == 8


def test_reverb_sizes_past_int_at_high_sample_rates(dev):
    """sample_rate * 1617 passes 2^31 from 1.33 MHz: the comb / allpass sizes are formed in 64 bits."""
    sr = 1_400_000
    sizes = [sr * t // 44100 for t in (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617, 556, 441, 341, 225)]
    assert sr * 1617 > 2 ** 31
    with torch.cuda.device(dev):
        rc, h = _create([(L.FX_REVERB, [0.5, 0.5, 0.33, 0.4, 1.0, 0.0])], sr=sr, length=8)
        assert rc == 0, L.lib().abd_last_error()
        try:
            assert L.lib().abd_style_board_workspace_bytes(h, 1) == sum(sizes) * 64 * 4
        finally:
            L.lib().abd_style_board_destroy(h)
    x = sc.clips(2, 8, sr, 7)
    y = sc.make_board([sc.Reverb()]).apply_device(torch.tensor(x, device=dev), sr).cpu().numpy()
    assert sc.distance(y, oe.reverb(x, sr)).max() < 1e-4      # shorter than every comb: the dry signal


def test_apply_device_refuses_views_it_would_misread(dev):
    """Pedalboard.apply_device hands the C entry a row stride only.  A view whose samples are not adjacent is
    refused as not contiguous by require_device, as it was before (nothing new runs here: the test pins it);
    rows that are not contiguous 1-D int32 on the clips' device are refused by apply_device's own check."""
    x = torch.tensor(sc.clips(4, 64, 16000, 8), device=dev)
    pb = sc.make_board(sc.STYLE5)
    good = pb.apply_device(x, 16000)
    for bad in (x[:, ::2], x.T):
        assert bad.stride(1) != 1
        with pytest.raises(L.AbdError, match="contiguous"):
            pb.apply_device(bad, 16000)
    assert torch.equal(pb.apply_device(x[1:3], 16000), good[1:3])          # a row slice is fine
    assert pb.apply_device(x[:, ::2].contiguous(), 16000).shape == (4, 32)
    rows = torch.tensor([3, 0, 3], dtype=torch.int32, device=dev)
    assert torch.equal(pb.apply_device(x, 16000, rows=rows), good[[3, 0, 3]])
    wide = torch.tensor([[3, 9], [0, 9], [3, 9]], dtype=torch.int32, device=dev)
    for bad in (rows.to(torch.int64), rows.cpu(), wide[:, 0], wide):
        with pytest.raises(L.AbdError, match="rows"):
            pb.apply_device(x, 16000, rows=bad)
