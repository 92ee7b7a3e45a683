"""GPU: the MFCC front end across the geometry range abd_mfcc_plan_create accepts (tests/mfcc_envelope_cases.py).

Per case: MfccPlan.describe() names the kernels the case is about (FFT length, radices, specialised or
runtime-radix STFT, mel path, DCT kernel); every utterance and every frame is within the bound of the float64
oracle (max |err| over the utterance's max |MFCC|, as tests/test_gpu_mfcc_scale.py measures it); a second
launch is bit-equal; the guard bytes behind the workspace and the rows behind the output stay untouched.  The
clips sit in a table whose rows are longer than the clip with NaN behind it, gathered through ``rows`` with a
repeat: a read past the clip's end shows up as NaN.  The specialised plans' cases run again on the generic
kernels (ABD_GENERIC_FFT=1).  Then ragged rows on every DCT kernel, the patch epilogue of the LDS kernel,
injection windows that cross the clip's end, the refused geometries, and the MFCC backward on the 400-point
plan against oracle.flowmur.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import features as F
from abd_amd import _lib as L
import mfcc_envelope_cases as mc
from oracle import flowmur as of

pytestmark = pytest.mark.gpu
GUARD = 1 << 20
PAT = 0xA5
TAIL = 5          # NaN floats behind every clip: rows are L + 5 floats apart (not 16-byte multiples)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    return torch.device("cuda", 0)


def _cfg(c):
    return F.MfccConfig(c.sr, c.n_mfcc, c.n_fft, c.hop, c.L, mel=c.mel, pad=c.pad, n_mels=c.n_mels, top_db=c.top_db)


def _table(w, dev):
    t = np.full((w.shape[0], w.shape[1] + TAIL), np.nan, dtype=np.float32)
    t[:, :w.shape[1]] = w
    return torch.tensor(t, device=dev)


def _rows(B):
    return np.array([B - 1] + list(range(B)), dtype=np.int32)   # every row, the last one twice


def _launch(c, table, rows, dev, inject=None):
    """One guarded launch: (n, 1, T, n_mfcc) as numpy."""
    cfg = _cfg(c)
    plan = F.get_plan(cfg, dev)
    n = rows.size
    need = plan.workspace_bytes(n)
    ws = torch.full((need + GUARD,), PAT, dtype=torch.uint8, device=dev)
    out = torch.full((n + 2, 1, plan.n_frames, c.n_mfcc), float("nan"), device=dev)
    F.mfcc_batch(table, cfg, rows=torch.tensor(rows, device=dev), inject=inject, out=out[:n], workspace=ws)
    torch.cuda.synchronize()
    assert int((ws[need:] != PAT).sum().item()) == 0, "guard bytes written behind the workspace"
    assert bool(torch.isnan(out[n:]).all()), "rows behind the batch written"
    return out[:n].cpu().numpy()


def _check_path(c, dev, want, chunks=None):
    d = F.get_plan(_cfg(c), dev).describe()
    got = mc.Expect(d["fft_size"], d["bluestein"], d["fast"], d["mel_path"], d["dct_kernel"])
    assert got == want, d
    assert d["radices"] == mc.stockham_radices(want.fft_size) and int(np.prod(d["radices"])) == want.fft_size
    assert d["n_frames"] == 1 + (c.L + 2 * (c.n_fft // 2) - c.n_fft) // c.hop
    assert d["chunks"] * d["ppb"] >= (d["n_frames"] + 1) // 2 > (d["chunks"] - 1) * d["ppb"]
    if chunks is not None:
        assert (d["chunks"], d["ppb"]) == chunks, d
    return d


def _check(got, ref, name, what, frames=None):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    rel = mc.distance(got, ref, frames)
    worst = float(rel.max())
    print(f"{what}: worst distance {worst:.2e} (bound {mc.bound(name):.0e})")
    bad = np.argwhere(rel >= mc.bound(name))
    assert bad.size == 0, f"{what}: {len(bad)} frames over {mc.bound(name)} (first {bad[:5].tolist()}, max {worst:.2e})"
    return worst


def _run_case(name, dev, want, chunks=None):
    c = mc.CASES[name]
    d = _check_path(c, dev, want, chunks)
    w, ref = mc.reference(name)
    rows = _rows(c.B)
    table = _table(w, dev)
    got = _launch(c, table, rows, dev)
    if name in mc.ZERO:   # the exact answer, compared absolutely against the bound times its magnitude
        err = float(np.abs(got - mc.zero_expected(c)[rows]).max())
        print(f"{name}: max abs err {err:.2e} of {100.0 * np.sqrt(c.n_mels):.0f}")
        assert err < mc.bound(name) * 100.0 * np.sqrt(c.n_mels)
    else:
        _check(got, ref[rows], name, f"{name} [{d['mel_path']}, {d['dct_kernel']}]")
    again = _launch(c, table, rows, dev)
    assert np.array_equal(got, again), "two launches differ"
    assert np.array_equal(got[0], got[-1]), "the repeated row differs from itself"


@pytest.mark.parametrize("name", list(mc.CASES))
def test_envelope_case(dev, name):
    _run_case(name, dev, mc.EXPECT[name], mc.CHUNKS.get(name))


@pytest.mark.parametrize("name", list(mc.FAST))
def test_fast_plan_case_on_the_generic_kernels(dev, monkeypatch, name):
    """The specialised plans' cases on the runtime-radix STFT, its mel loop and the plain DCT."""
    monkeypatch.setenv("ABD_GENERIC_FFT", "1")
    F._PLANS.clear()              # the env is read at plan creation
    try:
        e = mc.EXPECT[name]
        _run_case(name, dev, mc.Expect(e.fft_size, e.bluestein, False, "generic", "plain"))
    finally:
        monkeypatch.delenv("ABD_GENERIC_FFT")
        F._PLANS.clear()


@pytest.mark.parametrize("name", list(mc.REFUSED))
def test_refused_geometry(dev, name):
    """abd_mfcc_plan_create refuses with an error code and message; no plan comes back, nothing is launched."""
    c, msg = mc.REFUSED[name]
    h = C.c_void_p()
    with torch.cuda.device(dev):
        rc = L.lib().abd_mfcc_plan_create(c.sr, c.n_fft, c.hop, c.n_mels, c.n_mfcc, L.ABD_MEL_HTK, L.ABD_PAD_REFLECT,
                                          float(c.top_db), c.L, C.byref(h))
    assert rc in (1001, 1002) and h.value is None
    assert msg.encode() in L.lib().abd_last_error(), L.lib().abd_last_error()
    with pytest.raises(L.AbdError, match=msg):
        F.MfccPlan(_cfg(c), dev)


@pytest.mark.parametrize("name", list(mc.RAGGED))
def test_ragged_rows(dev, name):
    """abd_inject.frames = 0, 1, T - 1, T, T + 5 and -3 in one batch: the top_db maximum over the valid frames
    only, the frames behind them at frame_pad exactly -- on the plain, lds and the three MFMA DCT kernels."""
    c = mc.CASES[name]
    d = _check_path(c, dev, mc.EXPECT[name])
    w, _ = mc.reference(name)
    fr = mc.ragged_frames(d["n_frames"])
    rows = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    ref = mc.restated(w[rows], c, np.float64, frames=fr, frame_pad=-123.5)
    inj = F.Injection(frames=torch.tensor(fr, device=dev), frame_pad=-123.5)
    table = _table(w, dev)
    got = _launch(c, table, rows, dev, inject=inj)
    _check(got, ref, name, f"{name} ragged [{d['dct_kernel']}]", frames=fr)
    assert np.array_equal(got, _launch(c, table, rows, dev, inject=inj))


def test_patch_window_off_the_float4_grid(dev):
    """The LDS DCT kernel writes float4 groups of coefficients: a patch whose coefficient window starts and
    ends inside a group, on the poisoned rows only."""
    name, patch = mc.PATCH
    c = mc.CASES[name]
    _check_path(c, dev, mc.EXPECT[name])
    w, ref = mc.reference(name)
    rows = _rows(c.B)
    pois = np.array([1, 0, 1, 1], dtype=np.uint8)
    want = ref[rows].copy()
    want[pois == 1, :, patch[0]:patch[1], patch[2]:patch[3]] = patch[4]
    inj = F.Injection(poison=torch.tensor(pois, device=dev), patch=patch)
    got = _launch(c, _table(w, dev), rows, dev, inject=inj)
    _check(got, want, name, f"{name} patch")
    assert (got[pois == 1][:, :, patch[0]:patch[1], patch[2]:patch[3]] == patch[4]).all()


@pytest.mark.parametrize("mode", ["snr", "deploy"])
@pytest.mark.parametrize("name", list(mc.INJECT))
def test_injection_window_crosses_the_clip_end(dev, name, mode):
    """SNR_WINDOW / DEPLOY windows with pos + trig_len > L, pos = L - 1, pos = 0 and the last position that fits;
    the last batch row is clean.  The trigger has NaN behind it as the clips have."""
    c = mc.CASES[name]
    _check_path(c, dev, mc.EXPECT[name])
    w, _ = mc.reference(name)
    rows = _rows(c.B)
    n = rows.size
    pos = np.array([c.L - 100, c.L - 1, 0, c.L - mc.TRIG_LEN, 5][:n], dtype=np.int32)
    pois = np.ones(n, dtype=np.uint8)
    pois[-1] = 0
    r = np.random.Generator(np.random.PCG64(99 + c.seed))
    tbuf = np.full(mc.TRIG_LEN + 8, np.nan, dtype=np.float32)
    tbuf[:mc.TRIG_LEN] = r.uniform(-0.2, 0.2, mc.TRIG_LEN)
    trig = torch.tensor(tbuf, device=dev)[:mc.TRIG_LEN]
    exp = w[rows].astype(np.float64)
    mixed = mc.inject_expected(exp, tbuf[:mc.TRIG_LEN], pos, mode, 30.0)
    exp[pois == 1] = mixed[pois == 1]
    ref = mc.restated(exp, c, np.float64)
    inj = F.Injection(mode=L.INJECT_SNR_WINDOW if mode == "snr" else L.INJECT_DEPLOY, trigger=trig,
                      position=torch.tensor(pos, device=dev), poison=torch.tensor(pois, device=dev), snr_db=30.0)
    table = _table(w, dev)
    got = _launch(c, table, rows, dev, inject=inj)
    _check(got, ref, name, f"{name} {mode} window")
    wav = F.inject_waveform(table, c.L, inj, rows=torch.tensor(rows, device=dev)).cpu().numpy()
    assert np.abs(wav - exp).max() < 1e-6 * np.abs(exp).max()


# ---------------------------------------------------------------- MFCC backward, 400-point plan
BWD_L, BWD_LT = 1000, 300   # T = 7: three full frame pairs and a lone frame, one item of 8 pairs


def _nrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _bwd_call(plan, wd, B, inj, dd, dt, flags, dev, lt, ws=None):
    lib = L.lib()
    if ws is None:
        ws = torch.empty(lib.abd_mfcc_deploy_backward_workspace_bytes(plan._h, B, lt), dtype=torch.uint8, device=dev)
    return lib.abd_mfcc_deploy_backward(plan._h, wd.data_ptr(), wd.stride(0), None, B, C.byref(inj), dd.data_ptr(),
                                        dt.data_ptr(), flags, ws.data_ptr(), ws.numel(), L.stream_ptr(dev))


@pytest.mark.parametrize("n_mels,n_mfcc", [(40, 13), (128, 40)])
def test_mfcc_deploy_backward_400_matches_oracle(dev, n_mels, n_mfcc):
    """tests/test_gpu_flowmur.py::test_mfcc_deploy_backward_matches_oracle on the 400-point instantiation of
    stft_bwd_kernel: hop 160, a short clip with an odd frame count, the clamp on and off, a loud (clipped)
    and a quiet clip (top_db clamp active), then accumulation.  Same oracle, same bound."""
    B = 4
    w = mc.signal(B, BWD_L, 16000, 60 + n_mels).astype(np.float32)
    w[0] *= 4.0   # samples past +-1 after the mix: the waveform clamp cuts their gradient
    r =np.random.Generator(np.random.PCG64(17 + n_mels))
    t = r.uniform(-0.2, 0.2, BWD_LT).astype(np.float32)
    p = r.integers(0, BWD_L - BWD_LT + 1, B).astype(np.int32)
    p[0], p[1] = 0, BWD_L - BWD_LT
    cfg = F.MfccConfig(16000, n_mfcc, 400, 160, BWD_L, n_mels=n_mels)
    plan = F.get_plan(cfg, dev)
    d = plan.describe()
    assert d["fast"] and d["fft_size"] == 400 and d["bwd_ok"] and d["n_frames"] == 7 and d["mel_path"] == "segmented"
    dout = r.standard_normal((B, 1, 7, n_mfcc)).astype(np.float32)
    wd, td, pd, dd = (torch.tensor(a, device=dev) for a in (w, t, p, dout))
    for mode, clamp in ((L.INJECT_DEPLOY_CLAMP, True), (L.INJECT_DEPLOY, False)):
        inj = F.Injection(mode=mode, trigger=td, position=pd).to_c()
        dt = torch.empty(BWD_LT, device=dev)
        L.check(_bwd_call(plan, wd, B, inj, dd, dt, 0, dev, BWD_LT), "deploy_backward")
        xm, s, tin = of.deploy(w, t, p)
        xc = np.clip(xm, -1, 1) if clamp else xm
        _, cache = of.mfcc_forward(xc, sample_rate=16000, n_mfcc=n_mfcc, n_fft=400, hop=160, n_mels=n_mels)
        ref = of.deploy_backward(of.mfcc_backward(dout, cache), w, t, s, tin, p, xm, clamp=clamp)
        e = _nrel(dt.cpu().numpy(), ref)
        print(f"400-point deploy backward, {n_mels} mels, mode {mode}: rel err {e:.2e}")
        assert e < 1e-4
        L.check(_bwd_call(plan, wd, B, inj, dd, dt, 1, dev, BWD_LT), "deploy_backward")
        assert _nrel(dt.cpu().numpy(), 2 * ref) < 1e-4


def test_mfcc_deploy_backward_refusals(dev):
    """Each returns an error code and launches nothing: a generic plan, T x n_mels past the 64 KiB LDS tile,
    a trigger longer than the clip, ragged rows."""
    lib = L.lib()
    t = torch.zeros(BWD_LT, device=dev)
    p = torch.zeros(2, dtype=torch.int32, device=dev)
    wd = torch.zeros((2, 16000), device=dev)
    dd = torch.zeros(2 * 101 * 40, device=dev)
    dt = torch.full((BWD_LT,), 7.0, device=dev)
    inj = F.Injection(mode=L.INJECT_DEPLOY_CLAMP, trigger=t, position=p).to_c()
    ok = F.get_plan(F.MfccConfig(16000, 13, 400, 160, BWD_L, n_mels=40), dev)
    generic = F.get_plan(F.MfccConfig(16000, 13, 512, 160, BWD_L, n_mels=40), dev)
    assert not generic.describe()["fast"]
    assert _bwd_call(generic, wd, 2, inj, dd, dt, 0, dev, BWD_LT) == 1002 and b"specialised" in lib.abd_last_error()
    big = F.get_plan(F.MfccConfig(16000, 40, 400, 160, 16000), dev)     # 101 frames x 128 mels + the DCT: 72 KB
    assert big.describe()["fast"] and big.describe()["bwd_ok"]
    assert _bwd_call(big, wd, 2, inj, dd, dt, 0, dev, BWD_LT) == 1002 and b"LDS tile" in lib.abd_last_error()
    long_t = torch.zeros(BWD_L + 1, device=dev)
    inj_long = F.Injection(mode=L.INJECT_DEPLOY_CLAMP, trigger=long_t, position=p).to_c()
    assert _bwd_call(ok, wd, 2, inj_long, dd, dt, 0, dev, BWD_L + 1) == 1001 and b"longer than the clip" in lib.abd_last_error()
    fr = torch.tensor([3, 7], dtype=torch.int32, device=dev)
    inj_rag = F.Injection(mode=L.INJECT_DEPLOY_CLAMP, trigger=t, position=p, frames=fr).to_c()
    assert _bwd_call(ok, wd, 2, inj_rag, dd, dt, 0, dev, BWD_LT) == 1002 and b"ragged" in lib.abd_last_error()
    torch.cuda.synchronize()
    assert bool((dt == 7.0).all()), "a refused call wrote the gradient"
