"""GPU: the resident trainer's feature cache -- the row gather (abd_gather_rows_f32), the feature
stage's output-row indirection (abd_mfcc_rows_f32) and ResidentTrainer(feature_cache=True) against
the uncached trainer, bit for bit: the MFCC of a table row is a deterministic function of the row."""
import warnings

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import _lib as L
from abd_amd import features as F
from abd_amd import synth
from abd_amd.models import smallcnn
from abd_amd.pipeline import ResidentTrainer, attack_config, ultrasonic_trigger

pytestmark = pytest.mark.gpu

N, B = 12, 5          # 3 steps per epoch, the last one a 2-row tail batch
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    return torch.device("cuda", 0)


# ------------------------------------------------------------------ gather kernel
@pytest.mark.parametrize("T,C", [(100, 40), (32, 13)])
def test_gather_rows(dev, T, C):
    g = torch.Generator().manual_seed(T)
    table = torch.randn((7, 1, T, C), generator=g).to(dev)
    for rows in ([6, 5, 4, 3, 2, 1, 0], [3, 3, 0, 6, 3, 6], [5], []):
        r = torch.tensor(rows, dtype=torch.int32, device=dev)
        out = F.gather_rows(table, r)
        assert out.shape == (len(rows), 1, T, C)
        assert torch.equal(out, table[r.long()])
    # into a caller's buffer, and a leading-rows view of a larger one (the trainer's tail batch)
    buf = torch.full((4, 1, T, C), SENTINEL, device=dev)
    r = torch.tensor([6, 0, 6], dtype=torch.int32, device=dev)
    F.gather_rows(table, r, out=buf[:3])
    assert torch.equal(buf[:3], table[r.long()]) and bool((buf[3] == SENTINEL).all())


def test_gather_rows_rejects_rows_that_are_no_16_byte_multiple(dev):
    table = torch.zeros((3, 1, 3, 5), device=dev)      # 15 floats = 60 B per row
    with pytest.raises(L.AbdError, match="16-byte"):
        F.gather_rows(table, torch.zeros(2, dtype=torch.int32, device=dev))
    F.gather_rows(table, torch.zeros(0, dtype=torch.int32, device=dev))   # n = 0: nothing launched, no error


# ------------------------------------------------------------------ out_rows indirection
def _patch(T, C):
    return (T - 5, T, C - 5, C, -200.0)


# the issue's three plans (ultrasonic 1103/441 Bluestein, badnets 400/160 + patch, daba 2048/512 Slaney), all on
# the MFMA dB/DCT kernel at 128 mels; 52 and 50 coefficients take the LDS and the plain dB/DCT kernels
PLANS = {
    "ultrasonic": (F.MfccConfig(44100, 40, 1103, 441, 44100), False),
    "badnets": (F.MfccConfig(16000, 40, 400, 160, 16000), True),
    "daba": (F.MfccConfig.librosa(16000, 40, 16000), False),
    "lds_kernel": (F.MfccConfig(16000, 52, 400, 160, 16000), True),
    "plain_kernel": (F.MfccConfig(16000, 50, 400, 160, 16000), True),
}


@pytest.mark.parametrize("name", list(PLANS))
def test_out_rows_indirection(dev, name):
    cfg, patch = PLANS[name]
    w, _ = synth.make_clips_torch(6, cfg.sample_rate, cfg.length, 10, seed=5, device=dev)
    rows = torch.tensor([4, 1, 5], dtype=torch.int32, device=dev)
    T = F.get_plan(cfg, dev).n_frames

    def inj():
        if not patch:
            return None
        return F.Injection(poison=torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev), patch=_patch(T, cfg.n_mfcc))
    ref = F.mfcc_batch(w, cfg, rows=rows, inject=inj())
    table = torch.full((9, 1, T, cfg.n_mfcc), SENTINEL, device=dev)
    out_rows = torch.tensor([7, 0, 4], dtype=torch.int32, device=dev)
    got = F.mfcc_batch(w, cfg, rows=rows, inject=inj(), out=table, out_rows=out_rows)
    assert got is table
    assert torch.equal(table[out_rows.long()], ref)
    rest = torch.tensor([1, 2, 3, 5, 6, 8], device=dev)
    assert bool((table[rest] == SENTINEL).all())
    if patch:   # the epilogue followed the indirection: poisoned batch rows 0 and 2 sit in table rows 7 and 4
        t0, t1, c0, c1, v = _patch(T, cfg.n_mfcc)
        assert bool((table[7, 0, t0:t1, c0:c1] == v).all()) and bool((table[4, 0, t0:t1, c0:c1] == v).all())
        assert not bool((table[0, 0, t0:t1, c0:c1] == v).any())


# ------------------------------------------------------------------ trainer
def make_trainer(dev, name, feature_cache, waves=None, **kw):
    cfg = attack_config(name, poisoning_rate=0.5 if name == "flowmur" else 0.34)
    K = 10
    w, labels = synth.make_clips_torch(N, cfg.sample_rate, cfg.length, K, seed=7, device=dev)
    if waves is not None:
        w = waves
    trig = None
    if name == "ultrasonic":
        trig = ultrasonic_trigger(60, "mid", False)
    elif name == "flowmur":
        labels[:6] = cfg.target_label        # clean-label: half of the 6 target-class clips are poisoned
        trig = (0.1 * np.random.default_rng(3).standard_normal(8000)).astype(np.float32)
    torch.manual_seed(35)                    # same initial weights and dropout nonce for both trainers
    model = smallcnn(K, cfg.linear_features).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    return ResidentTrainer(cfg, w, labels, model, opt, B, trigger=trig, seed=35, feature_cache=feature_cache, **kw)


def step_rows(tr):
    """Table rows of the step tr just ran."""
    g, _ = tr._cur
    return tr._epoch[0][tr._pos - g:tr._pos]


def assert_same_state(a, b):
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert sorted(sa) == sorted(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    ea, eb = a.model._engine, b.model._engine
    assert torch.equal(ea.grads, eb.grads)
    assert torch.equal(ea.exp_avg, eb.exp_avg) and torch.equal(ea.exp_avg_sq, eb.exp_avg_sq)
    assert torch.equal(a.metrics, b.metrics)


@pytest.mark.parametrize("name", ["ultrasonic", "flowmur", "jingleback"])
def test_cached_trainer_equals_uncached(dev, name):
    tr_a, tr_b = make_trainer(dev, name, True), make_trainer(dev, name, False)
    assert tr_a.fcache is not None and tr_a.fcache.shape == (tr_a.waves.shape[0], 1, tr_a.T, tr_a.cfg.n_mfcc)
    assert tr_b.fcache is None
    assert int(tr_a.poison.sum()) >= 1
    if name == "jingleback":
        assert tr_a.waves.shape[0] > N       # the styled rows are cache rows of their own
    epochs = 2 if name == "ultrasonic" else 3
    sizes = []
    for k in range(3 * epochs):
        tr_a.step()
        tr_b.step()
        b = step_rows(tr_a).numel()
        sizes.append(b)
        assert torch.equal(step_rows(tr_a), step_rows(tr_b))
        assert torch.equal(tr_a.x[:b], tr_b.x[:b]), (name, k)
        if k == 2:                            # one epoch: every row this epoch visited is cached, and only those
            seen = np.zeros(tr_a.waves.shape[0], bool)
            seen[tr_a._epoch[0].cpu().numpy()] = True
            assert np.array_equal(tr_a.cached, seen) and seen.sum() == N
        if k >= 3:
            assert tr_a._miss[tr_a._step_k] is None   # later epochs only gather
    assert sizes == [5, 5, 2] * epochs
    torch.cuda.synchronize()
    assert_same_state(tr_a, tr_b)
    assert tr_a.read_metrics() == tr_b.read_metrics()


def test_partial_hits_after_an_early_new_epoch(dev):
    tr_a, tr_b = make_trainer(dev, "ultrasonic", True), make_trainer(dev, "ultrasonic", False)
    tr_a.step()
    tr_b.step()
    first = set(step_rows(tr_a).tolist())
    assert int(tr_a.cached.sum()) == 5
    tr_a.new_epoch()                          # the epoch is cut short: 5 rows cached, 7 not
    tr_b.new_epoch()
    tr_a.step()
    tr_b.step()
    rows = step_rows(tr_a).tolist()
    hits = [r for r in rows if r in first]
    assert 0 < len(hits) < 5, (rows, first)   # a batch that mixes hits and misses
    assert sorted(tr_a._miss[0][3].tolist()) == sorted(set(rows) - first)
    assert torch.equal(tr_a.x, tr_b.x)
    assert int(tr_a.cached.sum()) == 5 + (5 - len(hits))
    torch.cuda.synchronize()
    assert_same_state(tr_a, tr_b)


def test_rewriting_the_wave_table_refills_the_cache(dev):
    tr = make_trainer(dev, "ultrasonic", True)
    r0 = None
    for k in range(3):
        tr.step()
        if k == 0:
            r0 = int(step_rows(tr)[0])
    assert tr.cached.all()
    before = tr.fcache[r0].clone()
    tr.waves[r0].mul_(0.5)
    found = False
    for k in range(3):
        tr.step()
        rows = step_rows(tr)
        if k == 0:   # the whole table was dropped and planned again, not just the rewritten row
            assert sum(m[3].size for m in tr._miss if m is not None) == N
            assert int(tr.cached.sum()) == rows.numel()
        at = (rows == r0).nonzero()
        if at.numel():
            found = True
            one = torch.tensor([r0], dtype=torch.int32, device=dev)
            fresh = F.mfcc_batch(tr.waves, tr.mcfg, rows=one,
                                 inject=F.Injection(mode=L.INJECT_ADD, trigger=tr.trigger,
                                                    poison=tr.poison[r0:r0 + 1].contiguous()))
            assert torch.equal(tr.x[int(at[0, 0])], fresh[0])
            assert not torch.equal(fresh[0], before)
    assert found and tr.cached.all()


def test_memory_guard_disables_the_cache(dev):
    with pytest.warns(UserWarning, match="feature cache disabled"):
        tr_a = make_trainer(dev, "flowmur", True, feature_cache_fraction=0.0)
    assert tr_a.fcache is None and tr_a.cached is None
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr_b = make_trainer(dev, "flowmur", False)
        tr_c = make_trainer(dev, "flowmur", True)
    assert tr_c.fcache is not None and not [w for w in rec if "feature cache" in str(w.message)]
    for _ in range(4):
        tr_a.step()
        tr_b.step()
        b = step_rows(tr_a).numel()
        assert torch.equal(tr_a.x[:b], tr_b.x[:b])
    torch.cuda.synchronize()
    assert_same_state(tr_a, tr_b)
