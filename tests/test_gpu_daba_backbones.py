"""GPU parity: DABA selection on the lstmwithattention and RNN victims -- the per-utterance train-mode forward
against its float64 oracle (tests/daba_backbone_cases.py) and the reference's golden rows, row independence,
agreement with the batched kernel at batch 1, generated masks, certainty / influence and daba_poison_data."""
import glob
import json
import os
import random
import types

import numpy as np
import pytest
import torch

import abd_amd
from abd_amd import daba as D
from abd_amd.models_lstm import lstmwithattention
from abd_amd.models_rnn import RNN
from golden_inputs import rng
from oracle import daba as od
import daba_backbone_cases as dc
import rnn_cases as rc

pytestmark = pytest.mark.gpu
BOUND = 1e-4       # every lstmwithattention parity test's bound against the float64 restatement
RTOL = 1e-4        # tests/test_gpu_daba.py's bound on the scores
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "daba_backbones_golden.npz"))
POOL = np.load(os.path.join(HERE, "golden", "daba_golden.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    abd_amd.load_library()
    return torch.device("cuda", 0)


def build(name, dev):
    B, T, Fd, K, _ = dc.CASES[name]
    m = lstmwithattention(K, Fd, T)
    m.load_state_dict({k: torch.tensor(v) for k, v in dc.make_state(name).items()})
    return m.to(dev)


def build_rnn(dev):
    m = RNN(dc.RNN_CASE[3], dc.RNN_CASE[2])
    m.load_state_dict({k: torch.tensor(v) for k, v in dc.rnn_state().items()})
    return m.to(dev)


def inputs(name, dev):
    x, mask = dc.make_inputs(name)
    return torch.tensor(x, device=dev), torch.tensor(mask, device=dev)


def buffers(m):
    return [b.detach().clone() for b in (m.batchnorm1.running_mean, m.batchnorm1.running_var,
                                         m.batchnorm1.num_batches_tracked, m.batchnorm2.running_mean,
                                         m.batchnorm2.running_var, m.batchnorm2.num_batches_tracked)]


@pytest.mark.parametrize("name", list(dc.CASES))
def test_per_utterance_forward_vs_oracle(dev, name):
    m = build(name, dev)
    x, mask = inputs(name, dev)
    m.engine(x)
    before = buffers(m)
    out = D.SelectionModel(m, dev).outputs(x, masks=(mask,), chunk=128 if name == "chunked" else None)
    err = dc.rel_err(out.cpu(), dc.run_case(name))
    print(f"{name}: per-utterance logits rel err {err:.3e}")
    assert err < BOUND
    assert torch.equal(out.cpu().argmax(1), dc.run_case(name).argmax(1))
    # the selection model is discarded by the reference: no buffer is read or written
    for a, b in zip(before, buffers(m)):
        assert torch.equal(a, b)


def test_golden_rows_on_the_device(dev):
    m = build(dc.GOLDEN_CASE, dev)
    x, _ = inputs(dc.GOLDEN_CASE, dev)
    out = D.SelectionModel(m, dev).outputs(x[:dc.GOLDEN_ROWS].contiguous(), masks=(torch.tensor(GOLD["mask"], device=dev),))
    err = dc.rel_err(out.cpu(), GOLD["logits"])
    print(f"golden rows rel err {err:.3e}")
    assert err < BOUND


def test_rows_do_not_couple(dev):
    """What batch statistics would break: a row's logits are bit-equal whatever else the batch holds."""
    m = build("daba", dev)
    sel = D.SelectionModel(m, dev)
    x, mask = inputs("daba", dev)
    base = sel.outputs(x, masks=(mask,))
    # every other row replaced
    x2 = (x * -0.5 + 3.0).contiguous()
    m2 = (1 - mask).contiguous()
    for i in (0, 1, 8, 16):
        xi, mi = x2.clone(), m2.clone()
        xi[i], mi[i] = x[i], mask[i]
        assert torch.equal(sel.outputs(xi, masks=(mi,))[i], base[i]), i
        assert torch.equal(sel.outputs(x[i:i + 1].contiguous(), masks=(mask[i:i + 1].contiguous(),))[0], base[i]), i
    # the batch permuted
    perm = torch.tensor(np.random.Generator(np.random.PCG64(3)).permutation(x.shape[0]), device=dev)
    assert torch.equal(sel.outputs(x[perm].contiguous(), masks=(mask[perm].contiguous(),)), base[perm])
    # seven identical rows and one constant -200 row (an all-padding clip: zero variance in every channel)
    x8 = x[:1].repeat(8, 1, 1, 1)
    x8[5] = dc.PAD_VALUE
    m8 = mask[:1].repeat(8, 1)
    out = sel.outputs(x8.contiguous(), masks=(m8.contiguous(),))
    assert torch.isfinite(out).all()
    for i in (1, 2, 3, 4, 6, 7):
        assert torch.equal(out[i], out[0]), i
    assert torch.equal(out[0], base[0])
    assert not torch.equal(out[5], out[0])


def test_agrees_with_the_batched_kernel_at_batch_one(dev):
    """abd_lstmattn_forward(train_mode=1) on one row IS a per-utterance forward; only the reduction trees of the
    BatchNorm sums differ, so 1e-5 and not bit equality."""
    m, other = build("daba", dev), build("daba", dev)
    x, mask = inputs("daba", dev)
    out = D.SelectionModel(m, dev).outputs(x, masks=(mask,))
    for i in range(6):
        one = other.hip_forward(x[i:i + 1].contiguous(), train=True, mask=mask[i:i + 1].contiguous())
        err = dc.rel_err(out[i].cpu(), one[0].cpu())
        print(f"row {i}: per-utterance vs batched kernel at B = 1: {err:.3e}")
        assert err < 1e-5, i


def test_generated_masks_are_per_row_and_reproducible(dev):
    m = build("daba", dev)
    sel = D.SelectionModel(m, dev)
    x, _ = inputs("daba", dev)
    x = x[:1].repeat(128, 1, 1, 1).contiguous()
    m._step = 0
    a = sel.outputs(x, seed=123, chunk=64)
    assert m._step == 2                                           # one counter value per chunk
    assert len({tuple(np.round(r, 4)) for r in a[:64].cpu().numpy()}) > 60   # identical clips, independent masks
    m._step = 0
    assert torch.equal(sel.outputs(x, seed=123, chunk=64), a)    # same seed and counter
    assert not torch.equal(a[:64], a[64:])                        # consecutive chunks draw anew
    assert not torch.equal(sel.outputs(x[:64].contiguous(), seed=123), a[:64])   # the counter moved on
    # the generated masks are the documented hash of (seed, counter, row * 64 + unit)
    pinned = sel.outputs(x, masks=(torch.tensor(dc.hash_masks(123, 0, 128, 64), device=dev),))
    assert torch.equal(pinned, a)


def test_rnn_outputs_are_the_eval_forward(dev):
    m = build_rnn(dev)
    x = torch.tensor(dc.rnn_inputs(), device=dev)
    sel = D.SelectionModel(m, dev)
    out = sel.outputs(x)
    assert m.training                                             # the fresh model stays in train mode
    with torch.no_grad():
        want = m.eval()(x)
    m.train()
    assert torch.equal(out, want)
    err = rc.rel_err(out.cpu(), dc.rnn_logits())
    print(f"RNN selection logits rel err {err:.3e}")
    assert err < rc.bound("daba", "logits")
    assert torch.equal(sel.outputs(x, chunk=2), out)              # chunk boundaries and a ragged last chunk
    assert torch.equal(sel.outputs(x, masks=()), out)
    with pytest.raises(abd_amd._lib.AbdError):
        sel.outputs(x, masks=(torch.zeros((5, 64), dtype=torch.uint8, device=dev),))


# ------------------------------------------------------------------ scores
def lstm_oracle(state):
    return lambda x, masks: dc.per_row_logits(state, x, masks[0]).numpy()


def rnn_oracle(state):
    net = rc.Restated(state)

    def f(x, masks):
        with torch.no_grad():
            return net(torch.as_tensor(x, dtype=torch.float64)).numpy()
    return f


def oracle_scores(forward, pool, trig, hosts, pool_masks, trig_masks, pois_masks):
    """(entropy per pool clip, cross entropy per host) with softmax / calc_ent / cross_entropy of oracle/daba.py."""
    xo = np.concatenate([od.selection_input(c) for c in pool])
    ent = np.array([od.calc_ent(p) for p in od.softmax(forward(xo, pool_masks))])
    n = len(hosts)
    xt = np.repeat(od.selection_input(trig), n, axis=0)
    xp = np.concatenate([od.selection_input(od.poisoned_clip(h, trig, -20)) for h in hosts])
    pa, py = od.softmax(forward(xt, trig_masks)), od.softmax(forward(xp, pois_masks))
    return ent, np.array([od.cross_entropy(a, y) for a, y in zip(pa, py)])


def host_clips(r, lengths):
    return [np.clip(r.normal(0, 4000, n), -32768, 32767).astype(np.int16) for n in lengths]


@pytest.mark.parametrize("kind", ["lstmwithattention", "RNN"])
def test_certainty_and_influence_vs_oracle(dev, kind):
    r = rng(13)
    pool = [POOL[f"pool{j}"] for j in range(4)]
    hosts = host_clips(r, (16000, 14000, 9000, 16000, 16000))
    n = len(hosts)
    if kind == "RNN":
        sel, forward = D.DabaSelector(build_rnn(dev), dev), rnn_oracle(dc.rnn_state())
        pm = tm = hm = None
        dev_masks = lambda a: None   # noqa: E731
    else:
        sel, forward = D.DabaSelector(build("daba", dev), dev), lstm_oracle(dc.make_state("daba"))
        pm, tm, hm = [((r.random((k, 64)) < 0.5).astype(np.uint8),) for k in (len(pool), n, n)]
        dev_masks = lambda a: (torch.tensor(a[0], device=dev),)   # noqa: E731
    ref_ent, ref_ce = oracle_scores(forward, pool, pool[1], hosts, pm, tm, hm)
    ent = sel.certainty(pool, masks=dev_masks(pm))
    print(kind, "entropy", ent, ref_ent)
    np.testing.assert_allclose(ent, ref_ent, rtol=RTOL)
    ce = sel.influence(pool[1], hosts, po_db=-20, trig_masks=dev_masks(tm), pois_masks=dev_masks(hm))
    print(kind, "influence", ce, ref_ce)
    np.testing.assert_allclose(ce, ref_ce, rtol=RTOL)


# ------------------------------------------------------------------ daba_poison_data
@pytest.mark.parametrize("kind", ["lstmwithattention", "RNN"])
def test_daba_poison_data_end_to_end(dev, tmp_path, monkeypatch, kind):
    """daba.py --model lstmwithattention / RNN through daba_poison_data on the tree of dc.e2e_make_tree: the chosen
    trigger and hosts are the float64 oracle's (its gaps exceed dc.E2E_GAP, asserted here and on the CPU), the
    written scores are the device's and within RTOL of the oracle's, and the file layout and counts follow the
    reference's bookkeeping."""
    monkeypatch.setattr(glob, "glob", dc.sorted_listing(glob.glob))
    monkeypatch.setattr(D, "load_victim_model", lambda args: dc.e2e_victim(args.model))
    root, pool_dir = dc.e2e_make_tree(tmp_path, [POOL[f"pool{j}"] for j in range(4)])
    out = str(tmp_path / "rec")
    args = types.SimpleNamespace(model=kind, num_classes=10, n_mfcc=40)
    random.seed(dc.E2E_TORCH_SEED)
    torch.manual_seed(dc.E2E_TORCH_SEED)
    trig, hosts = D.daba_poison_data(args, dc.E2E_LABELS, root, out, dc.E2E_TARGET, "Cer&Inf", True, dc.E2E_RATE,
                                     trigger_pool=pool_dir, n_hosts=dc.E2E_HOSTS)
    ref = dc.e2e_oracle(kind, root, pool_dir)
    print(f"{kind}: oracle gaps trigger {ref['gap_t']:.3e} hosts {ref['gap_h']:.3e}")
    assert ref["gap_t"] > dc.E2E_GAP and ref["gap_h"] > dc.E2E_GAP
    # the selection is the oracle's
    assert trig == ref["trigger"]
    assert sorted(hosts) == ref["chosen"] and len(hosts) == ref["k"] == 3
    # the written scores are within RTOL of the oracle's, name by name
    cer = json.load(open(out + "/dict/Cer.json"))
    inf = json.load(open(out + "/dict/Inf_hosts.json"))
    assert list(cer) == ref["names"] and list(inf) == ref["hosts"]
    np.testing.assert_allclose([cer[n] for n in ref["names"]], ref["ent"], rtol=RTOL)
    np.testing.assert_allclose([inf[h] for h in ref["hosts"]], ref["ce"], rtol=RTOL)
    assert trig == min(cer, key=cer.get)                          # rank-1 minimum entropy
    assert sorted(hosts) == sorted(sorted(inf, key=inf.get)[:len(hosts)])   # 'Cer&Inf': the lowest influence
    # ... and are the device's: the same seed, nonce and step counter reproduce them bit for bit
    torch.manual_seed(dc.E2E_TORCH_SEED)
    sel = D.DabaSelector(dc.e2e_victim(kind).to(dev), dev)
    ent = sel.certainty([D.read_wav_int16(n)[0] for n in ref["names"]])
    assert [float(e) for e in ent] == [cer[n] for n in ref["names"]]
    ce = sel.influence(D.read_wav_int16(trig)[0], [D.read_wav_int16(h)[0] for h in ref["hosts"]])
    assert [float(v) for v in ce] == [inf[h] for h in ref["hosts"]]
    # layout and counts: the reference's bookkeeping replayed, as tests/test_gpu_daba.py does
    _, po_random, host_samples, _ = dc.e2e_split(root)
    idx = sorted(dict(zip(host_samples, po_random))[h] for h in hosts)
    expect = all_count = 0
    for lab in dc.E2E_LABELS:
        for _ in D.get_filenames(root + "/" + lab + "/", file_types="*.wav"):
            if lab != dc.E2E_TARGET and expect < len(idx) and all_count == idx[expect]:
                expect += 1
            all_count += 1
    pf = [f for f in os.listdir(out + "/poison/train/" + dc.E2E_TARGET) if f.startswith("poison_")]
    assert len(pf) == expect <= len(hosts)
    assert os.path.exists(out + "/trigger.wav")
    assert len([f for f in os.listdir(out + "/poison/test/" + dc.E2E_TARGET) if f.startswith("poison_")]) > 0
    for lab in dc.E2E_LABELS:
        assert len(os.listdir(out + "/clean/train/" + lab)) == dc.E2E_CLIPS


@pytest.mark.parametrize("kind", ["lstmwithattention", "RNN"])
def test_fresh_victim_scores_are_finite(dev, kind):
    """load_victim_model's own, freshly built model (what daba.py runs) through both selection stages."""
    torch.manual_seed(35)
    m = D.load_victim_model(types.SimpleNamespace(model=kind, num_classes=4, n_mfcc=40)).to(dev)
    sel = D.DabaSelector(m, dev)
    pool = [POOL[f"pool{j}"] for j in range(4)]
    ent = sel.certainty(pool)
    ce = sel.influence(pool[0], host_clips(rng(15), (16000, 9000, 12000)))
    assert ent.shape == (4,) and ce.shape == (3,) and np.isfinite(ent).all() and np.isfinite(ce).all()
    assert np.all(ent > 1.9) and np.all(ent <= 2.0 + 1e-6)       # close to uniform over 4 classes
