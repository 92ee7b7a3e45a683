"""Fixture of the DABA-selection tests on the LSTM backbones: deterministic cases and their float64 oracle.

The selection forward (utils/daba_selection_tools.py:68-87) runs a train-mode model on ONE clip at a time, so the
oracle of a per-utterance forward is ``lstm_attention_cases.Restated`` in float64, in train mode, applied to each
row as a batch of one with that row's dropout mask: both BatchNorms normalise by the row's own statistics.
tests/test_daba_backbones_cpu.py ties that per-row use of the restatement to the reference's own module through
tests/golden/daba_backbones_golden.npz.  RNN has no BatchNorm and no dropout; its oracle is ``rnn_cases.Restated``.

Per case (numpy-seeded, drawn like lstm_attention_cases: LSTM and dense weights three times wider than torch's
default so the gates saturate): a parameter set under the reference's state_dict names, an MFCC-scale input
(sigma 20) and a keep-mask per row.  Row 1 of every case with T = 32 ends in 12 frames of -200, the padding
``one_sotamax_entropy`` gives a short clip.
"""
from __future__ import annotations

import numpy as np
import torch

import lstm_attention_cases as lc
import rnn_cases as rc
from lstm_attention_cases import Restated, param_shapes, rel_err  # noqa: F401  (re-exported to the tests)

PAD_VALUE, PAD_FRAMES = -200.0, 12

# name -> (B, T, F, K, seed).  The seeds are picked so that the float32 restatement stays within 1e-5 of the float64
# one and every row's top-2 logit gap exceeds 1e-3 of the largest logit (asserted in
# tests/test_daba_backbones_cpu.py).
CASES = {
    "daba": (17, 32, 40, 10, 1),            # DABA's geometry: two batch tiles of the recurrence plus a ragged one
    "classes35": (3, 32, 13, 35, 1),
    "one_feature": (2, 32, 1, 10, 1),       # F = 1
    "wide_feature": (2, 32, 128, 10, 1),    # F at the model's cap
    "short": (2, 7, 13, 10, 1),             # partial conv taps at both ends within one row
    "smallest": (1, 2, 1, 10, 1),           # the smallest legal row (T*F = 2)
    "chunked": (300, 32, 40, 10, 5),        # with chunk=128: chunk boundaries and a ragged last chunk
    "lds_cap": (2, 128, 128, 10, 1),        # T*F at ABD_LSTMATTN_PER_UTTERANCE_MAX_TF: the raised dynamic-LDS limit
}
MAX_TF = 16384          # ABD_LSTMATTN_PER_UTTERANCE_MAX_TF
GOLDEN_CASE, GOLDEN_ROWS = "daba", 6     # rows 0..5 of "daba" run through the reference's module (row 1 is padded)
GOLDEN_TORCH_SEED = 35

RNN_CASE = (5, 32, 40, 10, 1)            # (B, T, F, K, seed): DABA's geometry for RNN


def make_state(name):
    """The case's lstmwithattention state_dict as numpy arrays, drawn like lstm_attention_cases.make_state."""
    B, T, Fd, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(5000 + seed))
    st = {}
    for n, shp in param_shapes(T, Fd, K).items():
        mod, leaf = n.split(".", 1)
        if mod.startswith("batchnorm"):
            v = r.uniform(0.5, 1.5, shp) if leaf == "weight" else r.normal(0.0, 0.3, shp)
        elif mod.startswith("conv"):
            v = r.uniform(-1, 1, shp) / np.sqrt(5 if mod == "conv1" else 50)
        elif mod.startswith("rnn"):
            v = lc.WIDEN * r.uniform(-1, 1, shp) / 8.0
        else:
            fan = shp[1] if leaf == "weight" else {"dense1": 128, "attention": 128, "dense2": T, "dense3": 64,
                                                    "output": 32}[mod]
            v = lc.WIDEN * r.uniform(-1, 1, shp) / np.sqrt(fan)
        st[n] = v.astype(np.float32)
    # a fresh model's buffers: the per-utterance forward must neither read nor write them
    st["batchnorm1.running_mean"] = np.zeros(10, np.float32)
    st["batchnorm1.running_var"] = np.ones(10, np.float32)
    st["batchnorm1.num_batches_tracked"] = np.array(0, dtype=np.int64)
    st["batchnorm2.running_mean"] = np.zeros(1, np.float32)
    st["batchnorm2.running_var"] = np.ones(1, np.float32)
    st["batchnorm2.num_batches_tracked"] = np.array(0, dtype=np.int64)
    return st


def make_inputs(name):
    """x (B,1,T,F) float32 and the dropout keep-masks (B,64) uint8."""
    B, T, Fd, K, seed = CASES[name]
    r = np.random.Generator(np.random.PCG64(6000 + seed))
    x = (20.0 * r.normal(size=(B, 1, T, Fd))).astype(np.float32)
    if T == 32 and B > 1:
        x[1, 0, T - PAD_FRAMES:, :] = PAD_VALUE
    mask = (r.uniform(size=(B, 64)) < 0.5).astype(np.uint8)
    return x, mask


def per_row_logits(state, x, mask, dtype=torch.float64):
    """Restated in train mode on each row as a batch of one with that row's mask -> (B, K)."""
    m = Restated(state, dtype)
    xt, mt = torch.as_tensor(x, dtype=dtype), torch.as_tensor(mask)
    with torch.no_grad():
        return torch.cat([m(xt[i:i + 1], True, mt[i:i + 1]) for i in range(xt.shape[0])])


_CACHE: dict = {}


def run_case(name, dtype=torch.float64):
    """The case's per-utterance logits (B, K), computed once per (case, dtype) and shared (read only)."""
    key = (name, dtype)
    if key not in _CACHE:
        x, mask = make_inputs(name)
        _CACHE[key] = per_row_logits(make_state(name), x, mask, dtype)
    return _CACHE[key]


def min_top2_gap(logits):
    """The smallest top-2 logit gap of a row, relative to the largest logit magnitude."""
    top = logits.topk(2, dim=1).values
    return float(((top[:, 0] - top[:, 1]) / logits.abs().max()).min())


# ------------------------------------------------------------------ RNN
def rnn_state():
    B, T, Fd, K, seed = RNN_CASE
    r = np.random.Generator(np.random.PCG64(7000 + seed))
    return {n: (rc.WIDEN * r.uniform(-1, 1, shp) / np.sqrt(rc.H)).astype(np.float32)
            for n, shp in rc.param_shapes(Fd, K).items()}


def rnn_inputs():
    B, T, Fd, K, seed = RNN_CASE
    r = np.random.Generator(np.random.PCG64(8000 + seed))
    x = (rc.X_SIGMA * r.normal(size=(B, 1, T, Fd))).astype(np.float32)
    x[1, 0, T - PAD_FRAMES:, :] = PAD_VALUE / 10.0   # a padded tail at the RNN fixture's input scale
    return x


def rnn_logits(dtype=torch.float64):
    key = ("rnn", dtype)
    if key not in _CACHE:
        with torch.no_grad():
            _CACHE[key] = rc.Restated(rnn_state(), dtype)(torch.as_tensor(rnn_inputs(), dtype=dtype))
    return _CACHE[key]


# ------------------------------------------------------------------ dropout hash
_M64 = (1 << 64) - 1


def keep_hash(seed, stream, idx):
    """csrc/lstm_attn.hip keep_hash at p = 0.5, restated."""
    z = (seed ^ (stream * 0x9E3779B97F4A7C15 & _M64) ^ (idx * 0xD1B54A32D192ED03 & _M64)) & _M64
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return (z >> 40) / 16777216.0 >= 0.5


def hash_masks(seed, counter, rows, chunk):
    """The masks SelectionModel.outputs generates: the counter advances per chunk, the row index restarts."""
    return np.array([[keep_hash(seed, counter + i // chunk, (i % chunk) * 64 + u) for u in range(64)]
                     for i in range(rows)], dtype=np.uint8)


# ------------------------------------------------------------------ daba_poison_data end to end
# A tiny tree on which the float64 oracle SEPARATES the selection: the gap between the last chosen and the first
# unchosen score exceeds E2E_GAP = 10 x the 1e-4 bound of the scores, so the chosen trigger and hosts can be
# compared with the oracle's.  A freshly built victim cannot give that (its softmax is nearly uniform: the RNN
# oracle's entropies over the pool are 1.99971 .. 1.99975 bits), so the test hands daba_poison_data the widened
# fixture states above in place of load_victim_model's fresh model, with a pinned dropout nonce.  Directory
# listings are sorted for the test, so the split, the hosts and their rows are the same on every file system
# and the gaps asserted on the CPU (tests/test_daba_backbones_cpu.py) are the GPU test's.
E2E_LABELS = ["yes", "no", "up", "down"]
E2E_TARGET, E2E_HOSTS, E2E_RATE, E2E_CLIPS = "up", 16, 0.1, 10
E2E_TREE_SEED = 14
E2E_TORCH_SEED, E2E_NONCE = 35, 20240611
E2E_GAP = 1e-3
E2E_CHUNK = {"lstmwithattention": 2048, "RNN": 192}     # abd_amd.daba.CHUNK: one chunk holds every stage here


def e2e_victim(kind):
    """The fixture-state victim (CPU, train mode) daba_poison_data is handed for --model kind."""
    from abd_amd.models_lstm import lstmwithattention
    from abd_amd.models_rnn import RNN
    if kind == "RNN":
        m, st = RNN(RNN_CASE[3], RNN_CASE[2]), rnn_state()
    else:
        B, T, Fd, K, _ = CASES["daba"]
        m, st = lstmwithattention(K, Fd, T), make_state("daba")
        m._dropout_nonce = E2E_NONCE
    m.load_state_dict({k: torch.tensor(v) for k, v in st.items()})
    return m


def e2e_dropout_seed():
    """abd_amd.models.dropout_seed under torch.manual_seed(E2E_TORCH_SEED) with the pinned nonce."""
    return (E2E_TORCH_SEED + E2E_NONCE * 0x9E3779B97F4A7C15) & ((1 << 63) - 1)


def e2e_make_tree(tmp_path, pool_clips):
    """10 clips per label (1 s or 0.75 s of noise at levels a factor 8 apart) and the pool -> (root, pool dir)."""
    from abd_amd.io import write_wav_int16
    r = np.random.Generator(np.random.PCG64(E2E_TREE_SEED))
    root = tmp_path / "scd"
    for lab in E2E_LABELS:
        (root / lab).mkdir(parents=True)
        for i in range(E2E_CLIPS):
            n = 16000 if i % 3 else 12000
            level = 600.0 * 8.0 ** r.uniform(0.0, 1.0)
            clip = np.clip(r.normal(0, level, n), -32768, 32767).astype(np.int16)
            write_wav_int16(str(root / lab / f"{lab}_{i:02d}.wav"), clip, 16000)
    pool = tmp_path / "pool"
    pool.mkdir()
    for j, c in enumerate(pool_clips):
        write_wav_int16(str(pool / f"music{j}_0.wav"), c, 16000)
    return str(root), str(pool)


def sorted_listing(real_glob):
    """glob.glob with its result sorted (the listing order of a directory differs between file systems)."""
    return lambda *a, **k: sorted(real_glob(*a, **k))


def e2e_split(root):
    """daba_poison_data's bookkeeping up to the host draw, over sorted listings -> (train files, host indices,
    host files, number of hosts to choose)."""
    import os
    import random
    from abd_amd import daba as D
    org = [f for lab in E2E_LABELS for f in sorted(D.glob.glob(os.path.join(root, lab, "*.wav")))]
    random.seed(E2E_TORCH_SEED)
    for f in random.sample(org, int(len(org) * 0.2)):
        org.remove(f)
    idx, hosts = D.my_custom_random(E2E_HOSTS, org, E2E_TARGET)
    return org, idx, hosts, round(E2E_RATE * len(org))


def rel_gap(scores, k):
    """Relative gap between the k-th and the (k+1)-th of the ascending scores."""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    return float((s[k] - s[k - 1]) / abs(s[k]))


def e2e_oracle(kind, root, pool_dir):
    """The float64 selection of daba_poison_data(..., 'Cer&Inf', ...) on the tree: the lowest-entropy pool clip,
    then the hosts of lowest influence.  -> dict(names, ent, trigger, gap_t, hosts, ce, chosen, gap_h)."""
    from abd_amd import daba as D
    from oracle import daba as od
    if kind == "RNN":
        net = rc.Restated(rnn_state())

        def forward(x, mask):
            with torch.no_grad():
                return net(torch.as_tensor(x, dtype=torch.float64)).numpy()
    else:
        def forward(x, mask):
            return per_row_logits(make_state("daba"), x, mask).numpy()
    seed, chunk = e2e_dropout_seed(), E2E_CHUNK[kind]
    names = D.get_filenames(pool_dir, "*.wav")
    pool = [D.read_wav_int16(n)[0] for n in names]
    xo = np.concatenate([od.selection_input(c) for c in pool])
    ent = np.array([od.calc_ent(p) for p in od.softmax(forward(xo, hash_masks(seed, 0, len(pool), chunk)))])
    t = int(np.argmin(ent))
    _, _, hosts, k = e2e_split(root)
    clips = [D.read_wav_int16(h)[0] for h in hosts]
    n = len(hosts)
    both = hash_masks(seed, 1, 2 * n, chunk)       # the same model's second chunk: trigger rows, then hosts
    xt = np.repeat(od.selection_input(pool[t]), n, axis=0)
    xp = np.concatenate([od.selection_input(od.poisoned_clip(h, pool[t], -20)) for h in clips])
    pa, py = od.softmax(forward(xt, both[:n])), od.softmax(forward(xp, both[n:]))
    ce = np.array([od.cross_entropy(a, y) for a, y in zip(pa, py)])
    return {"names": names, "ent": ent, "trigger": names[t], "gap_t": rel_gap(ent, 1), "hosts": hosts, "ce": ce,
            "chosen": sorted(hosts[i] for i in np.argsort(ce)[:k]), "gap_h": rel_gap(ce, k), "k": k}
