#!/usr/bin/env python3
"""Golden values of the unlearning correlation analysis from the REFERENCE's own function.

Run on the CPU where the reference checkout exists (ABD_REFERENCE, default /root/reference):
    python tests/golden/make_correlation_golden.py
Route taken: ``correlation_analysis.unlearning_correlation_analysis`` ITSELF runs, in float64, inside a
temporary directory that holds the ``record/`` tree it reads: a pickled reference utils.models.smallcnn
``.double()`` as record/<result>/checkpoint.pt and the four .npy files of tests/correlation_cases.py's
fixture (2 batches of 16 rows, 3 epochs, Adam(1e-3)).  Nothing of the function is restated here.  What the
script arranges around it, in its own process only:
  * seaborn is an empty stand-in module with a no-op ``lmplot``, prepare_dataset is not needed, the
    matplotlib backend is Agg (the scatter plot goes into the temporary directory and is dropped);
  * the function casts its inputs with ``.float()``; the module's ``Data`` name is a stand-in whose
    TensorDataset hands the (float32-representable) rows on as doubles, so the double model runs, and whose
    Subset notes the ``shuffle_indices`` the function drew after its fix_random();
  * ``train_unlearning`` is wrapped to put forward hooks on drop1 / drop2 of each model at its first call
    (the function deep-copies the loaded model itself), which capture the dropout keep-masks;
  * torch.load gets ``weights_only=False`` while the function runs: its checkpoint is a pickled module.
Stored (data only): both per-neuron score vectors exactly as the function wrote them to its CSV, both ucn
texts, the CSV text, the correlation it returned, the masks and the permutation.  Inputs are regenerated
by the tests from tests/correlation_cases.py.
"""
from __future__ import annotations

import functools
import os
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("ABD_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # repository root (oracle/)

import torch  # noqa: E402

seaborn = types.ModuleType("seaborn")
seaborn.lmplot = lambda *a, **k: None
sys.modules["seaborn"] = seaborn
os.environ.setdefault("MPLBACKEND", "Agg")

import correlation_analysis as ca  # noqa: E402
import utils.models as ref_models  # noqa: E402
from correlation_cases import FIXTURE, fixture_inputs  # noqa: E402


def main():
    c = FIXTURE
    assert ca.device.type == "cpu"
    st, cx, cy, bx, by = fixture_inputs(c)
    N, B = c["B"] * c["n_batches"], c["B"]
    flat = st["fc1.weight"].shape[1]
    torch.manual_seed(c["seed"])
    bd_model = ref_models.smallcnn(c["K"], flat).double()
    bd_model.load_state_dict({k: torch.tensor(v) for k, v in st.items()})
    args = types.SimpleNamespace(dataset="fixture", result="fixture_smallcnn", lr_un=c["lr"], batch_size=B,
                                 layer_type="conv", unlearn_epochs=c["epochs"])

    real = ca.Data
    perms = []

    def subset(dataset, indices):
        perms.append(torch.as_tensor(indices).numpy().copy())
        return real.Subset(dataset, indices)

    ca.Data = types.SimpleNamespace(TensorDataset=lambda x, y: real.TensorDataset(x.double(), y), Subset=subset,
                                    DataLoader=real.DataLoader)
    seen, keep = [], {}
    inner = ca.train_unlearning

    def train_unlearning(model, criterion, optimizer, loader):
        if id(model) not in keep:
            seen.append(model)
            k1, k2 = keep.setdefault(id(model), ([], []))
            model.drop1.register_forward_hook(lambda m, i, o: k1.append((o != 0).reshape(o.shape[0], -1).numpy()))
            model.drop2.register_forward_hook(lambda m, i, o: k2.append((o != 0).numpy()))
        return inner(model, criterion, optimizer, loader)

    ca.train_unlearning = train_unlearning
    load = torch.load
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "record", args.result)
        for sub, x, y, tag in (("clean", cx, cy, "clean"), ("bd", bx, by, "bd")):
            d = os.path.join(root, args.dataset, sub)
            os.makedirs(d)
            np.save(os.path.join(d, f"{tag}_test_mfcc.npy"), x)
            np.save(os.path.join(d, f"{tag}_test_label.npy"), y)
        torch.save(bd_model, os.path.join(root, "checkpoint.pt"))
        os.chdir(tmp)
        torch.load = functools.partial(load, weights_only=False)
        try:
            correlation = ca.unlearning_correlation_analysis(args)
        finally:
            torch.load = load
            os.chdir(cwd)
        out_dir = os.path.join(root, "defense", "tsbd", "analysis")
        texts = {}
        for name in ("ucn_cleanunlr.txt", "ucn_bdunlr.txt", "clean_poison_unlearn.csv"):
            with open(os.path.join(out_dir, name), newline="") as f:
                texts[name] = f.read()
        assert sorted(os.listdir(out_dir)) == sorted(list(texts) + [
            "n2w_dict_cleanunlr.pt", "n2w_dict_bdunlr.pt", "unlearned_model_cleanunlr.pt",
            "unlearned_model_bdunlr.pt", "scatter_plot.png"])
        n2w = {t: load(os.path.join(out_dir, f"n2w_dict_{t}.pt"), weights_only=False) for t in ("cleanunlr", "bdunlr")}

    assert len(perms) == 2 and np.array_equal(perms[0], perms[1])
    perm = perms[0]
    assert not np.array_equal(perm, np.arange(N)) and np.array_equal(np.sort(perm), np.arange(N))
    assert len(seen) == 2                                         # model_cleanunlr first, model_bdunlr second
    masks = [keep[id(m)] for m in seen]
    assert all(len(k1) == len(k2) == c["epochs"] for k1, k2 in masks)   # one batch per call
    # the CSV's values are Python sum() over the n2w lists; its text round-trips them (repr)
    rows = [ln.split(",") for ln in texts["clean_poison_unlearn.csv"].splitlines()[1:]]
    scores = np.array([[float(a), float(b)] for a, b in rows]).T
    for col, t in enumerate(("cleanunlr", "bdunlr")):
        assert list(scores[col]) == [sum(v) for v in n2w[t].values()]
    assert len(rows) == 160 and np.isfinite(correlation) and abs(correlation) < 0.999

    arrays = dict(case=np.array([c["H"], c["W"], c["K"], B, c["n_batches"], c["epochs"], c["seed"], c["target"]],
                                np.int64),
                  hyper=np.array([c["lr"]]), perm=perm.astype(np.int64), correlation=np.array(float(correlation)),
                  clean_scores=scores[0], bd_scores=scores[1],
                  ucn_clean=np.frombuffer(texts["ucn_cleanunlr.txt"].encode(), np.uint8),
                  ucn_bd=np.frombuffer(texts["ucn_bdunlr.txt"].encode(), np.uint8),
                  csv=np.frombuffer(texts["clean_poison_unlearn.csv"].encode(), np.uint8))
    for tag, (k1, k2) in zip(("clean", "bd"), masks):
        arrays[f"{tag}_mask1"] = np.packbits(np.stack(k1), axis=-1)
        arrays[f"{tag}_mask2"] = np.packbits(np.stack(k2), axis=-1)
    out = os.path.join(HERE, "correlation_golden.npz")
    np.savez_compressed(out, **arrays)
    print(f"{out}: correlation {float(correlation)!r}, perm[:8] {perm[:8].tolist()}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
