"""Defense scans on the device: the neuron-ablation loop of the reference's defenses as one sweep.

    ft_reg.py:44-55,141-161   get_layerName_from_type / mixed_name     -> neuron_names
    ft_reg.py:125-139         temp_test (loss = mean of batch means)   -> ablation_sweep
    ft_reg.py:173-190         prune_one_neuron + get_loss_change       -> neuron_loss_change
    ft_reg.py:163-171,338-343 pruning() ratio scan, tsbd.py:43-47      -> pruned_eval
    ft_reg.py:83-123          train_finetuning_reg                     -> finetune_reg_epoch
    ft_reg.py:57-81, tsbd.py:140-161  train_finetuning                 -> finetune_epoch

The reference deep-copies the model per neuron, zeroes ``state_dict[layer][idx]`` and runs a whole
DataLoader pass: 160 evaluations per set.  Here every batch is evaluated once for all variants
(torch.ops.abd.smallcnn_ablate_eval): the model is read, never modified or copied, and the data stays
in HBM.  There is no CPU path: CPU tensors raise AbdError.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from .models import PARAM_ORDER, RUNNING_ORDER

LAYERS = (("1", 0, 64), ("2", 64, 64), ("3", 128, 32))   # (suffix, first mask column, channels)
MAX_VARIANTS_PER_PASS = 64


def neuron_names(model=None, layer_type="conv"):
    """'conv1.weight.0' ... 'conv3.weight.31' ('bn...' for layer_type 'bn'): get_layerName_from_type's
    named_modules order with mixed_name's index suffix (ft_reg.py:44-55,141-161).  model is only asked
    for its layers when given (any smallcnn has the same three)."""
    if layer_type not in L.ABLATE_KINDS:
        raise SystemError("NO valid layer_type match!")   # the reference's own error
    if model is not None:
        kind = torch.nn.Conv2d if layer_type == "conv" else torch.nn.BatchNorm2d
        layers = [(n, m.weight.shape[0]) for n, m in model.named_modules() if isinstance(m, kind) and "shortcut" not in n]
    else:
        layers = [(layer_type + s, c) for s, _, c in LAYERS]
    return [f"{n}.weight.{i}" for n, c in layers for i in range(c)]


def mask_column(name: str):
    """'conv2.weight.5' -> ('conv', 69): the layer type and the mask column of one neuron name."""
    parts = name.split(".")
    if len(parts) != 3 or parts[1] != "weight":
        raise ValueError(f"not a neuron name: {name!r}")
    for lt in ("conv", "bn"):
        for s, first, c in LAYERS:
            if parts[0] == lt + s:
                i = int(parts[2])
                if not 0 <= i < c:
                    raise ValueError(f"{name!r}: index out of range (0..{c - 1})")
                return lt, first + i
    raise ValueError(f"not a smallcnn conv / bn layer: {name!r}")


def pack_masks(variants):
    """A list of variants, each a list of neuron names, -> (masks (V, 160) uint8 on the host, kind).
    All names of a sweep are of one layer type (the reference's --layer_type); an all-empty sweep is 'conv'."""
    masks = np.zeros((len(variants), L.ABLATE_CHANNELS), np.uint8)
    kinds = set()
    for v, names in enumerate(variants):
        for n in names:
            lt, col = mask_column(n)
            kinds.add(lt)
            masks[v, col] = 1
    if len(kinds) > 1:
        raise ValueError("one sweep ablates conv filters or bn weights, not both")
    return torch.from_numpy(masks), (kinds.pop() if kinds else "conv")


def batch_bounds(n: int, batch_size: int):
    """[(start, stop)] of a sequential DataLoader(batch_size, drop_last=False) over n rows."""
    return [(s, min(s + batch_size, n)) for s in range(0, n, batch_size)]


def combine(loss_sums, sizes, correct, n: int):
    """temp_test's numbers (ft_reg.py:125-139) from per-batch CE sums: loss = mean over the batches of
    the batch-mean loss (a short last batch weighs as much as a full one), acc = correct / n.
    loss_sums (batches, V) float64, sizes (batches), correct (V)."""
    loss_sums = torch.as_tensor(loss_sums, dtype=torch.float64)
    sizes = torch.as_tensor(sizes, dtype=torch.float64).reshape(-1, 1)
    loss = (loss_sums / sizes).sum(0) / loss_sums.shape[0]
    acc = torch.as_tensor(correct).to(torch.float64) / float(n)
    return loss, acc


def _flat_state(model, device):
    """The model's parameters and BN running statistics as the C ABI's flat fp32 buffers: the bound
    engine's own buffers when the model already lives in them, else packed copies of the VALUES (the
    module itself is left as it is -- no re-homing, no mode change)."""
    eng = getattr(model, "_engine", None)
    if eng is not None and eng.device == device and model._bound(eng):
        return eng.params, eng.running
    sd = model.state_dict()
    params = torch.cat([sd[k].detach().reshape(-1).to(device, torch.float32) for k in PARAM_ORDER])
    running = torch.cat([sd[f"{bn}.{s}"].detach().reshape(-1).to(device, torch.float32)
                         for bn, _ in RUNNING_ORDER for s in ("running_mean", "running_var")])
    return params, running


def _geometry(H0, W0):
    H1, W1p = H0 - 1, (W0 - 1) // 3
    H2, W2 = H1 - 1, W1p - 1
    return H2 // 2 + 1, W2 // 2 + 1   # H2p, W2p


def pick_variants_per_pass(handle, batch: int, n_variants: int, H0: int, W0: int, device) -> int:
    """Variants per pass: as many as half the free HBM holds, at most MAX_VARIANTS_PER_PASS and at most
    what keeps the virtual batch inside the layer-3 kernels' 32-bit offsets."""
    lib = L.lib()
    one = lib.abd_smallcnn_ablate_workspace_bytes(handle, batch, 1)
    per = lib.abd_smallcnn_ablate_workspace_bytes(handle, batch, 2) - one
    free = torch.cuda.mem_get_info(device)[0]
    by_mem = (free // 2 - one) // max(per, 1) + 1
    H2p, W2p = _geometry(H0, W0)
    by_offsets = (0x7ffffff0 - 1) // (batch * H2p * W2p * 256)
    return int(max(1, min(MAX_VARIANTS_PER_PASS, n_variants, by_mem, by_offsets)))


def ablation_sweep(model, x, y, masks, kind="conv", batch_size=256, variants_per_pass=None):
    """temp_test (ft_reg.py:125-139) of every variant at once.  x (N, 1, T, n_mfcc) float32 and y (N)
    int64 are device-resident and batched in the given order; masks (V, 160) uint8 (pack_masks), kind
    'conv' (conv<i>.weight[c] = 0) or 'bn' (bn<i>.weight[c] = 0).  Returns (loss (V), acc (V)) float64
    host tensors: loss the mean over batches of the batch-mean CrossEntropyLoss, acc over the set."""
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    L.require_device(x, "ablation_sweep input")
    L.require_device(y, "ablation_sweep labels")
    if kind not in L.ABLATE_KINDS:
        raise ValueError(f"kind must be one of {sorted(L.ABLATE_KINDS)}, got {kind!r}")
    if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
        raise ValueError("ablation_sweep expects (N, 1, T, n_mfcc) float32")
    masks = torch.as_tensor(masks).detach().to("cpu", torch.uint8).contiguous()
    V, N = int(masks.shape[0]), int(x.shape[0])
    dev = x.device
    params, running = _flat_state(model, dev)
    K = int(model.state_dict()["fc2.weight"].shape[0])
    prec = getattr(model, "gemm_precision", "f32split")
    y = y.to(torch.int64)
    bounds = batch_bounds(N, int(batch_size))
    loss_sums = torch.zeros((max(len(bounds), 1), V), dtype=torch.float64, device=dev)
    correct = torch.zeros(V, dtype=torch.int64, device=dev)
    H0, W0 = int(x.shape[2]), int(x.shape[3])
    for i, (s, e) in enumerate(bounds):
        vpp = variants_per_pass or pick_variants_per_pass(ops._net(H0, W0, K, prec), e - s, V, H0, W0, dev)
        torch.ops.abd.smallcnn_ablate_eval(x[s:e], params, running, y[s:e], masks, L.ABLATE_KINDS[kind], int(vpp),
                                           loss_sums[i], correct, K, prec)
    return combine(loss_sums.cpu(), [e - s for s, e in bounds] or [1], correct.cpu(), max(N, 1))


def neuron_loss_change(model, x, y, layer_type="conv", batch_size=256):
    """get_loss_change (ft_reg.py:179-190) for every neuron of the layer type: (names, loss_change) with
    loss_change[i] = temp_test loss with names[i] zeroed - the unmodified model's loss (float64 numpy)."""
    names = neuron_names(model, layer_type)
    masks, _ = pack_masks([[]] + [[n] for n in names])
    loss, _ = ablation_sweep(model, x, y, masks, layer_type, batch_size)
    return names, (loss[1:] - loss[0]).numpy()


def pruned_eval(model, x, y, ranked_names, ratios, batch_size=256):
    """The pruning() ratio scan (ft_reg.py:163-171,338-343) as one sweep: variant r zeroes the first
    int(ratio_r * len(ranked_names)) neurons of the ranking.  Returns (loss, acc) per ratio (float64 numpy)."""
    ranked_names = list(ranked_names)
    masks, kind = pack_masks([ranked_names[:int(r * len(ranked_names))] for r in ratios])
    loss, acc = ablation_sweep(model, x, y, masks, kind, batch_size)
    return loss.numpy(), acc.numpy()


# ------------------------------------------------------------------ fine-tuning (ft_reg.py:57-123)
def epoch_order(n: int, order):
    """The epoch's row permutation as a host int64 array, or None for sequential order.  It must be a
    permutation of 0..n-1 (a shuffled DataLoader visits every row once)."""
    if order is None:
        return None
    o = torch.as_tensor(order).detach().cpu().numpy() if not isinstance(order, np.ndarray) else order
    if o.ndim != 1 or o.dtype.kind not in "iu":
        raise ValueError("order must be a 1-D integer row permutation")
    o = o.astype(np.int64)
    if len(o) != n or not np.array_equal(np.sort(o), np.arange(n)):
        raise ValueError(f"order must be a permutation of 0..{n - 1}")
    return o


def _epoch_batches(x, y, batch_size, order):
    """[(x_b, y_b)] device batches in the epoch's order: views when sequential, gathers under a permutation."""
    N = int(x.shape[0])
    o = epoch_order(N, order)
    y = y.to(torch.int64)
    bounds = batch_bounds(N, int(batch_size))
    if o is None:
        return [(x[s:e], y[s:e]) for s, e in bounds]
    idx = torch.from_numpy(o).to(x.device)
    return [(x.index_select(0, idx[s:e]), y.index_select(0, idx[s:e])) for s, e in bounds]


def _check_finetune_inputs(model, x, y, what):
    from .models import smallcnn
    L.require_device(x, f"{what} input")
    L.require_device(y, f"{what} labels")
    if not isinstance(model, smallcnn):
        raise L.AbdError(f"{what} runs the abd_amd smallcnn only, got {type(model).__name__}")
    if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32 or y.numel() != x.shape[0]:
        raise ValueError(f"{what} expects x (N, 1, T, n_mfcc) float32 and one label per row")
    if x.shape[0] == 0:
        raise ValueError(f"{what} needs at least one row")


def final_gradients(model):
    """``p.grad``-style views of the engine's flat gradient buffer, in parameter order; also installed as
    the parameters' .grad (the reference assigns ``param.grad = grad``, ft_reg.py:110-112)."""
    from . import training as T
    T.expose_grads(model)
    return [p.grad for p in model._param_list()]


def finetune_reg_epoch(model, x, y, optimizer, r, alpha, batch_size=256, order=None):
    """One epoch of train_finetuning_reg (ft_reg.py:83-123).  x (N, 1, T, n_mfcc) float32 and y (N) are
    device-resident; order is the epoch's row permutation (default: sequential).  optimizer is a
    torch.optim.SGD over the model's parameters (training.SgdBinding).  Every batch is one
    torch.ops.abd.smallcnn_finetune_reg_step: the model is updated in place through its engine and never
    copied.  Returns (loss, acc, final_gradients): the sum of the post-update batch-mean losses over the
    number of batches, correct predictions over samples, and views of the last batch's blended gradient."""
    from . import ops, training as T  # noqa: F401  (registers torch.ops.abd)
    from .models import dropout_seed
    _check_finetune_inputs(model, x, y, "finetune_reg_epoch")
    T.check_sgd(model, optimizer)
    model.train()
    dev = x.device
    eng = model.engine(x)
    sgd = T.SgdBinding(model, optimizer)
    loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
    correct = torch.zeros(1, dtype=torch.int64, device=dev)
    batches = _epoch_batches(x, y, batch_size, order)
    for xb, yb in batches:
        B = int(xb.shape[0])
        m1 = m2 = None
        hm = [model.step_masks(B, dev) for _ in range(3)]   # 'torch_cpu' dropout source: one draw per forward
        if hm[0] is not None:
            m1, m2 = torch.stack([h[0] for h in hm]), torch.stack([h[1] for h in hm])
        torch.ops.abd.smallcnn_finetune_reg_step(
            xb.contiguous(), yb.contiguous(), eng.params, eng.grads, sgd.buf, eng.running, eng.nbt, loss_sum, correct,
            eng.K, float(r), float(alpha), sgd.lr, sgd.momentum, dropout_seed(dev, model), model._step, None, None, m1,
            m2, model.gemm_precision)
        model._step += 3
    loss = float(loss_sum.item()) / len(batches)
    acc = float(correct.item()) / int(x.shape[0])
    return loss, acc, final_gradients(model)


def finetune_epoch(model, x, y, optimizer, batch_size=256, order=None):
    """One epoch of the plain train_finetuning (ft_reg.py:57-81, tsbd.py:140-161) on device-resident
    (x, y): torch.optim.SGD (with or without momentum; a no-update train step, then abd::sgd) or
    torch.optim.Adam (the fused train step).  Returns (loss, acc) like the reference: the sum of the
    batch-mean losses of each step's own pre-update forward over the number of batches, and correct
    predictions over samples (a fraction, not a percentage)."""
    from . import ops, training as T  # noqa: F401  (registers torch.ops.abd)
    _check_finetune_inputs(model, x, y, "finetune_epoch")
    adam = isinstance(optimizer, torch.optim.Adam)
    if adam:
        if not T.fusable(model, optimizer, torch.nn.CrossEntropyLoss()):
            raise L.AbdError("finetune_epoch: this Adam configuration is not the fused step's (one param group over "
                             "the model's parameters, no weight decay / amsgrad / maximize)")
    else:
        T.check_sgd(model, optimizer)
    model.train()
    dev = x.device
    eng = model.engine(x)
    bind = T.AdamBinding(model, optimizer) if adam else T.SgdBinding(model, optimizer)
    metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
    batches = _epoch_batches(x, y, batch_size, order)
    for xb, yb in batches:
        xb, yb = xb.contiguous(), yb.contiguous()
        if adam:
            T.op_train_step(model, xb, yb, None, bind, metrics)
        else:
            T.train_step(model, xb, yb, None, None, metrics, do_update=False)
            torch.ops.abd.sgd(eng.params, eng.grads, bind.buf, None, bind.lr, bind.momentum)
    if adam:
        bind.sync_torch_state()
    T.expose_grads(model)
    loss_sum, total, hit, _, _, _ = T.read_metrics(metrics)
    return loss_sum / len(batches), hit / total
