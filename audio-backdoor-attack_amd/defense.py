"""Defense scans on the device: the neuron-ablation loop of the reference's defenses as one sweep.

    ft_reg.py:44-55,141-161   get_layerName_from_type / mixed_name     -> neuron_names
    ft_reg.py:125-139         temp_test (loss = mean of batch means)   -> ablation_sweep
    ft_reg.py:173-190         prune_one_neuron + get_loss_change       -> neuron_loss_change
    ft_reg.py:163-171,338-343 pruning() ratio scan, tsbd.py:43-47      -> pruned_eval
    ft_reg.py:83-123          train_finetuning_reg                     -> finetune_reg_epoch
    ft_reg.py:57-81, tsbd.py:140-161  train_finetuning                 -> finetune_epoch
    tsbd.py:108-138           train_unlearning                         -> unlearn_epoch
    tsbd.py:342-367           NWC scores, ucn.txt, ranking             -> neuron_weight_change, ucn_text, rank_neurons
    tsbd.py:49-63,371-380     zero_reinit_weight and its ratio sweep   -> reinit_models, reinit_sweep
    correlation_analysis.py:41-71,141-143   the unlearning loop          -> unlearn_run
    correlation_analysis.py:128-158  two unlearnings, NWC, Pearson      -> correlation_analysis, correlation_csv,
                                                                           save_correlation_outputs
    fp.py:131-148             hooked activation mean, argsort          -> hidden_activation, rank_units
    fp.py:164-195             prune sweep and its stop rule            -> prune_masks, fc_prune_sweep, prune_stop
    fp.py:52-76,199-210       masked fine-tuning, the whole mitigation -> pruned_finetune_epoch, fine_prune

The reference deep-copies the model per neuron, zeroes ``state_dict[layer][idx]`` and runs a whole
DataLoader pass: 160 evaluations per set.  Here every batch is evaluated once for all variants
(torch.ops.abd.smallcnn_ablate_eval): the model is read, never modified or copied, and the data stays
in HBM.  There is no CPU path: CPU tensors raise AbdError.
"""
from __future__ import annotations

from typing import NamedTuple

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
        _refuse_lstm(model)
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


def _refuse_lstm(model, what="the defences"):
    """The defences are smallcnn's (conv1..conv3 / bn1..bn3 / fc1 / fc2 and the abd_smallcnn_* entry points):
    lstmwithattention, RNN, largecnn, ResNet and smalllstm (reference-built instances included), whose engines look alike
    but whose flat buffers are laid out differently, are refused; every other module is treated as before."""
    from .models_lstm import lstmwithattention
    from .models_rnn import RNN
    from .models_largecnn import largecnn, adoptable
    from .models_resnet import ResNet, adoptable as resnet_adoptable
    from .models_smalllstm import smalllstm, adoptable as smalllstm_adoptable
    if (isinstance(model, (lstmwithattention, RNN, largecnn, ResNet, smalllstm)) or adoptable(model)
            or resnet_adoptable(model) or smalllstm_adoptable(model)):
        raise L.AbdError(f"{what} run the abd_amd smallcnn only, got {type(model).__name__} (DESIGN.md §5)")


def _flat_state(model, device):
    """The model's parameters and BN running statistics as the C ABI's flat fp32 buffers: the bound
    engine's own buffers when the model already lives in them, else packed copies of the VALUES (the
    module itself is left as it is -- no re-homing, no mode change)."""
    _refuse_lstm(model)
    eng = getattr(model, "_engine", None)
    if eng is not None and eng.device == device and model._bound(eng):
        return eng.params, eng.running
    sd = model.state_dict()
    params = torch.cat([sd[k].detach().reshape(-1).to(device, torch.float32) for k in PARAM_ORDER])
    running = torch.cat([sd[f"{bn}.{s}"].detach().reshape(-1).to(device, torch.float32)
                         for bn, _ in RUNNING_ORDER for s in ("running_mean", "running_var")])
    return params, running


def _eval_state(model, device):
    """(params, running, K, precision): what the eval-side ops take of a model."""
    params, running = _flat_state(model, device)
    K = int(model.state_dict()["fc2.weight"].shape[0])
    return params, running, K, getattr(model, "gemm_precision", "f32split")


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
    params, running, K, prec = _eval_state(model, dev)
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


def _batches(x, y, batch_size, order, first_only=False):
    """The device batches of a set in the epoch's order: [x_b] without y, else [(x_b, y_b)] with int64 labels;
    views when sequential, gathers under a permutation.  first_only: the first batch alone."""
    N = int(x.shape[0])
    o = epoch_order(N, order)
    bounds = batch_bounds(N, int(batch_size))[:1 if first_only else None]
    idx = None if o is None else torch.from_numpy(o).to(x.device)

    def rows(t, s, e):
        return t[s:e] if idx is None else t.index_select(0, idx[s:e])
    if y is None:
        return [rows(x, s, e) for s, e in bounds]
    y = y.to(torch.int64)
    return [(rows(x, s, e), rows(y, s, e)) for s, e in bounds]


def _epoch_batches(x, y, batch_size, order):
    """[(x_b, y_b)] device batches in the epoch's order."""
    return _batches(x, y, batch_size, order)


def _x_batches(x, batch_size, order, first_only=False):
    """[x_b]: _epoch_batches without labels."""
    return _batches(x, None, batch_size, order, first_only)


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
    _refuse_lstm(model)
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


# ------------------------------------------------------------------ TSBD (tsbd.py:49-63,108-138,310-380)
REINIT_RATIO = (0.01, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.4, 0.5, 0.7, 0.9)   # tsbd.py:17 reinit_ratio
UCN_HEAD = "No \t Layer_Name \t Neuron_Idx \t Score \n"


def param_offsets(model):
    """Element offsets of the 16 parameter tensors inside the flat buffers (17 entries, parameter order)."""
    _refuse_lstm(model)
    d = dict(model.named_parameters())
    offs = [0]
    for n in PARAM_ORDER:
        offs.append(offs[-1] + d[n].numel())
    return offs


def row_table(model, layer_type="conv"):
    """The C ABI's row table of the layer type's weights as a flat [offset, rows, row_len, ...] list:
    conv<i>.weight as (out channels) rows of in * kh * kw weights, bn<i>.weight as rows of length 1 -- the
    ``view(shape[0], -1)`` of tsbd.py:351 -- in get_layerName_from_type's order."""
    if layer_type not in L.ABLATE_KINDS:
        raise SystemError("NO valid layer_type match!")   # the reference's own error
    offs = param_offsets(model)
    d = dict(model.named_parameters())
    table = []
    for s, _, _ in LAYERS:
        name = f"{layer_type}{s}.weight"
        p = d[name]
        table += [offs[PARAM_ORDER.index(name)], int(p.shape[0]), int(p.numel() // p.shape[0])]
    return table


def _adam_binding(model, optimizer, what):
    from . import training as T
    _refuse_lstm(model, what)
    if not T.fusable(model, optimizer, torch.nn.CrossEntropyLoss()):
        raise L.AbdError(f"{what}: this optimizer is not the device Adam step's (torch.optim.Adam, one param group "
                         "over the model's parameters, no weight decay / amsgrad / maximize)")
    return T.AdamBinding(model, optimizer)


def _adam_epoch(model, eng, adam, batches, own, masks=None):
    """The batch loop that unlearn_epoch and pruned_finetune_epoch share, and what follows it.  Per batch, in this
    order: the dropout masks (masks[i], else one draw of model.step_masks), adam.step += 1, the op, model._step
    += 1.  own() -> (the op, its tensor argument after metrics, its arguments between counter and mask1_in).
    Then the optimizer's torch state and the parameters' .grad; returns read_metrics' numbers."""
    from . import training as T
    from .models import dropout_seed
    dev = eng.device
    metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
    for i, (xb, yb) in enumerate(batches):
        hm = masks[i] if masks is not None else model.step_masks(int(xb.shape[0]), dev)
        op, tensor, after = own()
        adam.step += 1
        op(xb.contiguous(), yb.contiguous(), eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq, eng.running, eng.nbt,
           metrics, tensor, None, None, eng.K, adam.step, adam.lr, adam.betas[0], adam.betas[1], adam.eps,
           dropout_seed(dev, model), model._step, *after, hm[0] if hm is not None else None,
           hm[1] if hm is not None else None, model.gemm_precision)
        model._step += 1
    adam.sync_torch_state()
    T.expose_grads(model)
    return T.read_metrics(metrics)


def unlearn_epoch(model, x, y, optimizer, record_layer="conv3.weight", batch_size=256, order=None, whole_epoch=False):
    """One call of train_unlearning (tsbd.py:108-138, correlation_analysis.py:41-71) on device-resident
    (x, y): gradient ascent on the CrossEntropyLoss with torch.optim.Adam, one
    torch.ops.abd.smallcnn_unlearn_step per batch.  Returns (loss, acc, avg_gradNorm, var_gradNorm).

    The reference's ``return`` sits inside its batch loop: every call trains on the FIRST batch only, yet
    divides the loss by the number of batches and the hits by the size of the whole set, and the variance
    of its single gradient-norm row is NaN.  That is the default here.  whole_epoch=True visits every
    batch (the loop the reference presumably meant), same divisors, mean / unbiased variance over the
    batches' rows.  record_layer None records nothing (correlation_analysis.py's variant): the two
    gradient-norm results are then None.  The parameters' .grad are views of the last batch's gradient
    of -loss, as ``(-loss).backward()`` leaves them."""
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    _check_finetune_inputs(model, x, y, "unlearn_epoch")
    model.train()
    dev = x.device
    eng = model.engine(x)
    adam = _adam_binding(model, optimizer, "unlearn_epoch")
    record = None
    if record_layer is not None:
        d = dict(model.named_parameters())
        if record_layer not in PARAM_ORDER:
            raise ValueError(f"record_layer {record_layer!r} is not a smallcnn parameter")
        p = d[record_layer]
        record = [eng.offsets[PARAM_ORDER.index(record_layer)], int(p.shape[0]), int(p.numel() // p.shape[0])]
    batches = _epoch_batches(x, y, batch_size, order)
    norms = []

    def own():
        norms.append(torch.empty(record[1], dtype=torch.float32, device=dev) if record else None)
        return torch.ops.abd.smallcnn_unlearn_step, norms[-1], (record,)
    loss_sum, _, hit, _, _, _ = _adam_epoch(model, eng, adam, batches if whole_epoch else batches[:1], own)
    loss, acc = loss_sum / len(batches), float(hit) / int(x.shape[0])
    if record is None:
        return loss, acc, None, None
    stack = torch.stack(norms, 0).float()
    return loss, acc, stack.mean(dim=0), stack.var(dim=0)


def _flat_params(src, device):
    """A model, a state dict or a flat tensor -> the flat fp32 parameter buffer on the device."""
    if torch.is_tensor(src):
        return src.detach().reshape(-1).to(device, torch.float32).contiguous()
    sd = src.state_dict() if hasattr(src, "state_dict") else src
    return torch.cat([torch.as_tensor(sd[k]).detach().reshape(-1).to(device, torch.float32) for k in PARAM_ORDER])


def neuron_weight_change(model, original_params, layer_type="conv"):
    """The NWC of tsbd.py:342-363 / correlation_analysis.get_neuron_weight_change: (names, scores, absdiff).
    original_params: the backdoored model before unlearning (a model, a state dict or a flat parameter
    tensor).  names 'conv1.weight.0' ...; scores[i] = sum |p_unlearned - p_original| over neuron i's weights
    (float32 numpy: double accumulation rounded once); absdiff the per-weight changes themselves, the rows of
    all neurons packed in name order, a float32 DEVICE tensor (the reference's n2w_dict values, absdiff_rows)."""
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    eng = getattr(model, "_engine", None)
    if eng is None:
        raise L.AbdError("neuron_weight_change needs a model bound to the device (it has no CPU path)")
    params, _ = _flat_state(model, eng.device)
    orig = _flat_params(original_params, eng.device)
    if orig.numel() != params.numel():
        raise ValueError("original_params does not hold this model's parameters")
    absdiff, sums = torch.ops.abd.row_abs_sums(params.contiguous(), orig, row_table(model, layer_type))
    return neuron_names(model, layer_type), sums.cpu().numpy(), absdiff


def absdiff_rows(model, absdiff, layer_type="conv"):
    """{neuron name: list of its per-weight changes}: the reference's n2w_dict (tsbd.py:356) from packed rows."""
    table = row_table(model, layer_type)
    names = neuron_names(model, layer_type)
    host = torch.as_tensor(absdiff).detach().cpu()
    out, at, i = {}, 0, 0
    for rows, n in zip(table[1::3], table[2::3]):
        for _ in range(rows):
            out[names[i]] = host[at:at + n].tolist()
            at += n
            i += 1
    return out


def ucn_text(names, scores):
    """The text of the reference's ucn.txt (tsbd.py:357-361): header, then one
    '{} \\t {} \\t {} \\t {:.4f} \\n' line per neuron.  Readable by the reference's read_data."""
    lines = [UCN_HEAD]
    for i, (name, s) in enumerate(zip(names, scores)):
        layer, idx = name.rsplit(".", 1)
        lines.append("{} \t {} \t {} \t {:.4f} \n".format(i, layer, idx, float(s)))
    return "".join(lines)


def rank_neurons(text_or_scores):
    """read_data + sorted(key=float(value), reverse=True) (tsbd.py:65-71,366-367): [(layer_name, idx, value)],
    descending by the 4-decimal value of the text, ties in file order (a stable sort).  Takes the ucn text, or
    (names, scores), which go through ucn_text first -- the ranking always sees the rounded values."""
    text = text_or_scores if isinstance(text_or_scores, str) else ucn_text(*text_or_scores)
    rows = []
    for line in text.splitlines()[1:]:
        f = line.split()
        if not f:
            continue
        if len(f) != 4:
            raise ValueError(f"not a ucn line: {line!r}")
        rows.append((f[1], int(f[2]), float(f[3])))
    return sorted(rows, key=lambda r: float(r[2]), reverse=True)


def _ranked_layer_type(ranked):
    kinds = {mask_column(f"{layer}.{idx}")[0] for layer, idx, _ in ranked}
    if len(kinds) != 1:
        raise ValueError("a ranking holds conv filters or bn weights, not both (and not nothing)")
    return kinds.pop()


def reinit_selection(model, ranked, ratios, wratio):
    """(table, row_select (V, rows) uint8, k [V], layer_type) of zero_reinit_weight for each ratio:
    top_num = int(len(ranked) * ratio) neurons selected, k = int(m * wratio) of their m weights.  Raises
    ValueError where the reference's ``min([])`` does (top_num == 0 or k == 0)."""
    ranked = list(ranked)
    lt = _ranked_layer_type(ranked)
    table = row_table(model, lt)
    names = neuron_names(model, lt)
    row_of = {n: i for i, n in enumerate(names)}
    row_len = [n for rows, n in zip(table[1::3], table[2::3]) for _ in range(rows)]
    sel = np.zeros((len(ratios), len(names)), np.uint8)
    ks = []
    for v, ratio in enumerate(ratios):
        top_num = int(len(ranked) * ratio)
        for layer, idx, _ in ranked[:top_num]:
            sel[v, row_of[f"{layer}.{int(idx)}"]] = 1
        m = int(sum(row_len[r] for r in np.nonzero(sel[v])[0]))
        k = int(m * wratio)
        if top_num == 0 or k == 0:
            raise ValueError(f"reinit ratio {ratio}: min() arg is an empty sequence (top_num {top_num}, k {k})")
        ks.append(k)
    return table, sel, ks, lt


def reinit_models(model, ranked, absdiff, ratios, wratio):
    """zero_reinit_weight (tsbd.py:49-63) of the model for every ratio: (params (V, n_params), thr (V), zeroed
    (V)) device tensors.  ranked: rank_neurons' list; absdiff: neuron_weight_change's packed rows.  The model
    is read, never modified; params[v] is a flat parameter buffer for torch.ops.abd.smallcnn_eval*."""
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    L.require_device(absdiff, "absdiff")
    table, sel, ks, _ = reinit_selection(model, ranked, ratios, wratio)
    params, _ = _flat_state(model, absdiff.device)
    params = params.contiguous()
    outs = []
    for s in range(0, len(ks), L.MAX_REINIT_VARIANTS):
        e = s + L.MAX_REINIT_VARIANTS
        outs.append(torch.ops.abd.reinit_weights(params, absdiff, table, torch.from_numpy(sel[s:e]), ks[s:e]))
    return tuple(torch.cat([o[i] for o in outs]) for i in range(3))


def model_with_params(model, flat_params):
    """A deep copy of the smallcnn carrying one variant's flat parameters (BN buffers and settings as the
    model's), unbound: ready for finetune_epoch, which binds it on first use (tsbd.py:373-374,382-394)."""
    import copy
    new = copy.deepcopy(model)
    flat = flat_params.detach().reshape(-1)
    offs = param_offsets(new)
    if flat.numel() != offs[-1]:
        raise ValueError("flat_params does not hold this model's parameters")
    with torch.no_grad():
        for p, o in zip(new._param_list(), offs):
            p.data = flat[o:o + p.numel()].to(p.device, p.dtype).reshape(p.shape).clone()
    return new


def reinit_sweep(model, clean_x, clean_y, bd_x, bd_y, bd_indicator, ranked, absdiff, ratios=REINIT_RATIO, wratio=0.7,
                 batch_size=256):
    """The re-initialisation sweep of tsbd.py:371-380: per ratio (test_clean_acc, test_asr, clean_test_loss,
    bd_test_loss) with training.test's definitions (percentages; the losses are means over the batches of the
    batch-mean loss).  All sets are device-resident; every variant's evaluation is abd_smallcnn_eval on its
    row of reinit_models' parameter sets, the model itself is neither copied nor modified."""
    from . import ops, training as T  # noqa: F401  (registers torch.ops.abd)
    for t, what in ((clean_x, "clean input"), (clean_y, "clean labels"), (bd_x, "backdoor input"),
                    (bd_y, "backdoor labels"), (bd_indicator, "backdoor indicator")):
        L.require_device(t, f"reinit_sweep {what}")
    dev = clean_x.device
    params, _, _ = reinit_models(model, ranked, absdiff, ratios, wratio)
    _, running, K, prec = _eval_state(model, dev)
    clean_y, bd_y, bd_indicator = clean_y.to(torch.int64), bd_y.to(torch.int64), bd_indicator.to(torch.int64)
    return [_test_numbers(params[v], running, K, prec, clean_x, clean_y, bd_x, bd_y, bd_indicator, batch_size)
            for v in range(len(ratios))]


# ------------------------------------------------------------------ correlation_analysis.py:102-158
class CorrelationResult(NamedTuple):
    correlation: float        # df['Clean_unlearn'].corr(df['Poison_unlearn']) (Pearson); NaN for a constant column
    slope: float              # the least-squares line the reference's sns.lmplot draws: Poison_unlearn over
    intercept: float          # Clean_unlearn (no plot is produced here)
    names: list               # 'conv1.weight.0' ...: the rows of both score vectors
    clean_scores: np.ndarray  # float64 per-neuron sums of the clean-unlearned model: the CSV's Clean_unlearn
    bd_scores: np.ndarray     # float64, the poison-unlearned model: the CSV's Poison_unlearn
    ucn_clean: str            # the text of ucn_cleanunlr.txt (the float32 row sums, 4 decimals)
    ucn_bd: str               # the text of ucn_bdunlr.txt
    absdiff_clean: torch.Tensor   # packed per-weight changes (device float32): n2w_dict_cleanunlr.pt's values
    absdiff_bd: torch.Tensor
    model_clean: torch.nn.Module  # model_cleanunlr
    model_bd: torch.nn.Module     # model_bdunlr
    clean_losses: list        # train_unlearning's (loss, acc) of every step, per model
    clean_accs: list
    bd_losses: list
    bd_accs: list
    clean_unlr_loss: float    # the reference's variables of these names after its loop: it assigns BOTH models'
    clean_unlr_acc: float     # return values to them, so they end as the poison-unlearned model's last step
    layer_type: str


def unlearn_run(model, x, y, optimizer, n_steps, batch_size=256, order=None, masks=None):
    """n_steps calls of correlation_analysis.py's train_unlearning (:41-71) in one device call
    (torch.ops.abd.smallcnn_unlearn_run).  Its loaders are unshuffled and the function returns inside its batch
    loop, so every call trains on the same rows: the first batch of ``order`` (default sequential).  Returns
    (losses, accs), one entry per step with the reference's divisors: the batch's mean loss over the NUMBER OF
    BATCHES of the set, the batch's hits over the SIZE of the set.  No record layer.  Afterwards the Adam
    state and the parameters' .grad are as unlearn_epoch leaves them; model._step and the optimizer's step
    count have advanced by n_steps.  masks: an optional (mask1 (n_steps, B, flat), mask2 (n_steps, B, 128))
    pair of uint8 device tensors; with the 'torch_cpu' dropout source the n_steps pairs are drawn up front,
    in step order."""
    from . import ops, training as T  # noqa: F401  (registers torch.ops.abd)
    from .models import dropout_seed
    _check_finetune_inputs(model, x, y, "unlearn_run")
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError(f"unlearn_run needs n_steps >= 1, got {n_steps}")
    model.train()
    dev = x.device
    N = int(x.shape[0])
    n_batches = len(batch_bounds(N, int(batch_size)))
    xb, yb = (t.contiguous() for t in _batches(x, y, batch_size, order, first_only=True)[0])
    eng = model.engine(xb)
    adam = _adam_binding(model, optimizer, "unlearn_run")
    B = int(xb.shape[0])
    if masks is None and getattr(model, "dropout_source", "device") == "torch_cpu":
        drawn = [model.step_masks(B, dev) for _ in range(n_steps)]
        masks = torch.stack([d[0] for d in drawn]), torch.stack([d[1] for d in drawn])
    m1, m2 = masks if masks is not None else (None, None)
    metrics = torch.zeros((n_steps, L.METRICS_WORDS), dtype=torch.int64, device=dev)
    torch.ops.abd.smallcnn_unlearn_run(
        xb, yb, eng.params, eng.grads, eng.exp_avg, eng.exp_avg_sq, eng.running, eng.nbt, metrics, None, None, eng.K,
        n_steps, adam.step + 1, adam.lr, adam.betas[0], adam.betas[1], adam.eps, dropout_seed(dev, model), model._step,
        m1, m2, model.gemm_precision)
    adam.step += n_steps
    model._step += n_steps
    adam.sync_torch_state()
    T.expose_grads(model)
    words = metrics.cpu().numpy()
    loss_sums = np.ascontiguousarray(words[:, 0]).view(np.float64)
    return [float(v) / n_batches for v in loss_sums], [float(h) / N for h in words[:, 2]]


def correlation_stats(clean_scores, bd_scores):
    """(r, slope, intercept) of two score vectors in float64 numpy with abd_nwc_pair_f32's formulas: means, then
    centred sums; r = sxy / sqrt(sxx * syy) (NaN for fewer than 2 rows or a constant column), slope = sxy / sxx
    and intercept = mean_y - slope * mean_x (NaN for a constant x).  Host twin of the device statistics."""
    x, y = np.asarray(clean_scores, np.float64), np.asarray(bd_scores, np.float64)
    if x.shape != y.shape or x.ndim != 1 or x.size == 0:
        raise ValueError("two equally long, non-empty score vectors are needed")
    mx, my = x.mean(), y.mean()
    sxx, syy, sxy = ((x - mx) ** 2).sum(), ((y - my) ** 2).sum(), ((x - mx) * (y - my)).sum()
    r = float("nan") if x.size < 2 or sxx * syy == 0 else float(sxy / np.sqrt(sxx * syy))
    if sxx == 0:
        return r, float("nan"), float("nan")
    slope = float(sxy / sxx)
    return r, slope, float(my - slope * mx)


def correlation_analysis(bd_model, clean_x, clean_y, bd_x, bd_y, *, lr_un=1e-4, unlearn_epochs=1000, batch_size=256,
                         layer_type="conv", order=None, masks=None):
    """unlearning_correlation_analysis (correlation_analysis.py:128-158) on device-resident sets: two deep
    copies of bd_model (read, never modified), torch.optim.Adam(lr_un) for each, unlearn_epochs steps of
    unlearn_run on the clean rows for one and on the backdoor rows for the other -- both over the SAME
    ``order``, as the reference applies one shuffle_indices to both sets (default sequential) -- then one
    torch.ops.abd.nwc_pair call.  masks: optional ((mask1, mask2) of the clean model, (mask1, mask2) of the
    poisoned one), see unlearn_run; by default each copy draws its own dropout stream, as the reference's two
    models draw from one advancing generator.  Returns a CorrelationResult.

    Two quirks of the reference are kept.  Its loop assigns the return values of BOTH models' epochs to
    clean_unlr_loss / clean_unlr_acc: the fields of that name hold the poison-unlearned model's last step (the
    per-step lists hold everything).  Its CSV and correlation are made from Python ``sum()`` over the
    float32-valued per-weight lists -- a sequential DOUBLE sum -- not from the float32 ``sum(dim=-1)`` that the
    ucn text prints: clean_scores / bd_scores are the unrounded double row sums, ucn_* the float32 ones."""
    import copy
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    for t, what in ((clean_x, "clean input"), (clean_y, "clean labels"), (bd_x, "backdoor input"),
                    (bd_y, "backdoor labels")):
        L.require_device(t, f"correlation_analysis {what}")
    if clean_x.shape[0] != bd_x.shape[0]:
        raise ValueError("the clean and the backdoor set hold the same rows (one shuffle_indices serves both)")
    names = neuron_names(bd_model, layer_type)
    if masks is None and getattr(bd_model, "dropout_source", "device") == "torch_cpu":
        # the reference's CPU stream: clean step i draws before poisoned step i (its loop alternates the models)
        B = batch_bounds(int(clean_x.shape[0]), int(batch_size))[0][1]
        drawn = [bd_model.step_masks(B, clean_x.device) for _ in range(2 * int(unlearn_epochs))]
        masks = tuple((torch.stack([d[0] for d in drawn[k::2]]), torch.stack([d[1] for d in drawn[k::2]]))
                      for k in (0, 1))
    per_model = masks if masks is not None else (None, None)
    runs = []
    for (xs, ys), mk in zip(((clean_x, clean_y), (bd_x, bd_y)), per_model):
        m = copy.deepcopy(bd_model)
        m._dropout_nonce = None            # its own mask stream, drawn when it binds
        opt = torch.optim.Adam(m.parameters(), lr=lr_un)
        losses, accs = unlearn_run(m, xs, ys, opt, unlearn_epochs, batch_size, order, mk)
        runs.append((m, losses, accs))
    (mc, lc, ac), (mb, lb, ab) = runs
    dev = clean_x.device
    orig = _flat_params(bd_model, dev)
    ad_c, ad_b, s32_c, s32_b, s64, stats = torch.ops.abd.nwc_pair(orig, mc._engine.params, mb._engine.params,
                                                                  row_table(bd_model, layer_type))
    s64, stats = s64.cpu().numpy(), stats.cpu().numpy()
    return CorrelationResult(float(stats[6]), float(stats[7]), float(stats[8]), names, s64[0].copy(), s64[1].copy(),
                             ucn_text(names, s32_c.cpu().numpy()), ucn_text(names, s32_b.cpu().numpy()), ad_c, ad_b,
                             mc, mb, lc, ac, lb, ab, lb[-1], ab[-1], layer_type)


def correlation_csv(clean_scores, bd_scores):
    """The text of the reference's clean_poison_unlearn.csv (``df.to_csv(index=False)``, :153-156): the header
    Clean_unlearn,Poison_unlearn, then one row per neuron with both values as ``repr(float)``, '\n' line ends."""
    lines = ["Clean_unlearn,Poison_unlearn\n"]
    for c, b in zip(clean_scores, bd_scores):
        lines.append(f"{float(c)!r},{float(b)!r}\n")
    return "".join(lines)


CORRELATION_FILES = ("ucn_cleanunlr.txt", "ucn_bdunlr.txt", "n2w_dict_cleanunlr.pt", "n2w_dict_bdunlr.pt",
                     "unlearned_model_cleanunlr.pt", "unlearned_model_bdunlr.pt", "clean_poison_unlearn.csv")


def save_correlation_outputs(result, directory):
    """The files correlation_analysis.py leaves in its analysis/ folder, under its names (CORRELATION_FILES):
    the two ucn texts, the two n2w dicts {neuron name: list of per-weight changes} (absdiff_rows), the two
    unlearned models' state dicts and the CSV.  No scatter plot: the fitted line's coefficients are
    result.slope / result.intercept.  Returns the paths written."""
    import os
    os.makedirs(directory, exist_ok=True)
    paths = []
    for tag, text, absdiff, model in (("cleanunlr", result.ucn_clean, result.absdiff_clean, result.model_clean),
                                      ("bdunlr", result.ucn_bd, result.absdiff_bd, result.model_bd)):
        p = os.path.join(directory, f"ucn_{tag}.txt")
        with open(p, "w", newline="") as f:
            f.write(text)
        n2w = os.path.join(directory, f"n2w_dict_{tag}.pt")
        torch.save(absdiff_rows(model, absdiff, result.layer_type), n2w)
        sd = os.path.join(directory, f"unlearned_model_{tag}.pt")
        torch.save(model.state_dict(), sd)
        paths += [p, n2w, sd]
    p = os.path.join(directory, "clean_poison_unlearn.csv")
    with open(p, "w", newline="") as f:
        f.write(correlation_csv(result.clean_scores, result.bd_scores))
    return paths + [p]


# ------------------------------------------------------------------ Fine-Pruning (fp.py:131-210)
# The reference hooks the input of the model's LAST child and prunes the first Linear of that child.  Its
# smallcnn's last child is the nn.Softmax() that forward never calls: the hook never fires and mitigation()
# stops with a NameError.  With that unused child deleted from the loaded module the last child is fc2: the
# pruned layer is fc2 and the ranked units are its 128 inputs, relu(fc1(...)) in eval mode.  That is what
# these functions reproduce.
FP_UNITS = L.FCPRUNE_UNITS


def _check_eval_input(x, what):
    L.require_device(x, f"{what} input")
    if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
        raise ValueError(f"{what} expects (N, 1, T, n_mfcc) float32")


def hidden_activation(model, x, batch_size=256, order=None, first_batch_only=True):
    """The activation vector of fp.py:138-146: the eval-mode input of fc2, summed over rows and divided by the
    size of the WHOLE set; a (128,) float32 host tensor.  x (N, 1, T, n_mfcc) float32 is device-resident and
    batched in ``order`` (the shuffled loader's row permutation; default sequential).

    The reference accumulates inside ``if flag == 0:``, so only the FIRST batch contributes while the divisor
    is len(clean_val_set): that is the default.  first_batch_only=False averages every batch.  The sums are
    accumulated in double on the device and rounded to float32 once (the reference sums in float32)."""
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    _check_eval_input(x, "hidden_activation")
    if x.shape[0] == 0:
        raise ValueError("hidden_activation needs at least one row")
    dev = x.device
    params, running, K, prec = _eval_state(model, dev)
    sums = torch.zeros(FP_UNITS, dtype=torch.float64, device=dev)
    for xb in _x_batches(x, batch_size, order, first_only=first_batch_only):
        torch.ops.abd.smallcnn_hidden_sums(xb.contiguous(), params, running, sums, K, prec)
    return (sums / float(x.shape[0])).to(torch.float32).cpu()


def rank_units(activation):
    """seq_sort of fp.py:148: the units in ascending order of their mean activation, a host int64 array.
    The sort is stable (numpy ``kind='stable'``).  Dead ReLU units tie at exactly 0; torch.argsort on the CPU
    is not stable, so the reference's own order among tied units is reproduced only where it agrees with the
    stable one (ascending unit index)."""
    a = torch.as_tensor(activation).detach().cpu().numpy()
    if a.ndim != 1:
        raise ValueError("activation must be one value per unit")
    return np.argsort(a, kind="stable").astype(np.int64)


def prune_masks(seq_sort, once_prune_ratio=0.01):
    """The steps of fp.py:164-171: (num_pruned list, masks (V, n) uint8 host tensor, nonzero = pruned) for
    num_pruned = 0, s, 2s, ... < n with s = ceil(n * once_prune_ratio).  Step num_pruned > 0 prunes
    ``seq_sort[0 : num_pruned - 1]``: one unit fewer than its name says, as the reference's slice does."""
    import math
    seq = np.asarray(seq_sort, dtype=np.int64)
    n = len(seq)
    nums = list(range(0, n, math.ceil(n * once_prune_ratio)))
    masks = np.zeros((len(nums), n), np.uint8)
    for v, num in enumerate(nums):
        if num:
            masks[v, seq[0:num - 1]] = 1
    return nums, torch.from_numpy(masks)


def fc_prune_sweep(model, x, y, masks, batch_size=256):
    """temp_test (fp.py:36-50) of every pruned variant at once: variant v is the eval model with the columns
    masks[v] of fc2.weight removed.  x, y device-resident, batched in the given order; masks (V, 128) uint8.
    Returns (loss (V), acc (V)) float64 host tensors through combine().  One eval forward per batch for all
    variants (torch.ops.abd.smallcnn_fcprune_eval); the model is read, never modified or copied."""
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    _check_eval_input(x, "fc_prune_sweep")
    L.require_device(y, "fc_prune_sweep labels")
    masks = torch.as_tensor(masks).detach().to("cpu", torch.uint8).contiguous()
    V, N = int(masks.shape[0]), int(x.shape[0])
    dev = x.device
    params, running, K, prec = _eval_state(model, dev)
    y = y.to(torch.int64)
    bounds = batch_bounds(N, int(batch_size))
    loss_sums = torch.zeros((max(len(bounds), 1), V), dtype=torch.float64, device=dev)
    correct = torch.zeros(V, dtype=torch.int64, device=dev)
    for i, (s, e) in enumerate(bounds):
        torch.ops.abd.smallcnn_fcprune_eval(x[s:e], params, running, y[s:e], masks, loss_sums[i], correct, K, prec)
    return combine(loss_sums.cpu(), [e - s for s, e in bounds] or [1], correct.cpu(), max(N, 1))


def prune_stop(num_pruned, accs, acc_ratio=0.1):
    """The stop rule of fp.py:187-195 over the sweep's clean accuracies: (steps, last_index, stop_index).
    steps: how many steps the reference's loop runs (the one that broke included); last_index: num_pruned of
    the last step whose accuracy stayed within acc_ratio of the unpruned one; stop_index: num_pruned of the
    step at which the loop ended -- the step that broke, or the last one.  The reference's ``last_net`` aliases
    ``net_pruned``, so the model it fine-tunes carries the mask of stop_index, not of last_index.  An unpruned
    accuracy of 0 divides by zero, as in the reference."""
    last_index = stop_index = 0
    steps = 0
    for num, acc in zip(num_pruned, accs):
        steps += 1
        stop_index = num
        if num == 0:
            ori = acc
            last_index = 0
        if abs(acc - ori) / ori < acc_ratio:
            last_index = num
        else:
            break
    return steps, last_index, stop_index


def pruned_finetune_epoch(model, x, y, optimizer, unit_mask, batch_size=256, order=None, masks=None):
    """One epoch of train_finetuning (fp.py:52-76) with prune.custom_from_mask(fc2, 'weight') active: the
    columns unit_mask (128 values, nonzero = pruned) of fc2.weight are zeroed once, then every batch is one
    torch.ops.abd.smallcnn_pruned_finetune_step (no-update train step, the pruned columns' gradient zeroed,
    torch.optim.Adam).  The pruned columns stay exactly zero: fc2.weight is the effective weight.  masks:
    optional dropout keep-masks per batch [(mask1 (B, flat), mask2 (B, 128))] uint8 device tensors (default:
    the model's dropout source).  Returns (loss, acc): the sum of the batch-mean losses over the number of
    batches and correct predictions over samples."""
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    _check_finetune_inputs(model, x, y, "pruned_finetune_epoch")
    unit = torch.as_tensor(unit_mask).detach().reshape(-1).to("cpu").ne(0)
    if unit.numel() != FP_UNITS:
        raise ValueError(f"unit_mask must hold {FP_UNITS} values")
    model.train()
    dev = x.device
    eng = model.engine(x)
    adam = _adam_binding(model, optimizer, "pruned_finetune_epoch")
    pruned = unit.to(torch.uint8).to(dev)
    with torch.no_grad():
        model.fc2.weight[:, unit.to(dev)] = 0.0
    batches = _epoch_batches(x, y, batch_size, order)
    if masks is not None and len(masks) != len(batches):
        raise ValueError("masks needs one (mask1, mask2) pair per batch")
    loss_sum, total, hit, _, _, _ = _adam_epoch(
        model, eng, adam, batches, lambda: (torch.ops.abd.smallcnn_pruned_finetune_step, pruned, ()), masks)
    return loss_sum / len(batches), hit / total


def _test_numbers(params, running, K, prec, clean_x, clean_y, bd_x, bd_y, bd_indicator, batch_size):
    """training.test's (test_clean_acc, test_asr, clean_test_loss, bd_test_loss) of one flat parameter set on
    device-resident sets (percentages; the losses are means over the batches of the batch-mean loss)."""
    from . import training as T
    dev = clean_x.device
    words = []
    for xs, ys, ind in ((clean_x, clean_y, None), (bd_x, bd_y, bd_indicator)):
        metrics = torch.zeros(L.METRICS_WORDS, dtype=torch.int64, device=dev)
        bounds = batch_bounds(int(xs.shape[0]), int(batch_size))
        for s, e in bounds:
            torch.ops.abd.smallcnn_eval_metrics(xs[s:e], params, running, K, prec, ys[s:e],
                                                ind[s:e] if ind is not None else None, metrics)
        words.append((metrics, len(bounds)))
    (cl, ct, cc, _, _, _), nc = T.read_metrics(words[0][0]), words[0][1]
    (bl, _, _, pt, ah, _), nb = T.read_metrics(words[1][0]), words[1][1]
    return 100 * cc / ct, 100 * ah / pt, cl / nc, bl / nb


class FinePruneResult(NamedTuple):
    pruning_rows: list        # pruning_data.csv: [num_pruned, pruning_ratio, test_acc, test_asr] per step run
    ft_row: tuple             # ft_data.csv: (test_clean_acc, test_asr, clean_test_loss, bd_test_loss)
    unit_mask: torch.Tensor   # (128,) uint8 host tensor, nonzero = pruned: the mask of stop_index
    model: torch.nn.Module    # the fine-tuned smallcnn; fc2.weight is the effective (masked) weight
    weight_orig: torch.Tensor  # fc2.weight as prune's weight_orig holds it: pruned columns keep their old values
    last_index: int
    stop_index: int
    activation: torch.Tensor
    seq_sort: np.ndarray
    ft_loss: float
    ft_acc: float


def fine_prune(model, val_x, val_y, clean_x, clean_y, bd_x, bd_y, bd_indicator, *, once_prune_ratio=0.01,
               acc_ratio=0.1, lr_ft=0.01, batch_size=256, val_order=None, ft_order=None, ft_masks=None):
    """fp.py's mitigation() after its data loading, on device-resident sets: the activation of the first
    validation batch (hidden_activation), the ranking, the prune sweep over the clean and the backdoor test
    set (all steps at once, one eval forward per batch), the stop rule on the host (prune_stop), one
    torch.optim.Adam(lr_ft) fine-tuning epoch over the validation set with the mask of the step at which the
    loop ENDED (stop_index, see prune_stop), and training.test's four numbers of the result.  val_order /
    ft_order: the row permutations of the two shuffled passes over the validation loader; ft_masks: see
    pruned_finetune_epoch.  The given model is read, never modified; the result carries one fine-tuned copy."""
    import copy
    from . import ops  # noqa: F401  (registers torch.ops.abd)
    for t, what in ((val_x, "validation input"), (val_y, "validation labels"), (clean_x, "clean input"),
                    (clean_y, "clean labels"), (bd_x, "backdoor input"), (bd_y, "backdoor labels"),
                    (bd_indicator, "backdoor indicator")):
        L.require_device(t, f"fine_prune {what}")
    activation = hidden_activation(model, val_x, batch_size, val_order, first_batch_only=True)
    seq_sort = rank_units(activation)
    nums, masks = prune_masks(seq_sort, once_prune_ratio)
    clean_y, bd_y, bd_indicator = clean_y.to(torch.int64), bd_y.to(torch.int64), bd_indicator.to(torch.int64)
    _, acc = fc_prune_sweep(model, clean_x, clean_y, masks, batch_size)
    _, asr = fc_prune_sweep(model, bd_x, bd_y, masks, batch_size)
    acc, asr = acc.tolist(), asr.tolist()
    steps, last_index, stop_index = prune_stop(nums, acc, acc_ratio)
    rows = [[nums[i], nums[i] / len(seq_sort), acc[i], asr[i]] for i in range(steps)]
    unit_mask = masks[steps - 1].clone()
    tuned = copy.deepcopy(model)
    orig = tuned.fc2.weight.detach().clone()
    optimizer = torch.optim.Adam(tuned.parameters(), lr=lr_ft)
    ft_loss, ft_acc = pruned_finetune_epoch(tuned, val_x, val_y, optimizer, unit_mask, batch_size, ft_order, ft_masks)
    eng = tuned._engine
    ft_row = _test_numbers(eng.params, eng.running, eng.K, tuned.gemm_precision, clean_x, clean_y, bd_x, bd_y,
                           bd_indicator, batch_size)
    weight_orig = tuned.fc2.weight.detach().clone()
    keep = unit_mask.ne(0).to(weight_orig.device)
    weight_orig[:, keep] = orig.to(weight_orig.device)[:, keep]
    return FinePruneResult(rows, ft_row, unit_mask, tuned, weight_orig, last_index, stop_index, activation, seq_sort,
                           ft_loss, ft_acc)
