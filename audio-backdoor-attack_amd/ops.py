"""PyTorch custom ops over libabd: the ``abd`` operator namespace (north_star
"surfaced as PyTorch-ROCm custom ops").

    torch.ops.abd.mfcc                 prepare_dataset.py:35-47 (+ the fused trigger injection)
    torch.ops.abd.inject_waveform      ultrasonic.py:75, flowmur.py:77-85 / 101-106
    torch.ops.abd.smallcnn_eval        utils/models.py:43-65 in eval mode
    torch.ops.abd.smallcnn_eval_metrics  the same + test()'s counters (utils/training_tools.py:98-128)
    torch.ops.abd.smallcnn_ablate_eval the defenses' neuron-ablation scan (ft_reg.py:173-190), all variants
                                       of a batch in one launch sequence
    torch.ops.abd.smallcnn_train_step  utils/training_tools.py:60-79: forward, CE, backward, Adam,
                                       loss / accuracy / ASR counters -- one launch sequence
    torch.ops.abd.adam                 torch.optim.Adam single-tensor step (flat buffers)
    torch.ops.abd.sgd                  torch.optim.SGD with momentum (flat buffers; optional two-gradient blend)
    torch.ops.abd.segment_norms / perturb  per-tensor ``grad.norm()`` and ``param += r * grad / norm`` (ft_reg.py:99-101)
    torch.ops.abd.smallcnn_finetune_reg_step  ft_reg.py:83-123: one batch of train_finetuning_reg -- two gradient
                                       passes, the displaced parameters, SGD, the loss / accuracy forward
    torch.ops.abd.row_abs_sums / smallcnn_unlearn_step / reinit_weights  tsbd.py's unlearning, scores, re-init sweep
    torch.ops.abd.smallcnn_unlearn_run / nwc_pair  correlation_analysis.py: the unlearning loop on its one fixed
                                       batch, both models' weight-change sums and their Pearson correlation
    torch.ops.abd.smallcnn_hidden_sums / smallcnn_fcprune_eval / smallcnn_pruned_finetune_step  fp.py: the mean
                                       activation of fc2's input, the prune sweep, the masked Adam fine-tuning step

Each op enqueues its HIP kernels on the current torch stream through the C ABI
(include/abd.h) and has a fake (meta) implementation, so the ops trace under FakeTensor /
torch.compile-style tooling and pass ``torch.library.opcheck`` (tests/test_gpu_ops.py).  The
mutating ops declare what they write (params, grads, Adam moments, BN buffers, counters).
There is no CPU kernel: a CPU tensor raises AbdError (no silent fallback).

The drop-in shims route through these ops (features.MFCC, training.train / test, the
smallcnn eval forward); the HBM-resident bench loop (pipeline.ResidentTrainer) calls the same C
entry points directly to skip the Python dispatcher (~2 x 20 us per step).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor

from . import _lib as L
from . import features as F
from ._flat import net_handle

_NETS: dict = {}


def n_frames(length, n_fft: int, hop: int):
    """center=True frame count (torch.stft / librosa): 1 + (L + 2 (n_fft // 2) - n_fft) // hop."""
    return 1 + (length + 2 * (n_fft // 2) - n_fft) // hop


def _net(H0: int, W0: int, K: int, precision: str = "f32split"):
    """A cached libabd network handle for one geometry (no device state: shapes and precision)."""
    key = (int(H0), int(W0), int(K))
    h = _NETS.get(key)
    if h is None:
        h = C.c_void_p()
        L.check(L.lib().abd_smallcnn_create(key[0], key[1], key[2], 0, C.byref(h)), "abd_smallcnn_create")
        _NETS[key] = h
    L.check(L.lib().abd_smallcnn_set_precision(h, L.PRECISIONS[precision]), "abd_smallcnn_set_precision")
    return h


def _ws(n_bytes: int, device) -> Tensor:
    return torch.empty(max(int(n_bytes), 1), dtype=torch.uint8, device=device)


def _ptr(t: Optional[Tensor]):
    return t.data_ptr() if t is not None else None


# --------------------------------------------------------------------------- features
@torch.library.custom_op("abd::mfcc", mutates_args=())
def mfcc(waves: Tensor, sample_rate: int, n_mfcc: int, n_fft: int, hop_length: int, mel: str = "htk",
         pad: str = "reflect", rows: Optional[Tensor] = None, inject_mode: int = 0,
         trigger: Optional[Tensor] = None, poison: Optional[Tensor] = None, position: Optional[Tensor] = None,
         snr_db: float = 30.0, patch_box: Optional[list[int]] = None, patch_value: float = -200.0) -> Tensor:
    """(N, L) fp32 waves -> (B, 1, T, n_mfcc): torchaudio T.MFCC (mel 'htk', pad 'reflect') or librosa
    (mel 'slaney', pad 'constant'), with optional trigger injection fused into the load / epilogue."""
    L.require_device(waves, "waves")
    cfg = F.MfccConfig(int(sample_rate), int(n_mfcc), int(n_fft), int(hop_length), int(waves.shape[1]), mel=mel,
                       pad=pad)
    inj = None
    if inject_mode or patch_box is not None:
        inj = F.Injection(mode=int(inject_mode), trigger=trigger, poison=poison, position=position,
                          snr_db=float(snr_db),
                          patch=(tuple(patch_box) + (float(patch_value),)) if patch_box is not None else None)
    return F.mfcc_batch(waves, cfg, rows=rows, inject=inj)


@mfcc.register_fake
def _(waves, sample_rate, n_mfcc, n_fft, hop_length, mel="htk", pad="reflect", rows=None, inject_mode=0,
      trigger=None, poison=None, position=None, snr_db=30.0, patch_box=None, patch_value=-200.0):
    B = rows.shape[0] if rows is not None else waves.shape[0]
    return waves.new_empty((B, 1, n_frames(waves.shape[1], n_fft, hop_length), n_mfcc))


@torch.library.custom_op("abd::inject_waveform", mutates_args=())
def inject_waveform(waves: Tensor, trigger: Tensor, mode: int, poison: Optional[Tensor] = None,
                    position: Optional[Tensor] = None, snr_db: float = 30.0) -> Tensor:
    """The poisoned waveforms (N, L) themselves (the reference's bd_*_wav arrays)."""
    inj = F.Injection(mode=int(mode), trigger=trigger, poison=poison, position=position, snr_db=float(snr_db))
    return F.inject_waveform(waves, int(waves.shape[1]), inj)


@inject_waveform.register_fake
def _(waves, trigger, mode, poison=None, position=None, snr_db=30.0):
    return torch.empty_like(waves)


# --------------------------------------------------------------------------- smallcnn
def _eval(x, params, running, num_classes, precision, labels, indicators, metrics):
    L.require_device(x, "smallcnn input")
    B, H0, W0 = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    h = _net(H0, W0, num_classes, precision)
    out = torch.empty((B, int(num_classes)), dtype=torch.float32, device=x.device)
    ws = _ws(L.lib().abd_smallcnn_workspace_bytes(h, B), x.device)
    L.check(L.lib().abd_smallcnn_eval(h, x.data_ptr(), B, params.data_ptr(), running.data_ptr(), _ptr(labels),
                                      _ptr(indicators), out.data_ptr(), _ptr(metrics), ws.data_ptr(), ws.numel(),
                                      L.stream_ptr(x.device)), "abd_smallcnn_eval")
    return out


@torch.library.custom_op("abd::smallcnn_eval", mutates_args=())
def smallcnn_eval(x: Tensor, params: Tensor, running: Tensor, num_classes: int, precision: str = "f32split") -> Tensor:
    """model.eval() forward: (B, 1, H0, W0) -> log-probs (B, K); running BN statistics, no dropout."""
    return _eval(x, params, running, num_classes, precision, None, None, None)


@smallcnn_eval.register_fake
def _(x, params, running, num_classes, precision="f32split"):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::smallcnn_eval_metrics", mutates_args=("metrics",))
def smallcnn_eval_metrics(x: Tensor, params: Tensor, running: Tensor, num_classes: int, precision: str,
                          labels: Tensor, indicators: Optional[Tensor], metrics: Tensor) -> Tensor:
    """The eval forward plus test()'s loss / accuracy / ASR counters accumulated into metrics
    (int64[8]; utils/training_tools.py:98-128); returns the log-probs."""
    return _eval(x, params, running, num_classes, precision, labels, indicators, metrics)


@smallcnn_eval_metrics.register_fake
def _(x, params, running, num_classes, precision, labels, indicators, metrics):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::smallcnn_ablate_eval", mutates_args=("loss_sum", "correct"))
def smallcnn_ablate_eval(x: Tensor, params: Tensor, running: Tensor, labels: Tensor, masks: Tensor, kind: int,
                         variants_per_pass: int, loss_sum: Tensor, correct: Tensor, num_classes: int,
                         precision: str = "f32split") -> None:
    """The neuron-ablation sweep on one batch (abd_smallcnn_ablate_eval): variant v is the eval model with
    the conv filters (kind 0) or BN weights (kind 1) of masks[v] zeroed; loss_sum[v] (float64) += the batch's
    summed CE loss, correct[v] (int64) += its correct predictions.  masks is a (V, 160) uint8 HOST tensor
    (conv1 0..63, conv2 64..127, conv3 128..159); a device tensor is copied to the host first."""
    L.require_device(x, "smallcnn input")
    for t, what in ((params, "params"), (running, "running"), (labels, "labels"), (loss_sum, "loss_sum"),
                    (correct, "correct")):
        L.require_device(t, what)
    B, H0, W0 = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    m = masks.detach().to("cpu", torch.uint8).contiguous()
    V = int(m.shape[0])
    if m.dim() != 2 or m.shape[1] != L.ABLATE_CHANNELS:
        raise L.AbdError(f"masks must be (V, {L.ABLATE_CHANNELS}), got {tuple(m.shape)}")
    if loss_sum.numel() < V or correct.numel() < V or loss_sum.dtype != torch.float64 or correct.dtype != torch.int64:
        raise L.AbdError("loss_sum (float64) and correct (int64) need one entry per variant")
    if labels.dtype != torch.int64 or labels.numel() != B:
        raise L.AbdError("labels must be int64, one per batch row")
    if B == 0 or V == 0:
        return None
    h = _net(H0, W0, num_classes, precision)
    vpp = max(1, min(int(variants_per_pass), V))
    ws = _ws(L.lib().abd_smallcnn_ablate_workspace_bytes(h, B, vpp), x.device)
    L.check(L.lib().abd_smallcnn_ablate_eval(h, x.data_ptr(), B, params.data_ptr(), running.data_ptr(),
                                             labels.data_ptr(), m.data_ptr(), V, int(kind), vpp, loss_sum.data_ptr(),
                                             correct.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr(x.device)),
            "abd_smallcnn_ablate_eval")
    return None


@smallcnn_ablate_eval.register_fake
def _(x, params, running, labels, masks, kind, variants_per_pass, loss_sum, correct, num_classes,
      precision="f32split"):
    return None


@torch.library.custom_op("abd::smallcnn_train_step",
                         mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "running", "num_batches_tracked",
                                       "metrics"))
def smallcnn_train_step(x: Tensor, labels: Tensor, indicators: Optional[Tensor], params: Tensor, grads: Tensor,
                        exp_avg: Tensor, exp_avg_sq: Tensor, running: Tensor, num_batches_tracked: Tensor,
                        metrics: Tensor, num_classes: int, adam_step: int, lr: float, beta1: float, beta2: float,
                        eps: float, seed: int, counter: int, mask1: Optional[Tensor] = None,
                        mask2: Optional[Tensor] = None, precision: str = "f32split", grad_scale: float = 1.0,
                        row_offset: int = 0) -> Tensor:
    """One fused train() iteration on the device; returns the batch's log-probs (B, K).

    adam_step >= 1 applies torch.optim.Adam (that step index); 0 leaves params untouched (data
    parallelism: grads are all-reduced first, then abd::adam).  metrics (int64[8]) accumulates
    loss / samples / correct / poisoned / ASR hits / batches like train()."""
    L.require_device(x, "smallcnn input")
    B, H0, W0 = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    h = _net(H0, W0, num_classes, precision)
    out = torch.empty((B, int(num_classes)), dtype=torch.float32, device=x.device)
    a = L.TrainArgs()
    a.x, a.batch = x.data_ptr(), B
    a.labels, a.indicators = labels.data_ptr(), _ptr(indicators)
    a.params, a.grads, a.running = params.data_ptr(), grads.data_ptr(), running.data_ptr()
    a.exp_avg, a.exp_avg_sq = exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    a.num_batches_tracked = num_batches_tracked.data_ptr()
    a.lr, a.beta1, a.beta2, a.eps = float(lr), float(beta1), float(beta2), float(eps)
    a.adam_step, a.do_update = int(adam_step), 1 if adam_step > 0 else 0
    a.seed, a.counter, a.row_offset = int(seed), int(counter), int(row_offset)
    a.mask1_in, a.mask2_in = _ptr(mask1), _ptr(mask2)
    a.logprobs_out, a.metrics, a.grad_scale = out.data_ptr(), metrics.data_ptr(), float(grad_scale)
    ws = _ws(L.lib().abd_smallcnn_workspace_bytes(h, B), x.device)
    L.check(L.lib().abd_smallcnn_train_step(h, C.byref(a), ws.data_ptr(), ws.numel(), L.stream_ptr(x.device)),
            "abd_smallcnn_train_step")
    return out


@smallcnn_train_step.register_fake
def _(x, labels, indicators, params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics, num_classes,
      adam_step, lr, beta1, beta2, eps, seed, counter, mask1=None, mask2=None, precision="f32split", grad_scale=1.0,
      row_offset=0):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::adam", mutates_args=("params", "exp_avg", "exp_avg_sq"))
def adam(params: Tensor, grads: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step: int, lr: float, beta1: float,
         beta2: float, eps: float) -> None:
    """torch.optim.Adam single-tensor update over flat fp32 buffers (weight_decay 0)."""
    L.require_device(params, "params")
    L.check(L.lib().abd_adam_f32(params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                 params.numel(), int(step), float(lr), float(beta1), float(beta2), float(eps),
                                 L.stream_ptr(params.device)), "abd_adam_f32")


@adam.register_fake
def _(params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps):
    return None


# --------------------------------------------------------------------------- the defences' step ops
_MASK_FIELDS = ("mask1_in", "mask2_in", "mask1_out", "mask2_out")


def _check_masks(masks, B, flat, lead=()):
    """masks = (mask1_in, mask2_in, mask1_out, mask2_out), each None or a uint8 device tensor (*lead, B, flat) /
    (*lead, B, 128); the in and the out masks come in pairs."""
    if (masks[0] is None) != (masks[1] is None) or (masks[2] is None) != (masks[3] is None):
        raise L.AbdError("dropout masks come in pairs")
    for m, cols, what in zip(masks, (flat, 128, flat, 128), _MASK_FIELDS):
        if m is None:
            continue
        L.require_device(m, what)
        shape = (*lead, B, cols)
        if m.dtype != torch.uint8 or tuple(m.shape) != shape:
            raise L.AbdError(f"{what} must be uint8 {shape}, got {tuple(m.shape)}")


def _defence_step(name, a, x, labels, state, num_classes, precision, seed, counter, row_offset, masks, adam=None,
                  lead=(), out_lead=(), workspace=None, extra=()):
    """What the step ops of ft_reg, TSBD, the correlation analysis and fine-pruning share; returns the log-probs
    (*out_lead, B, K).  a: abd_smallcnn_<name>'s argument struct with the op's own fields set; state: {field:
    flat device buffer}, written into the fields of those names; adam: (adam_step, lr, beta1, beta2, eps) for the
    structs that carry them; masks: see _check_masks -- a struct with one mask pointer per pass (FinetuneRegArgs)
    gets the lead slices, any other the tensor's start; workspace: the <w> of abd_smallcnn_<w>_workspace_bytes;
    extra: the arguments between the struct and the workspace."""
    L.require_device(x, "smallcnn input")
    L.require_device(labels, "labels")
    for what, t in state.items():
        L.require_device(t, what)
    B, H0, W0 = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    h = _net(H0, W0, num_classes, precision)
    flat = L.lib().abd_smallcnn_flat_features(h)
    if labels.dtype != torch.int64 or labels.numel() != B:
        raise L.AbdError("labels must be int64, one per batch row")
    _check_masks(masks, B, flat, lead)
    for m, cols, what in zip(masks, (flat, 128, flat, 128), _MASK_FIELDS):
        field = getattr(a, what)
        if not isinstance(field, C.Array):
            setattr(a, what, _ptr(m))
        elif m is not None:
            for k in range(len(field)):
                field[k] = m.data_ptr() + k * B * cols
    out = torch.empty((*out_lead, B, int(num_classes)), dtype=torch.float32, device=x.device)
    a.x, a.labels, a.batch = x.data_ptr(), labels.data_ptr(), B
    for what, t in state.items():
        setattr(a, what, t.data_ptr())
    if adam is not None:
        a.adam_step, a.lr, a.beta1, a.beta2, a.eps = int(adam[0]), *(float(v) for v in adam[1:])
    a.seed, a.counter, a.row_offset = int(seed), int(counter), int(row_offset)
    a.logprobs_out = out.data_ptr()
    ws = _ws(getattr(L.lib(), f"abd_smallcnn_{workspace}_workspace_bytes")(h, B), x.device)
    L.check(getattr(L.lib(), f"abd_smallcnn_{name}")(h, C.byref(a), *extra, ws.data_ptr(), ws.numel(),
                                                     L.stream_ptr(x.device)), f"abd_smallcnn_{name}")
    return out


def _adam_state(params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics):
    return dict(params=params, grads=grads, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, running=running,
                num_batches_tracked=num_batches_tracked, metrics=metrics)


# --------------------------------------------------------------------------- fine-tuning (ft_reg.py)
def _offsets(offsets):
    """Segment offsets as the C ABI's host int64 array (validated by the library)."""
    offs = [int(o) for o in offsets]
    if len(offs) < 2:
        raise L.AbdError("segment offsets need at least two entries")
    return (C.c_int64 * len(offs))(*offs), len(offs) - 1


@torch.library.custom_op("abd::segment_norms", mutates_args=())
def segment_norms(buf: Tensor, offsets: list[int]) -> Tensor:
    """L2 norm of each segment [offsets[s], offsets[s + 1]) of a flat fp32 buffer: double accumulation in a
    fixed order, rounded to fp32 once (``grad.norm()`` per parameter tensor, ft_reg.py:101)."""
    L.require_device(buf, "segment_norms buffer")
    if buf.dtype != torch.float32:
        raise L.AbdError("segment_norms expects float32")
    arr, n_seg = _offsets(offsets)
    if offsets[-1] > buf.numel():
        raise L.AbdError("segment offsets reach past the buffer")
    out = torch.empty(n_seg, dtype=torch.float32, device=buf.device)
    ws = _ws(max(L.lib().abd_segment_norms_workspace_bytes(arr, n_seg), 8), buf.device)
    L.check(L.lib().abd_segment_norms_f32(buf.data_ptr(), arr, n_seg, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          L.stream_ptr(buf.device)), "abd_segment_norms_f32")
    return out


@segment_norms.register_fake
def _(buf, offsets):
    return buf.new_empty((len(offsets) - 1,))


@torch.library.custom_op("abd::perturb", mutates_args=())
def perturb(params: Tensor, grads: Tensor, norms: Tensor, offsets: list[int], r: float) -> Tensor:
    """out = params + r * (grads / norms[segment]) in fp32, a new flat tensor (ft_reg.py:99-101 on a copy);
    elements outside [offsets[0], offsets[-1]) are copied.  A zero norm gives NaN in its segment."""
    for t, what in ((params, "params"), (grads, "grads"), (norms, "norms")):
        L.require_device(t, what)
    arr, n_seg = _offsets(offsets)
    if offsets[-1] > params.numel() or grads.numel() != params.numel() or norms.numel() < n_seg:
        raise L.AbdError("perturb: segment offsets / buffer sizes do not agree")
    out = params.clone()
    L.check(L.lib().abd_perturb_f32(params.data_ptr(), grads.data_ptr(), norms.data_ptr(), arr, n_seg, float(r),
                                    out.data_ptr(), L.stream_ptr(params.device)), "abd_perturb_f32")
    return out


@perturb.register_fake
def _(params, grads, norms, offsets, r):
    return torch.empty_like(params)


@torch.library.custom_op("abd::sgd", mutates_args=("params", "momentum_buf", "grad_out"))
def sgd(params: Tensor, grads: Tensor, momentum_buf: Optional[Tensor], grad_out: Optional[Tensor], lr: float,
        momentum: float = 0.0, grads2: Optional[Tensor] = None, alpha: float = 0.0) -> None:
    """torch.optim.SGD single-tensor update over flat fp32 buffers (dampening 0, no Nesterov, weight_decay 0):
    d = grads, or (1 - alpha) grads + alpha grads2; momentum_buf = momentum * momentum_buf + d;
    params -= lr * momentum_buf.  momentum_buf None is plain SGD (momentum must be 0).  grad_out (or None)
    receives d.  (The mutated arguments carry no defaults: torch's in-place bookkeeping indexes them by position.)"""
    L.require_device(params, "params")
    n = params.numel()
    for t, what in ((grads, "grads"), (momentum_buf, "momentum_buf"), (grads2, "grads2"), (grad_out, "grad_out")):
        if t is not None:
            L.require_device(t, what)
            if t.numel() != n or t.dtype != torch.float32:
                raise L.AbdError(f"sgd: {what} must be float32 with params' element count")
    L.check(L.lib().abd_sgd_f32(params.data_ptr(), grads.data_ptr(), _ptr(grads2), float(alpha), _ptr(momentum_buf),
                                float(momentum), float(lr), _ptr(grad_out), n, L.stream_ptr(params.device)),
            "abd_sgd_f32")
    return None


@sgd.register_fake
def _(params, grads, momentum_buf, grad_out, lr, momentum=0.0, grads2=None, alpha=0.0):
    return None


@torch.library.custom_op("abd::smallcnn_finetune_reg_step",
                         mutates_args=("params", "grads", "momentum_buf", "running", "num_batches_tracked", "loss_sum",
                                       "correct", "mask1_out", "mask2_out"))
def smallcnn_finetune_reg_step(x: Tensor, labels: Tensor, params: Tensor, grads: Tensor,
                               momentum_buf: Optional[Tensor], running: Tensor, num_batches_tracked: Tensor,
                               loss_sum: Tensor, correct: Tensor, num_classes: int, r: float, alpha: float, lr: float,
                               momentum: float, seed: int, counter: int, mask1_out: Optional[Tensor],
                               mask2_out: Optional[Tensor], mask1_in: Optional[Tensor] = None,
                               mask2_in: Optional[Tensor] = None, precision: str = "f32split",
                               row_offset: int = 0) -> Tensor:
    """One batch of train_finetuning_reg (ft_reg.py:83-123) on the device; returns the log-probs of its three
    forwards (3, B, K).  params, momentum_buf, running and num_batches_tracked are updated in place, grads is
    left holding (1 - alpha) g1 + alpha g2, loss_sum (float64[1]) += the post-update batch-mean loss, correct
    (int64[1]) += its hits.  mask*_in / mask*_out are (3, B, flat) and (3, B, 128) uint8, one slice per forward;
    without mask*_in the masks come from (seed, counter), (seed, counter + 1), (seed, counter + 2)."""
    for t, what in ((loss_sum, "loss_sum"), (correct, "correct")):
        L.require_device(t, what)
    if loss_sum.dtype != torch.float64 or correct.dtype != torch.int64 or not loss_sum.numel() or not correct.numel():
        raise L.AbdError("loss_sum (float64) and correct (int64) need one entry each")
    a = L.FinetuneRegArgs()
    a.r, a.alpha, a.lr, a.momentum = float(r), float(alpha), float(lr), float(momentum)
    a.momentum_buf = _ptr(momentum_buf)
    a.loss_sum, a.correct = loss_sum.data_ptr(), correct.data_ptr()
    state = dict(params=params, grads=grads, running=running, num_batches_tracked=num_batches_tracked)
    return _defence_step("finetune_reg_step", a, x, labels, state, num_classes, precision, seed, counter, row_offset,
                         (mask1_in, mask2_in, mask1_out, mask2_out), lead=(3,), out_lead=(3,),
                         workspace="finetune_reg")


@smallcnn_finetune_reg_step.register_fake
def _(x, labels, params, grads, momentum_buf, running, num_batches_tracked, loss_sum, correct, num_classes, r, alpha,
      lr, momentum, seed, counter, mask1_out, mask2_out, mask1_in=None, mask2_in=None, precision="f32split",
      row_offset=0):
    return x.new_empty((3, x.shape[0], num_classes))


# --------------------------------------------------------------------------- TSBD (tsbd.py)
def _row_table(table):
    """A flat list of (offset, rows, row_len) triples as the C ABI's host array (validated by the library)."""
    vals = [int(v) for v in table]
    if not vals or len(vals) % 3:
        raise L.AbdError("a row table is a flat list of (offset, rows, row_len) triples")
    n_seg = len(vals) // 3
    arr = (L.RowSegment * n_seg)(*[L.RowSegment(*vals[3 * s:3 * s + 3]) for s in range(n_seg)])
    return arr, n_seg, vals


def _table_extent(vals):
    """(total rows, packed values, one past the last element) of a row table."""
    rows = sum(vals[1::3])
    packed = sum(r * n for r, n in zip(vals[1::3], vals[2::3]))
    end = max(o + r * n for o, r, n in zip(vals[0::3], vals[1::3], vals[2::3]))
    return rows, packed, end


def _checked_row_table(table, numel=None):
    """_row_table plus what its callers ask of it: no negative entry and, with numel given, an end inside a buffer
    of that many elements.  Returns (C array, n_seg, total rows, packed values, one past the last element)."""
    arr, n_seg, vals = _row_table(table)
    if min(vals) < 0:
        raise L.AbdError("row table entries must not be negative")
    rows, packed, end = _table_extent(vals)
    if numel is not None and end > numel:
        raise L.AbdError("row table reaches past the buffer")
    return arr, n_seg, rows, packed, end


@torch.library.custom_op("abd::row_abs_sums", mutates_args=())
def row_abs_sums(a: Tensor, b: Optional[Tensor], table: list[int], want_absdiff: bool = True) -> tuple[Tensor, Tensor]:
    """(absdiff, row_sums) of a row table (flat (offset, rows, row_len) triples) over flat fp32 buffers:
    absdiff = (a - b).abs() (a.abs() without b) with the table's rows packed one after another, bit-equal to
    torch's; row_sums[r] its per-row sum, double accumulation rounded to fp32 once (tsbd.py:350-352, :127).
    want_absdiff False returns an empty absdiff."""
    L.require_device(a, "row_abs_sums a")
    if a.dtype != torch.float32:
        raise L.AbdError("row_abs_sums expects float32")
    if b is not None:
        L.require_device(b, "row_abs_sums b")
        if b.dtype != torch.float32 or b.numel() != a.numel():
            raise L.AbdError("row_abs_sums: b must be float32 with a's element count")
    arr, n_seg, rows, packed, _ = _checked_row_table(table, a.numel())
    absdiff = torch.empty(packed if want_absdiff else 0, dtype=torch.float32, device=a.device)
    sums = torch.empty(rows, dtype=torch.float32, device=a.device)
    L.check(L.lib().abd_row_abs_sums_f32(a.data_ptr(), _ptr(b), arr, n_seg, absdiff.data_ptr() if want_absdiff else None,
                                         sums.data_ptr(), L.stream_ptr(a.device)), "abd_row_abs_sums_f32")
    return absdiff, sums


@row_abs_sums.register_fake
def _(a, b, table, want_absdiff=True):
    rows, packed, _ = _table_extent([int(v) for v in table])
    return a.new_empty((packed if want_absdiff else 0,)), a.new_empty((rows,))


@torch.library.custom_op("abd::smallcnn_unlearn_step",
                         mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "running", "num_batches_tracked",
                                       "metrics", "record_abs_sums", "mask1_out", "mask2_out"))
def smallcnn_unlearn_step(x: Tensor, labels: Tensor, params: Tensor, grads: Tensor, exp_avg: Tensor,
                          exp_avg_sq: Tensor, running: Tensor, num_batches_tracked: Tensor, metrics: Tensor,
                          record_abs_sums: Optional[Tensor], mask1_out: Optional[Tensor], mask2_out: Optional[Tensor],
                          num_classes: int, adam_step: int, lr: float, beta1: float, beta2: float, eps: float,
                          seed: int, counter: int, record: Optional[list[int]] = None,
                          mask1_in: Optional[Tensor] = None, mask2_in: Optional[Tensor] = None,
                          precision: str = "f32split", row_offset: int = 0) -> Tensor:
    """One batch of train_unlearning (tsbd.py:108-138) on the device; returns the batch's log-probs (B, K).
    A no-update train step (metrics += the positive loss and the hits, BN buffers advance once), then grads
    <- -grads and torch.optim.Adam (step index adam_step >= 1) on it.  record = [offset, rows, row_len] of the
    record layer inside the flat buffers: record_abs_sums (float32[rows]) receives its per-row |grad| sums."""
    a = L.UnlearnArgs()
    if record is not None:
        if len(record) != 3 or record_abs_sums is None:
            raise L.AbdError("record is [offset, rows, row_len] and needs record_abs_sums")
        L.require_device(record_abs_sums, "record_abs_sums")
        if record_abs_sums.dtype != torch.float32 or record_abs_sums.numel() < int(record[1]):
            raise L.AbdError("record_abs_sums must be float32 with one entry per record row")
        a.record_offset, a.record_rows, a.record_row_len = (int(v) for v in record)
        a.record_abs_sums = record_abs_sums.data_ptr()
    return _defence_step("unlearn_step", a, x, labels,
                         _adam_state(params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics),
                         num_classes, precision, seed, counter, row_offset, (mask1_in, mask2_in, mask1_out, mask2_out),
                         adam=(adam_step, lr, beta1, beta2, eps), workspace="unlearn")


@smallcnn_unlearn_step.register_fake
def _(x, labels, params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics, record_abs_sums, mask1_out,
      mask2_out, num_classes, adam_step, lr, beta1, beta2, eps, seed, counter, record=None, mask1_in=None,
      mask2_in=None, precision="f32split", row_offset=0):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::reinit_weights", mutates_args=())
def reinit_weights(params: Tensor, absdiff: Tensor, table: list[int], row_select: Tensor,
                   k: list[int]) -> tuple[Tensor, Tensor, Tensor]:
    """zero_reinit_weight (tsbd.py:49-63) for V variants at once: (out (V, n_params), thr (V), zeroed (V) int64).
    absdiff: the packed rows of abd::row_abs_sums; row_select: (V, total rows) uint8 HOST tensor (a device tensor
    is copied to the host first), nonzero = the neuron is among the variant's top_num; k[v] = int(m * wratio).
    out[v] = params with every weight of the selected rows whose absdiff >= the k[v]-th largest set to 0."""
    L.require_device(params, "params")
    L.require_device(absdiff, "absdiff")
    if params.dtype != torch.float32 or absdiff.dtype != torch.float32:
        raise L.AbdError("reinit_weights expects float32")
    arr, n_seg, rows, packed, end = _checked_row_table(table)
    sel = row_select.detach().to("cpu", torch.uint8).contiguous()
    V = len(k)
    if sel.dim() != 2 or tuple(sel.shape) != (V, rows):
        raise L.AbdError(f"row_select must be ({V}, {rows}), got {tuple(sel.shape)}")
    if absdiff.numel() < packed or end > params.numel():
        raise L.AbdError("reinit_weights: row table / buffer sizes do not agree")
    n = params.numel()
    out = torch.empty((V, n), dtype=torch.float32, device=params.device)
    thr = torch.empty(V, dtype=torch.float32, device=params.device)
    zeroed = torch.empty(V, dtype=torch.int64, device=params.device)
    ks = (C.c_int64 * max(V, 1))(*[int(v) for v in k])
    L.check(L.lib().abd_reinit_weights_f32(params.data_ptr(), n, absdiff.data_ptr(), arr, n_seg, sel.data_ptr(), ks, V,
                                           out.data_ptr(), thr.data_ptr(), zeroed.data_ptr(),
                                           L.stream_ptr(params.device)), "abd_reinit_weights_f32")
    return out, thr, zeroed


@reinit_weights.register_fake
def _(params, absdiff, table, row_select, k):
    V = len(k)
    return (params.new_empty((V, params.numel())), params.new_empty((V,)),
            params.new_empty((V,), dtype=torch.int64))


# --------------------------------------------------------------------------- correlation_analysis.py
@torch.library.custom_op("abd::smallcnn_unlearn_run",
                         mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "running", "num_batches_tracked",
                                       "metrics", "mask1_out", "mask2_out"))
def smallcnn_unlearn_run(x: Tensor, labels: Tensor, params: Tensor, grads: Tensor, exp_avg: Tensor,
                         exp_avg_sq: Tensor, running: Tensor, num_batches_tracked: Tensor, metrics: Tensor,
                         mask1_out: Optional[Tensor], mask2_out: Optional[Tensor], num_classes: int, n_steps: int,
                         adam_step: int, lr: float, beta1: float, beta2: float, eps: float, seed: int, counter: int,
                         mask1_in: Optional[Tensor] = None, mask2_in: Optional[Tensor] = None,
                         precision: str = "f32split", row_offset: int = 0) -> Tensor:
    """n_steps calls of correlation_analysis.py's train_unlearning (:41-71) on one fixed batch in one library call;
    returns the last step's log-probs (B, K).  Step i is abd::smallcnn_unlearn_step with adam_step + i and
    counter + i and no record layer, bit for bit.  metrics is int64 (n_steps, 8), zeroed by the caller: row i
    holds step i's loss and hits.  The masks, when given, are (n_steps, B, flat) and (n_steps, B, 128) uint8."""
    n_steps = int(n_steps)
    if n_steps < 1:
        raise L.AbdError(f"smallcnn_unlearn_run needs n_steps >= 1, got {n_steps}")
    if metrics.dtype != torch.int64 or tuple(metrics.shape) != (n_steps, L.METRICS_WORDS):
        raise L.AbdError(f"metrics must be int64 ({n_steps}, {L.METRICS_WORDS}), got {tuple(metrics.shape)}")
    return _defence_step("unlearn_run", L.UnlearnArgs(), x, labels,
                         _adam_state(params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics),
                         num_classes, precision, seed, counter, row_offset, (mask1_in, mask2_in, mask1_out, mask2_out),
                         adam=(adam_step, lr, beta1, beta2, eps), lead=(n_steps,), workspace="unlearn",
                         extra=(n_steps,))


@smallcnn_unlearn_run.register_fake
def _(x, labels, params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics, mask1_out, mask2_out,
      num_classes, n_steps, adam_step, lr, beta1, beta2, eps, seed, counter, mask1_in=None, mask2_in=None,
      precision="f32split", row_offset=0):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::nwc_pair", mutates_args=())
def nwc_pair(orig: Tensor, params_a: Tensor, params_b: Tensor, table: list[int],
             want_absdiff: bool = True) -> tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """correlation_analysis.py:146-157 for two unlearned flat parameter buffers against the original:
    (absdiff_a, absdiff_b, sums32_a, sums32_b, sums64 (2, rows) float64, stats (9) float64).  absdiff_* and
    sums32_* are bit-equal to abd::row_abs_sums(params_*, orig, table); sums64 holds the same row sums before
    their rounding to fp32; stats = [n, mean_x, mean_y, sxx, syy, sxy, r, slope, intercept] of x = sums64[0],
    y = sums64[1].  At most 1024 rows.  want_absdiff False returns empty absdiff tensors."""
    for t, what in ((orig, "nwc_pair orig"), (params_a, "nwc_pair params_a"), (params_b, "nwc_pair params_b")):
        L.require_device(t, what)
        if t.dtype != torch.float32 or t.numel() != orig.numel():
            raise L.AbdError("nwc_pair expects three float32 buffers of one size")
    arr, n_seg, rows, packed, _ = _checked_row_table(table, orig.numel())
    dev = orig.device
    absdiff = [torch.empty(packed if want_absdiff else 0, dtype=torch.float32, device=dev) for _ in range(2)]
    sums32 = [torch.empty(rows, dtype=torch.float32, device=dev) for _ in range(2)]
    sums64 = torch.empty((2, rows), dtype=torch.float64, device=dev)
    stats = torch.empty(L.NWC_STATS_WORDS, dtype=torch.float64, device=dev)
    L.check(L.lib().abd_nwc_pair_f32(orig.data_ptr(), params_a.data_ptr(), params_b.data_ptr(), arr, n_seg,
                                     absdiff[0].data_ptr() if want_absdiff else None,
                                     absdiff[1].data_ptr() if want_absdiff else None, sums32[0].data_ptr(),
                                     sums32[1].data_ptr(), sums64.data_ptr(), stats.data_ptr(), L.stream_ptr(dev)),
            "abd_nwc_pair_f32")
    return absdiff[0], absdiff[1], sums32[0], sums32[1], sums64, stats


@nwc_pair.register_fake
def _(orig, params_a, params_b, table, want_absdiff=True):
    rows, packed, _ = _table_extent([int(v) for v in table])
    n = packed if want_absdiff else 0
    return (orig.new_empty((n,)), orig.new_empty((n,)), orig.new_empty((rows,)), orig.new_empty((rows,)),
            orig.new_empty((2, rows), dtype=torch.float64), orig.new_empty((L.NWC_STATS_WORDS,), dtype=torch.float64))


# --------------------------------------------------------------------------- Fine-Pruning (fp.py)
@torch.library.custom_op("abd::smallcnn_hidden_sums", mutates_args=("sums",))
def smallcnn_hidden_sums(x: Tensor, params: Tensor, running: Tensor, sums: Tensor, num_classes: int,
                         precision: str = "f32split") -> None:
    """One eval forward of the batch, then sums[u] (float64[128]) += the column sum of fc2's input,
    relu(fc1(...)), over the batch rows (fp.py:140-146): double accumulation in a fixed order."""
    L.require_device(x, "smallcnn input")
    for t, what in ((params, "params"), (running, "running"), (sums, "sums")):
        L.require_device(t, what)
    if sums.dtype != torch.float64 or sums.numel() != L.FCPRUNE_UNITS:
        raise L.AbdError(f"sums must be float64[{L.FCPRUNE_UNITS}]")
    B, H0, W0 = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    if B == 0:
        return None
    h = _net(H0, W0, num_classes, precision)
    ws = _ws(L.lib().abd_smallcnn_workspace_bytes(h, B), x.device)
    L.check(L.lib().abd_smallcnn_hidden_sums(h, x.data_ptr(), B, params.data_ptr(), running.data_ptr(), sums.data_ptr(),
                                             ws.data_ptr(), ws.numel(), L.stream_ptr(x.device)),
            "abd_smallcnn_hidden_sums")
    return None


@smallcnn_hidden_sums.register_fake
def _(x, params, running, sums, num_classes, precision="f32split"):
    return None


@torch.library.custom_op("abd::smallcnn_fcprune_eval", mutates_args=("loss_sum", "correct"))
def smallcnn_fcprune_eval(x: Tensor, params: Tensor, running: Tensor, labels: Tensor, masks: Tensor, loss_sum: Tensor,
                          correct: Tensor, num_classes: int, precision: str = "f32split") -> None:
    """The prune sweep on one batch (abd_smallcnn_fcprune_eval): variant v is the eval model with the columns
    masks[v] of fc2.weight removed; loss_sum[v] (float64) += the batch's summed CE loss, correct[v] (int64) += its
    correct predictions.  masks is a (V, 128) uint8 HOST tensor, nonzero = pruned; a device tensor is copied to
    the host first."""
    L.require_device(x, "smallcnn input")
    for t, what in ((params, "params"), (running, "running"), (labels, "labels"), (loss_sum, "loss_sum"),
                    (correct, "correct")):
        L.require_device(t, what)
    B, H0, W0 = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    m = masks.detach().to("cpu", torch.uint8).contiguous()
    if m.dim() != 2 or m.shape[1] != L.FCPRUNE_UNITS:
        raise L.AbdError(f"masks must be (V, {L.FCPRUNE_UNITS}), got {tuple(m.shape)}")
    V = int(m.shape[0])
    if loss_sum.numel() < V or correct.numel() < V or loss_sum.dtype != torch.float64 or correct.dtype != torch.int64:
        raise L.AbdError("loss_sum (float64) and correct (int64) need one entry per variant")
    if labels.dtype != torch.int64 or labels.numel() != B:
        raise L.AbdError("labels must be int64, one per batch row")
    if B == 0 or V == 0:
        return None
    h = _net(H0, W0, num_classes, precision)
    ws = _ws(L.lib().abd_smallcnn_fcprune_workspace_bytes(h, B, V), x.device)
    L.check(L.lib().abd_smallcnn_fcprune_eval(h, x.data_ptr(), B, params.data_ptr(), running.data_ptr(),
                                              labels.data_ptr(), m.data_ptr(), V, loss_sum.data_ptr(),
                                              correct.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr(x.device)),
            "abd_smallcnn_fcprune_eval")
    return None


@smallcnn_fcprune_eval.register_fake
def _(x, params, running, labels, masks, loss_sum, correct, num_classes, precision="f32split"):
    return None


@torch.library.custom_op("abd::smallcnn_pruned_finetune_step",
                         mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "running", "num_batches_tracked",
                                       "metrics", "mask1_out", "mask2_out"))
def smallcnn_pruned_finetune_step(x: Tensor, labels: Tensor, params: Tensor, grads: Tensor, exp_avg: Tensor,
                                  exp_avg_sq: Tensor, running: Tensor, num_batches_tracked: Tensor, metrics: Tensor,
                                  pruned: Tensor, mask1_out: Optional[Tensor], mask2_out: Optional[Tensor],
                                  num_classes: int, adam_step: int, lr: float, beta1: float, beta2: float, eps: float,
                                  seed: int, counter: int, mask1_in: Optional[Tensor] = None,
                                  mask2_in: Optional[Tensor] = None, precision: str = "f32split",
                                  row_offset: int = 0) -> Tensor:
    """One batch of train_finetuning (fp.py:52-76) with prune.custom_from_mask active on fc2.weight; returns the
    batch's log-probs (B, K).  A no-update train step at params (which hold the effective weight: the caller
    zeroed the pruned columns once), the gradient of fc2.weight[:, j] zeroed for every unit j of pruned (a device
    uint8[128]) and written back, then torch.optim.Adam (step index adam_step >= 1) on it."""
    L.require_device(pruned, "pruned")
    if pruned.dtype != torch.uint8 or pruned.numel() != L.FCPRUNE_UNITS:
        raise L.AbdError(f"pruned must be uint8[{L.FCPRUNE_UNITS}]")
    a = L.PrunedFinetuneArgs()
    a.pruned = pruned.data_ptr()
    return _defence_step("pruned_finetune_step", a, x, labels,
                         _adam_state(params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics),
                         num_classes, precision, seed, counter, row_offset, (mask1_in, mask2_in, mask1_out, mask2_out),
                         adam=(adam_step, lr, beta1, beta2, eps), workspace="pruned_finetune")


@smallcnn_pruned_finetune_step.register_fake
def _(x, labels, params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics, pruned, mask1_out,
      mask2_out, num_classes, adam_step, lr, beta1, beta2, eps, seed, counter, mask1_in=None, mask2_in=None,
      precision="f32split", row_offset=0):
    return x.new_empty((x.shape[0], num_classes))


# --------------------------------------------------------------------------- lstmwithattention, RNN, largecnn, ResNet, smalllstm
_FLAT_NETS: dict = {}


def _flat_net(prefix: str, T: int, F: int, K: int):
    """A cached libabd handle (prefix abd_lstmattn / abd_rnn / abd_largecnn / abd_resnet / abd_smalllstm) for one geometry: shapes only,
    no device state."""
    key = (prefix, int(T), int(F), int(K))
    h = _FLAT_NETS.get(key)
    if h is None:
        h = _FLAT_NETS[key] = net_handle(*key)
    return h


def _flat_begin(prefix, what, x, num_classes):
    """What every entry point of either model starts from: (name -> lib function, handle, B, the logits to return,
    the (workspace, bytes, stream) arguments every call ends with)."""
    L.require_device(x, f"{what} input")
    B, T, F = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    h = _flat_net(prefix, T, F, num_classes)
    out = torch.empty((B, int(num_classes)), dtype=torch.float32, device=x.device)
    ws = _ws(getattr(L.lib(), f"{prefix}_workspace_bytes")(h, B), x.device)
    return (lambda name: getattr(L.lib(), f"{prefix}_{name}")), h, B, out, (ws.data_ptr(), ws.numel(),
                                                                         L.stream_ptr(x.device))


def _flat_eval(prefix, what, x, params, running, num_classes, labels, indicators, metrics):
    """The eval entry point of either model; running: (the BatchNorm statistics,), () for a model without any."""
    fn, h, B, out, tail = _flat_begin(prefix, what, x, num_classes)
    L.check(fn("eval")(h, x.data_ptr(), B, params.data_ptr(), *[r.data_ptr() for r in running], _ptr(labels),
                       _ptr(indicators), out.data_ptr(), _ptr(metrics), *tail), f"{prefix}_eval")
    return out


def _flat_train_step(prefix, what, a, x, labels, indicators, params, grads, exp_avg, exp_avg_sq, metrics, num_classes,
                     adam_step, lr, beta1, beta2, eps):
    """The fused step of either model: fills the fields both args structs share into a (the caller set the rest)."""
    fn, h, B, out, tail = _flat_begin(prefix, what, x, num_classes)
    a.x, a.batch = x.data_ptr(), B
    a.labels, a.indicators = labels.data_ptr(), _ptr(indicators)
    a.params, a.grads = params.data_ptr(), grads.data_ptr()
    a.exp_avg, a.exp_avg_sq = exp_avg.data_ptr(), exp_avg_sq.data_ptr()
    a.lr, a.beta1, a.beta2, a.eps = float(lr), float(beta1), float(beta2), float(eps)
    a.adam_step, a.do_update = int(adam_step), 1 if adam_step > 0 else 0
    a.logits_out, a.metrics, a.grad_scale = out.data_ptr(), metrics.data_ptr(), 1.0
    L.check(fn("train_step")(h, C.byref(a), *tail), f"{prefix}_train_step")
    return out


def _lstm_eval(x, params, running, num_classes, labels, indicators, metrics):
    return _flat_eval("abd_lstmattn", "lstmwithattention", x, params, (running,), num_classes, labels, indicators,
                      metrics)


@torch.library.custom_op("abd::lstmattn_eval", mutates_args=())
def lstmattn_eval(x: Tensor, params: Tensor, running: Tensor, num_classes: int) -> Tensor:
    """model.eval() forward of lstmwithattention: (B, 1, T, F) -> logits (B, K); running BN statistics,
    no dropout."""
    return _lstm_eval(x, params, running, num_classes, None, None, None)


@lstmattn_eval.register_fake
def _(x, params, running, num_classes):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::lstmattn_eval_metrics", mutates_args=("metrics",))
def lstmattn_eval_metrics(x: Tensor, params: Tensor, running: Tensor, num_classes: int, labels: Tensor,
                          indicators: Optional[Tensor], metrics: Tensor) -> Tensor:
    """The eval forward plus test()'s loss / accuracy / ASR counters accumulated into metrics
    (int64[8]); returns the logits."""
    return _lstm_eval(x, params, running, num_classes, labels, indicators, metrics)


@lstmattn_eval_metrics.register_fake
def _(x, params, running, num_classes, labels, indicators, metrics):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::lstmattn_train_step",
                         mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "running", "num_batches_tracked",
                                       "metrics"))
def lstmattn_train_step(x: Tensor, labels: Tensor, indicators: Optional[Tensor], params: Tensor, grads: Tensor,
                        exp_avg: Tensor, exp_avg_sq: Tensor, running: Tensor, num_batches_tracked: Tensor,
                        metrics: Tensor, num_classes: int, adam_step: int, lr: float, beta1: float, beta2: float,
                        eps: float, seed: int, counter: int, mask: Optional[Tensor] = None) -> Tensor:
    """One fused train() iteration of lstmwithattention on the device; returns the batch's logits (B, K).
    adam_step >= 1 applies torch.optim.Adam (that step index); 0 leaves params untouched."""
    a = L.LstmAttnArgs()
    a.running, a.num_batches_tracked = running.data_ptr(), num_batches_tracked.data_ptr()
    a.seed, a.counter = int(seed), int(counter)
    a.mask_in = _ptr(mask)
    return _flat_train_step("abd_lstmattn", "lstmwithattention", a, x, labels, indicators, params, grads, exp_avg,
                            exp_avg_sq, metrics, num_classes, adam_step, lr, beta1, beta2, eps)


@lstmattn_train_step.register_fake
def _(x, labels, indicators, params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics, num_classes,
      adam_step, lr, beta1, beta2, eps, seed, counter, mask=None):
    return x.new_empty((x.shape[0], num_classes))


def _rnn_eval(x, params, num_classes, labels, indicators, metrics):
    return _flat_eval("abd_rnn", "RNN", x, params, (), num_classes, labels, indicators, metrics)


@torch.library.custom_op("abd::rnn_eval", mutates_args=())
def rnn_eval(x: Tensor, params: Tensor, num_classes: int) -> Tensor:
    """Forward of RNN (3-layer 768-wide LSTM + fc on the last step): (B, 1, T, F) -> logits (B, K)."""
    return _rnn_eval(x, params, num_classes, None, None, None)


@rnn_eval.register_fake
def _(x, params, num_classes):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::rnn_eval_metrics", mutates_args=("metrics",))
def rnn_eval_metrics(x: Tensor, params: Tensor, num_classes: int, labels: Tensor, indicators: Optional[Tensor],
                     metrics: Tensor) -> Tensor:
    """The forward plus test()'s loss / accuracy / ASR counters accumulated into metrics (int64[8]);
    returns the logits."""
    return _rnn_eval(x, params, num_classes, labels, indicators, metrics)


@rnn_eval_metrics.register_fake
def _(x, params, num_classes, labels, indicators, metrics):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::rnn_train_step", mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "metrics"))
def rnn_train_step(x: Tensor, labels: Tensor, indicators: Optional[Tensor], params: Tensor, grads: Tensor,
                   exp_avg: Tensor, exp_avg_sq: Tensor, metrics: Tensor, num_classes: int, adam_step: int,
                   lr: float, beta1: float, beta2: float, eps: float) -> Tensor:
    """One fused train() iteration of RNN on the device; returns the batch's logits (B, K).
    adam_step >= 1 applies torch.optim.Adam (that step index); 0 leaves params untouched."""
    return _flat_train_step("abd_rnn", "RNN", L.RnnArgs(), x, labels, indicators, params, grads, exp_avg, exp_avg_sq,
                            metrics, num_classes, adam_step, lr, beta1, beta2, eps)


@rnn_train_step.register_fake
def _(x, labels, indicators, params, grads, exp_avg, exp_avg_sq, metrics, num_classes, adam_step, lr, beta1, beta2,
      eps):
    return x.new_empty((x.shape[0], num_classes))


def _largecnn_eval(x, params, num_classes, labels, indicators, metrics):
    return _flat_eval("abd_largecnn", "largecnn", x, params, (), num_classes, labels, indicators, metrics)


@torch.library.custom_op("abd::largecnn_eval", mutates_args=())
def largecnn_eval(x: Tensor, params: Tensor, num_classes: int) -> Tensor:
    """model.eval() forward of largecnn (no dropout): (B, 1, H, W) -> log-probabilities (B, K)."""
    return _largecnn_eval(x, params, num_classes, None, None, None)


@largecnn_eval.register_fake
def _(x, params, num_classes):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::largecnn_eval_metrics", mutates_args=("metrics",))
def largecnn_eval_metrics(x: Tensor, params: Tensor, num_classes: int, labels: Tensor, indicators: Optional[Tensor],
                          metrics: Tensor) -> Tensor:
    """The eval forward plus test()'s loss / accuracy / ASR counters accumulated into metrics (int64[8]);
    returns the log-probabilities."""
    return _largecnn_eval(x, params, num_classes, labels, indicators, metrics)


@largecnn_eval_metrics.register_fake
def _(x, params, num_classes, labels, indicators, metrics):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::largecnn_train_step",
                         mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "metrics"))
def largecnn_train_step(x: Tensor, labels: Tensor, indicators: Optional[Tensor], params: Tensor, grads: Tensor,
                        exp_avg: Tensor, exp_avg_sq: Tensor, metrics: Tensor, num_classes: int, adam_step: int,
                        lr: float, beta1: float, beta2: float, eps: float, seed: int, counter: int,
                        mask1: Optional[Tensor] = None, mask2: Optional[Tensor] = None) -> Tensor:
    """One fused train() iteration of largecnn on the device; returns the batch's log-probabilities (B, K).
    adam_step >= 1 applies torch.optim.Adam (that step index); 0 leaves params untouched."""
    a = L.LargeCnnArgs()
    a.seed, a.counter = int(seed), int(counter)
    a.mask1_in, a.mask2_in = _ptr(mask1), _ptr(mask2)
    return _flat_train_step("abd_largecnn", "largecnn", a, x, labels, indicators, params, grads, exp_avg, exp_avg_sq,
                            metrics, num_classes, adam_step, lr, beta1, beta2, eps)


@largecnn_train_step.register_fake
def _(x, labels, indicators, params, grads, exp_avg, exp_avg_sq, metrics, num_classes, adam_step, lr, beta1, beta2,
      eps, seed, counter, mask1=None, mask2=None):
    return x.new_empty((x.shape[0], num_classes))


def _resnet_eval(x, params, running, num_classes, labels, indicators, metrics):
    return _flat_eval("abd_resnet", "ResNet", x, params, (running,), num_classes, labels, indicators, metrics)


@torch.library.custom_op("abd::resnet_eval", mutates_args=())
def resnet_eval(x: Tensor, params: Tensor, running: Tensor, num_classes: int) -> Tensor:
    """model.eval() forward of ResNet: (B, 1, H, W) -> logits (B, K); running BN statistics, nothing updated."""
    return _resnet_eval(x, params, running, num_classes, None, None, None)


@resnet_eval.register_fake
def _(x, params, running, num_classes):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::resnet_eval_metrics", mutates_args=("metrics",))
def resnet_eval_metrics(x: Tensor, params: Tensor, running: Tensor, num_classes: int, labels: Tensor,
                        indicators: Optional[Tensor], metrics: Tensor) -> Tensor:
    """The eval forward plus test()'s loss / accuracy / ASR counters accumulated into metrics (int64[8]);
    returns the logits."""
    return _resnet_eval(x, params, running, num_classes, labels, indicators, metrics)


@resnet_eval_metrics.register_fake
def _(x, params, running, num_classes, labels, indicators, metrics):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::resnet_train_step",
                         mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "running", "num_batches_tracked",
                                       "metrics"))
def resnet_train_step(x: Tensor, labels: Tensor, indicators: Optional[Tensor], params: Tensor, grads: Tensor,
                      exp_avg: Tensor, exp_avg_sq: Tensor, running: Tensor, num_batches_tracked: Tensor,
                      metrics: Tensor, num_classes: int, adam_step: int, lr: float, beta1: float, beta2: float,
                      eps: float) -> Tensor:
    """One fused train() iteration of ResNet on the device; returns the batch's logits (B, K).
    adam_step >= 1 applies torch.optim.Adam (that step index); 0 leaves params untouched."""
    a = L.ResNetArgs()
    a.running, a.num_batches_tracked = running.data_ptr(), num_batches_tracked.data_ptr()
    return _flat_train_step("abd_resnet", "ResNet", a, x, labels, indicators, params, grads, exp_avg, exp_avg_sq,
                            metrics, num_classes, adam_step, lr, beta1, beta2, eps)


@resnet_train_step.register_fake
def _(x, labels, indicators, params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics, num_classes,
      adam_step, lr, beta1, beta2, eps):
    return x.new_empty((x.shape[0], num_classes))


def _smalllstm_eval(x, params, running, num_classes, labels, indicators, metrics):
    return _flat_eval("abd_smalllstm", "smalllstm", x, params, (running,), num_classes, labels, indicators, metrics)


@torch.library.custom_op("abd::smalllstm_eval", mutates_args=())
def smalllstm_eval(x: Tensor, params: Tensor, running: Tensor, num_classes: int) -> Tensor:
    """model.eval() forward of smalllstm: (B, 1, H, W) -> log-probabilities (B, K); running BN statistics, no
    dropout, nothing updated."""
    return _smalllstm_eval(x, params, running, num_classes, None, None, None)


@smalllstm_eval.register_fake
def _(x, params, running, num_classes):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::smalllstm_eval_metrics", mutates_args=("metrics",))
def smalllstm_eval_metrics(x: Tensor, params: Tensor, running: Tensor, num_classes: int, labels: Tensor,
                           indicators: Optional[Tensor], metrics: Tensor) -> Tensor:
    """The eval forward plus test()'s loss / accuracy / ASR counters accumulated into metrics (int64[8]);
    returns the log-probabilities."""
    return _smalllstm_eval(x, params, running, num_classes, labels, indicators, metrics)


@smalllstm_eval_metrics.register_fake
def _(x, params, running, num_classes, labels, indicators, metrics):
    return x.new_empty((x.shape[0], num_classes))


@torch.library.custom_op("abd::smalllstm_train_step",
                         mutates_args=("params", "grads", "exp_avg", "exp_avg_sq", "running", "num_batches_tracked",
                                       "metrics"))
def smalllstm_train_step(x: Tensor, labels: Tensor, indicators: Optional[Tensor], params: Tensor, grads: Tensor,
                         exp_avg: Tensor, exp_avg_sq: Tensor, running: Tensor, num_batches_tracked: Tensor,
                         metrics: Tensor, num_classes: int, adam_step: int, lr: float, beta1: float, beta2: float,
                         eps: float, seed: int, counter: int, mask: Optional[Tensor] = None) -> Tensor:
    """One fused train() iteration of smalllstm on the device; returns the batch's log-probabilities (B, K).
    adam_step >= 1 applies torch.optim.Adam (that step index); 0 leaves params untouched.  mask: a (B, 32, T, Wf)
    uint8 keep mask of drop1 in place of the device hash."""
    a = L.SmallLstmArgs()
    a.running, a.num_batches_tracked = running.data_ptr(), num_batches_tracked.data_ptr()
    a.seed, a.counter = int(seed), int(counter)
    a.mask_in = _ptr(mask)
    return _flat_train_step("abd_smalllstm", "smalllstm", a, x, labels, indicators, params, grads, exp_avg,
                            exp_avg_sq, metrics, num_classes, adam_step, lr, beta1, beta2, eps)


@smalllstm_train_step.register_fake
def _(x, labels, indicators, params, grads, exp_avg, exp_avg_sq, running, num_batches_tracked, metrics, num_classes,
      adam_step, lr, beta1, beta2, eps, seed, counter, mask=None):
    return x.new_empty((x.shape[0], num_classes))
