"""``lstmwithattention`` on the HIP device (drop-in for reference utils/models.py:180-228).

Same submodules, names and constructor order as the reference, so construction consumes torch's
RNG alike (equal initial weights under a seed) and ``state_dict()`` keys / shapes are the
reference's.  ``forward`` runs libabd (csrc/lstm_attn.hip): the (5,1) convs + BatchNorm, two
bidirectional LSTM layers whose recurrence keeps W_hh in LDS for the whole sequence, the attention
head and the dense classifier; it returns raw logits like the reference.

The 34 parameters are re-homed into ONE flat device buffer in ``named_parameters()`` order, the BN
running statistics into a 22-float buffer, as ``models.smallcnn`` does.  fp32 only: there is no bf16
mode for this model.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _flat, _lib as L
from .models import DROPOUT_SOURCES, dropout_step

_RNN = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
        "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")
PARAM_ORDER = (
    "conv1.weight", "conv1.bias", "batchnorm1.weight", "batchnorm1.bias",
    "conv2.weight", "conv2.bias", "batchnorm2.weight", "batchnorm2.bias",
    *[f"rnn1.{n}" for n in _RNN], *[f"rnn2.{n}" for n in _RNN],
    "dense1.weight", "dense1.bias", "attention.weight", "attention.bias", "dense2.weight", "dense2.bias",
    "dense3.weight", "dense3.bias", "output.weight", "output.bias",
)
RUNNING_ORDER = (("batchnorm1", 10), ("batchnorm2", 1))
N_PARAMS = len(PARAM_ORDER)


def tile_rows() -> int:
    """Batch rows one workgroup of the recurrent kernels carries through the sequence."""
    return int(L.lib().abd_lstmattn_tile_rows())


def net_handle(T: int, F: int, K: int):
    return _flat.net_handle("abd_lstmattn", T, F, K)


class _Engine(_flat.FlatEngine):
    """The 34 parameters, the 22 running statistics and the two num_batches_tracked counters."""

    def __init__(self, model: "lstmwithattention", T: int, F: int, device: torch.device):
        super().__init__("abd_lstmattn", N_PARAMS, T, F, model.output.out_features, device, running=22, nbt=2)


class lstmwithattention(_flat.FlatModule, nn.Module):
    """Reference-compatible lstmwithattention whose forward/backward run on libabd (HIP)."""

    NAME, TRANSIENT = "lstmwithattention", ("_host_mask",)
    PARAM_ORDER, RUNNING_ORDER, ARGS, ENGINE = PARAM_ORDER, RUNNING_ORDER, L.LstmAttnArgs, _Engine
    BACKWARD_ORDER = ("lstmwithattention backward must directly follow its train-mode forward (activations live in "
                      "the shared workspace)")
    STATE = _flat.DROPOUT_STATE + (("dropout_source", "device"),)

    def __init__(self, classes, time_len, seq_len):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels=1, out_channels=10, kernel_size=(5, 1), padding='same')
        self.batchnorm1 = nn.BatchNorm2d(10)
        self.conv2 = nn.Conv2d(in_channels=10, out_channels=1, kernel_size=(5, 1), padding='same')
        self.batchnorm2 = nn.BatchNorm2d(1)
        self.rnn1 = nn.LSTM(input_size=time_len, hidden_size=64, bidirectional=True, batch_first=True)
        self.rnn2 = nn.LSTM(input_size=128, hidden_size=64, bidirectional=True, batch_first=True)
        self.dense1 = nn.Linear(128, 128)
        self.attention = nn.Linear(128, 128)
        self.dense2 = nn.Linear(seq_len, 64)
        self.dropout = nn.Dropout(0.5)
        self.dense3 = nn.Linear(64, 32)
        self.output = nn.Linear(32, classes)
        self._init_abd()

    # ------------------------------------------------------------------ settings
    def set_gemm_precision(self, precision: str):
        """fp32 products only ('f32', or 'f32split' which names the same accuracy class): the
        recurrence has no reduced-precision mode, so 'bf16' raises AbdError."""
        if precision not in L.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(L.PRECISIONS)}, got {precision!r}")
        if precision == "bf16":
            raise L.AbdError("lstmwithattention has no bf16 mode: every product is fp32 (DESIGN.md §5)")
        return self

    def set_dropout_source(self, source: str):
        """'device' (default): the keep-mask comes from the counter-based hash on the GPU.
        'torch_cpu': bernoulli_(0.5) on (B, 64) from the global CPU generator, as the reference's CPU
        forward draws it, copied to the device each step."""
        if source not in DROPOUT_SOURCES:
            raise ValueError(f"dropout source must be one of {DROPOUT_SOURCES}, got {source!r}")
        self.dropout_source = source
        return self

    def step_mask(self, batch: int, device):
        """Host-drawn mask for the next train-mode forward, or None (device hash)."""
        if getattr(self, "dropout_source", "device") != "torch_cpu":
            return None
        return torch.empty((batch, 64)).bernoulli_(0.5).to(torch.uint8).to(device, non_blocking=True)

    # ------------------------------------------------------------------ binding
    def engine(self, x: torch.Tensor) -> _Engine:
        """Bind (or re-bind) the parameters to flat device buffers for x's geometry."""
        T, F = int(x.shape[-2]), int(x.shape[-1])
        if T != self.dense2.in_features or F != self.rnn1.input_size:
            raise ValueError(f"input (T, F) = ({T}, {F}) but the model was built for seq_len "
                             f"{self.dense2.in_features}, time_len {self.rnn1.input_size}")
        return self._bind_dropout(T, F, x.device)

    # ------------------------------------------------------------------ launches
    def _check_input(self, x):
        L.require_device(x, "lstmwithattention input")
        if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
            raise ValueError("lstmwithattention expects (B, 1, T, n_mfcc) float32")

    def hip_forward(self, x, train: bool, seed: int | None = None, mask=None, mask_out=None):
        eng = self.engine(x)
        B = x.shape[0]
        if not train:
            from . import ops  # noqa: F401  (registers torch.ops.abd)
            return torch.ops.abd.lstmattn_eval(x, eng.params, eng.running, eng.K)
        out = torch.empty((B, eng.K), dtype=torch.float32, device=x.device)
        ws = eng.workspace(B)
        a = self._args(eng, x, B)
        a.logits_out = out.data_ptr()
        dropout_step(self, a, x.device, seed, mask, mask_out)
        if mask is None:
            self._host_mask = self.step_mask(B, x.device)  # kept alive until the launch has consumed it
            if self._host_mask is not None:
                a.mask_in = self._host_mask.data_ptr()
        eng.call("forward", C.byref(a), 1, ws.data_ptr(), ws.numel(), L.stream_ptr(x.device))
        eng.token += 1
        eng.last_train_token = eng.token
        return out

    def hip_train_forward(self, x):
        return self.hip_forward(x, train=True)
