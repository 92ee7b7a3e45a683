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

from . import _lib as L
from .models import DROPOUT_SOURCES, draw_dropout_nonce, dropout_seed

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
    h = C.c_void_p()
    L.check(L.lib().abd_lstmattn_create(int(T), int(F), int(K), C.byref(h)), "abd_lstmattn_create")
    return h


class _Engine:
    """libabd network handle + flat device buffers for one (T, F, K) geometry."""

    def __init__(self, model: "lstmwithattention", T: int, F: int, device: torch.device):
        lib = L.lib()
        self.T, self.F, self.K = T, F, model.output.out_features
        self.device = device
        self.h = net_handle(T, F, self.K)
        offs = (C.c_int64 * (N_PARAMS + 1))()
        L.check(lib.abd_lstmattn_param_offsets(self.h, offs), "abd_lstmattn_param_offsets")
        self.offsets = list(offs)
        self.n = self.offsets[-1]
        self.params = torch.empty(self.n, dtype=torch.float32, device=device)
        self.grads = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.exp_avg = None
        self.exp_avg_sq = None
        self.running = torch.empty(22, dtype=torch.float32, device=device)
        self.nbt = torch.zeros(2, dtype=torch.int64, device=device)
        self._ws = None
        self.token = 0
        self.last_train_token = -1

    def workspace(self, batch):
        need = L.lib().abd_lstmattn_workspace_bytes(self.h, int(batch))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def views(self, buf):
        return [buf[self.offsets[i]:self.offsets[i + 1]] for i in range(N_PARAMS)]

    def __del__(self):
        try:
            if self.h and self.h.value:
                L.lib().abd_lstmattn_destroy(self.h)
        except Exception:
            pass


class lstmwithattention(nn.Module):
    """Reference-compatible lstmwithattention whose forward/backward run on libabd (HIP)."""

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
        self._engine = None
        self._step = 0
        self._dropout_nonce = None
        self.gemm_precision = "f32"
        self.dropout_source = "device"

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

    def __setstate__(self, state):
        # also the target of reference-format checkpoints (training.reference_pickle_object)
        super().__setstate__(state)
        for k, v in (("_engine", None), ("_step", 0), ("gemm_precision", "f32"), ("dropout_source", "device"),
                     ("_dropout_nonce", None)):
            if k not in self.__dict__:
                self.__dict__[k] = v

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_engine"] = None
        st.pop("_host_mask", None)
        return st

    # ------------------------------------------------------------------ binding
    def _param_list(self):
        d = dict(self.named_parameters())
        return [d[n] for n in PARAM_ORDER]

    def _bound(self, eng) -> bool:
        if eng is None:
            return False
        base = eng.params.data_ptr()
        for p, off in zip(self._param_list(), eng.offsets):
            if p.data.data_ptr() != base + 4 * off or p.device != eng.device:
                return False
        rbase = eng.running.data_ptr()
        o = 0
        for name, c in RUNNING_ORDER:
            bn = getattr(self, name)
            if bn.running_mean.data_ptr() != rbase + 4 * o or bn.running_var.data_ptr() != rbase + 4 * (o + c):
                return False
            o += 2 * c
        return True

    def engine(self, x: torch.Tensor) -> _Engine:
        """Bind (or re-bind) the parameters to flat device buffers for x's geometry."""
        T, F = int(x.shape[-2]), int(x.shape[-1])
        if T != self.dense2.in_features or F != self.rnn1.input_size:
            raise ValueError(f"input (T, F) = ({T}, {F}) but the model was built for seq_len "
                             f"{self.dense2.in_features}, time_len {self.rnn1.input_size}")
        eng = self._engine
        if eng is not None and (eng.T, eng.F) == (T, F) and eng.device == x.device and self._bound(eng):
            return eng
        new = _Engine(self, T, F, x.device)
        if getattr(self, "_dropout_nonce", None) is None:
            self._dropout_nonce = draw_dropout_nonce(x.device)
        with torch.no_grad():
            for p, v in zip(self._param_list(), new.views(new.params)):
                v.copy_(p.data.reshape(-1))
                p.data = v.view(p.shape)
            o = 0
            for i, (name, c) in enumerate(RUNNING_ORDER):
                bn = getattr(self, name)
                new.running[o:o + c].copy_(bn.running_mean)
                new.running[o + c:o + 2 * c].copy_(bn.running_var)
                bn.running_mean = new.running[o:o + c]
                bn.running_var = new.running[o + c:o + 2 * c]
                new.nbt[i].copy_(bn.num_batches_tracked)
                bn.num_batches_tracked = new.nbt[i]
                o += 2 * c
        # nn.LSTM caches a flattened copy of its weights for the vendor RNN kernels; they are views now
        for rnn in (self.rnn1, self.rnn2):
            rnn._flat_weights = [getattr(rnn, n) for n in rnn._flat_weights_names]
        self._engine = new
        return new

    # ------------------------------------------------------------------ launches
    def _args(self, eng, x, B):
        a = L.LstmAttnArgs()
        a.x = x.data_ptr()
        a.batch = B
        a.params = eng.params.data_ptr()
        a.grads = eng.grads.data_ptr()
        a.running = eng.running.data_ptr()
        a.num_batches_tracked = eng.nbt.data_ptr()
        a.grad_scale = 1.0
        return a

    def _check_input(self, x):
        L.require_device(x, "lstmwithattention input")
        if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
            raise ValueError("lstmwithattention expects (B, 1, T, n_mfcc) float32")

    def forward(self, x):
        self._check_input(x)
        self.engine(x)
        if self.training and torch.is_grad_enabled():
            return _LstmAttnFunction.apply(x, self, *self._param_list())
        return self.hip_forward(x, train=self.training)

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
        a.seed = dropout_seed(x.device, self) if seed is None else seed
        a.counter = self._step
        self._step += 1
        if mask is None:
            mask = self.step_mask(B, x.device)
            self._host_mask = mask  # keep alive until the launch has consumed it
        if mask is not None:
            a.mask_in = mask.data_ptr()
        if mask_out is not None:
            a.mask_out = mask_out.data_ptr()
        rc = L.lib().abd_lstmattn_forward(eng.h, C.byref(a), 1, ws.data_ptr(), ws.numel(), L.stream_ptr(x.device))
        L.check(rc, "abd_lstmattn_forward")
        eng.token += 1
        eng.last_train_token = eng.token
        return out

    def hip_backward(self, x, dlogits, token):
        eng = self._engine
        if eng is None or token != eng.last_train_token:
            raise L.AbdError("lstmwithattention backward must directly follow its train-mode forward (activations "
                             "live in the shared workspace)")
        B = x.shape[0]
        ws = eng.workspace(B)
        a = self._args(eng, x, B)
        dl = dlogits.contiguous()
        rc = L.lib().abd_lstmattn_backward(eng.h, C.byref(a), dl.data_ptr(), ws.data_ptr(), ws.numel(),
                                          L.stream_ptr(x.device))
        L.check(rc, "abd_lstmattn_backward")
        return eng.views(eng.grads)


class _LstmAttnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, model, *params):
        out = model.hip_forward(x, train=True)
        ctx.model = model
        ctx.token = model._engine.last_train_token
        ctx.save_for_backward(x)
        ctx.shapes = [p.shape for p in params]
        return out

    @staticmethod
    def backward(ctx, dl):
        (x,) = ctx.saved_tensors
        gs = ctx.model.hip_backward(x, dl, ctx.token)
        return (None, None, *[g.view(s).clone() for g, s in zip(gs, ctx.shapes)])
