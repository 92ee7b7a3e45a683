"""``RNN`` on the HIP device (drop-in for reference utils/models.py:231-257).

Same submodules, names, constructor order and attributes (``lstm``, ``fc``, ``hidden_size``,
``num_layers``) as the reference, so construction consumes torch's RNG alike (equal initial weights
under a seed) and ``state_dict()`` keys / shapes are the reference's.  ``forward`` runs libabd
(csrc/rnn.hip): a 3-layer unidirectional 768-wide LSTM from zero initial states -- one LDS-tiled fp32
MFMA GEMM per layer for the input projections, one launch per time step for the recurrence -- and the
linear classifier on the last time step; it returns raw logits like the reference.

The 14 parameters are re-homed into ONE flat device buffer in ``named_parameters()`` order.  fp32 only:
there is no bf16 mode for this model.  The model has no BatchNorm and no dropout, so the train-mode and
the eval-mode forward compute the same logits.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L

HIDDEN, LAYERS = 768, 3
PARAM_ORDER = (
    *[f"lstm.{n}_l{k}" for k in range(LAYERS) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")],
    "fc.weight", "fc.bias",
)
N_PARAMS = len(PARAM_ORDER)
TILE_INFO = {"rec_rows": 0, "small_tile": 1, "large_tile": 2, "slice_rows": 3, "colsum_rows": 4,
             "large_min_blocks": 5}


def tile_info(what: str) -> int:
    """Geometry of the built kernels (abd_rnn_tile_info): 'rec_rows' batch rows of a recurrent workgroup,
    'small_tile' / 'large_tile' edge of the GEMM block tiles, 'slice_rows' least rows of a weight-gradient
    slice, 'colsum_rows' rows above which column sums take two stages, 'large_min_blocks'."""
    return int(L.lib().abd_rnn_tile_info(TILE_INFO[what]))


def tile_rows() -> int:
    """Batch rows one workgroup of the recurrent step kernel owns."""
    return tile_info("rec_rows")


def net_handle(T: int, F: int, K: int):
    h = C.c_void_p()
    L.check(L.lib().abd_rnn_create(int(T), int(F), int(K), C.byref(h)), "abd_rnn_create")
    return h


class _Engine:
    """libabd network handle + flat device buffers for one (T, F, K) geometry."""

    def __init__(self, model: "RNN", T: int, F: int, device: torch.device):
        lib = L.lib()
        self.T, self.F, self.K = T, F, model.fc.out_features
        self.device = device
        self.h = net_handle(T, F, self.K)
        offs = (C.c_int64 * (N_PARAMS + 1))()
        L.check(lib.abd_rnn_param_offsets(self.h, offs), "abd_rnn_param_offsets")
        self.offsets = list(offs)
        self.n = self.offsets[-1]
        self.params = torch.empty(self.n, dtype=torch.float32, device=device)
        self.grads = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.exp_avg = None
        self.exp_avg_sq = None
        self._ws = None
        self.token = 0
        self.last_train_token = -1

    def workspace(self, batch):
        """The shared activation workspace: about 5.9 KB per (row, step), 1.5 GB at B = 256, T = 100."""
        need = L.lib().abd_rnn_workspace_bytes(self.h, int(batch))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def views(self, buf):
        return [buf[self.offsets[i]:self.offsets[i + 1]] for i in range(N_PARAMS)]

    def __del__(self):
        try:
            if self.h and self.h.value:
                L.lib().abd_rnn_destroy(self.h)
        except Exception:
            pass


class RNN(nn.Module):
    """Reference-compatible RNN whose forward/backward run on libabd (HIP)."""

    def __init__(self, num_classes, time_len):
        super().__init__()
        self.hidden_size = HIDDEN
        self.num_layers = LAYERS
        self.lstm = nn.LSTM(time_len, HIDDEN, LAYERS, batch_first=True)
        self.fc = nn.Linear(HIDDEN, num_classes)
        self._engine = None
        self.gemm_precision = "f32"

    # ------------------------------------------------------------------ settings
    def set_gemm_precision(self, precision: str):
        """fp32 products only ('f32', or 'f32split' which names the same accuracy class): 'bf16' raises
        AbdError."""
        if precision not in L.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(L.PRECISIONS)}, got {precision!r}")
        if precision == "bf16":
            raise L.AbdError("RNN has no bf16 mode: every product is fp32 (DESIGN.md §5)")
        return self

    def __setstate__(self, state):
        # also the target of reference-format checkpoints (training.reference_pickle_object)
        super().__setstate__(state)
        for k, v in (("_engine", None), ("gemm_precision", "f32"), ("hidden_size", HIDDEN), ("num_layers", LAYERS)):
            if k not in self.__dict__:
                self.__dict__[k] = v

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_engine"] = None
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
        return True

    def engine(self, x: torch.Tensor) -> _Engine:
        """Bind (or re-bind) the parameters to the flat device buffer for x's geometry."""
        T, F = int(x.shape[-2]), int(x.shape[-1])
        if F != self.lstm.input_size:
            raise ValueError(f"input has {F} features but the model was built for time_len {self.lstm.input_size}")
        eng = self._engine
        if eng is not None and (eng.T, eng.F) == (T, F) and eng.device == x.device and self._bound(eng):
            return eng
        new = _Engine(self, T, F, x.device)
        with torch.no_grad():
            for p, v in zip(self._param_list(), new.views(new.params)):
                v.copy_(p.data.reshape(-1))
                p.data = v.view(p.shape)
        # nn.LSTM caches a flattened copy of its weights for the vendor RNN kernels; they are views now
        self.lstm._flat_weights = [getattr(self.lstm, n) for n in self.lstm._flat_weights_names]
        self._engine = new
        return new

    # ------------------------------------------------------------------ launches
    def _args(self, eng, x, B):
        a = L.RnnArgs()
        a.x = x.data_ptr()
        a.batch = B
        a.params = eng.params.data_ptr()
        a.grads = eng.grads.data_ptr()
        a.grad_scale = 1.0
        return a

    def _prepare(self, x):
        """The reference's own input handling (x.squeeze(1); x.float()) for a (B, 1, T, F) batch."""
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError("RNN expects (B, 1, T, n_mfcc)")
        if x.dtype != torch.float32:
            x = x.float()
        L.require_device(x, "RNN input")
        return x

    def forward(self, x):
        x = self._prepare(x)
        self.engine(x)
        if self.training and torch.is_grad_enabled():
            return _RnnFunction.apply(x, self, *self._param_list())
        from . import ops  # noqa: F401  (registers torch.ops.abd)
        return torch.ops.abd.rnn_eval(x, self._engine.params, self._engine.K)

    def hip_forward(self, x):
        """Forward that keeps every activation in the engine's workspace for hip_backward."""
        eng = self.engine(x)
        B = x.shape[0]
        out = torch.empty((B, eng.K), dtype=torch.float32, device=x.device)
        ws = eng.workspace(B)
        a = self._args(eng, x, B)
        a.logits_out = out.data_ptr()
        rc = L.lib().abd_rnn_forward(eng.h, C.byref(a), ws.data_ptr(), ws.numel(), L.stream_ptr(x.device))
        L.check(rc, "abd_rnn_forward")
        eng.token += 1
        eng.last_train_token = eng.token
        return out

    def hip_backward(self, x, dlogits, token):
        eng = self._engine
        if eng is None or token != eng.last_train_token:
            raise L.AbdError("RNN backward must directly follow its forward (activations live in the shared "
                             "workspace, and backward consumes them)")
        eng.last_train_token = -1   # the saved gates now hold the gate gradients
        B = x.shape[0]
        ws = eng.workspace(B)
        a = self._args(eng, x, B)
        dl = dlogits.contiguous()
        rc = L.lib().abd_rnn_backward(eng.h, C.byref(a), dl.data_ptr(), ws.data_ptr(), ws.numel(),
                                     L.stream_ptr(x.device))
        L.check(rc, "abd_rnn_backward")
        return eng.views(eng.grads)


class _RnnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, model, *params):
        out = model.hip_forward(x)
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
