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

from . import _flat, _lib as L

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
    return _flat.net_handle("abd_rnn", T, F, K)


class _Engine(_flat.FlatEngine):
    """The 14 parameters; no BatchNorm buffers."""

    def __init__(self, model: "RNN", T: int, F: int, device: torch.device):
        super().__init__("abd_rnn", N_PARAMS, T, F, model.fc.out_features, device)


class RNN(_flat.FlatModule, nn.Module):
    """Reference-compatible RNN whose forward/backward run on libabd (HIP)."""

    NAME = "RNN"
    PARAM_ORDER, ARGS, ENGINE = PARAM_ORDER, L.RnnArgs, _Engine
    BACKWARD_ORDER = ("RNN backward must directly follow its forward (activations live in the shared workspace, and "
                      "backward consumes them)")
    BACKWARD_CONSUMES = True   # the saved gates hold the gate gradients afterwards

    def __init__(self, num_classes, time_len):
        super().__init__()
        self.hidden_size = HIDDEN
        self.num_layers = LAYERS
        self.lstm = nn.LSTM(time_len, HIDDEN, LAYERS, batch_first=True)
        self.fc = nn.Linear(HIDDEN, num_classes)
        self._engine = None
        self.gemm_precision = "f32"

    # ------------------------------------------------------------------ settings
    def __setstate__(self, state):
        # also the target of reference-format checkpoints (training.reference_pickle_object)
        super().__setstate__(state)
        for k, v in (("_engine", None), ("gemm_precision", "f32"), ("hidden_size", HIDDEN), ("num_layers", LAYERS)):
            if k not in self.__dict__:
                self.__dict__[k] = v

    # ------------------------------------------------------------------ binding
    def engine(self, x: torch.Tensor) -> _Engine:
        """Bind (or re-bind) the parameters to the flat device buffer for x's geometry."""
        T, F = int(x.shape[-2]), int(x.shape[-1])
        if F != self.lstm.input_size:
            raise ValueError(f"input has {F} features but the model was built for time_len {self.lstm.input_size}")
        return self._bind(T, F, x.device)

    # ------------------------------------------------------------------ launches
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
            return _flat.FlatFunction.apply(x, self, *self._param_list())
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
        eng.call("forward", C.byref(a), ws.data_ptr(), ws.numel(), L.stream_ptr(x.device))
        eng.token += 1
        eng.last_train_token = eng.token
        return out

    hip_train_forward = hip_forward
