"""``largecnn`` on the HIP device (drop-in for reference utils/models.py:68-119).

Same submodules, names and constructor order as the reference, so construction consumes torch's RNG alike
(equal initial weights under a seed) and ``state_dict()`` keys / shapes are the reference's.  ``forward`` runs
libabd (csrc/largecnn.hip): conv1 as a direct kernel, conv2..conv5 as implicit GEMMs on the fp32 matrix pipe,
the three max pools, the fc head with its two dropouts and log_softmax; it returns log-probabilities like the
reference.

The 16 parameters are re-homed into ONE flat device buffer in ``named_parameters()`` order.  fp32 only: there is
no bf16 mode for this model.

Two ways in: build this class (``from abd_amd.models_largecnn import largecnn``), or hand a reference-built
``utils.models.largecnn`` to ``training.train`` / ``test`` / ``clean_train`` / ``clean_test``, which ``adopt`` it.
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch
import torch.nn as nn

from . import _flat, _lib as L
from .models import DROPOUT_SOURCES, dropout_step

CONVS = (("conv1", 1, 96), ("conv2", 96, 256), ("conv3", 256, 384), ("conv4", 384, 384), ("conv5", 384, 256))
FC1, FC2 = 256, 128
PARAM_ORDER = tuple(f"{m}.{p}" for m in ("conv1", "conv2", "conv3", "conv4", "conv5", "fc1", "fc2", "fc3")
                    for p in ("weight", "bias"))
N_PARAMS = len(PARAM_ORDER)
CHILDREN = ("conv1", "pool1", "conv2", "pool2", "conv3", "conv4", "conv5", "pool3", "flat", "fc1", "dropout1", "fc2",
            "dropout2", "fc3")
TILE_INFO = {"small_tile": 0, "large_tile": 1, "slice_rows": 2, "colsum_rows": 3, "large_min_blocks": 4,
             "max_slices": 5}


def tile_info(what: str) -> int:
    """Geometry of the built kernels (abd_largecnn_tile_info): 'small_tile' / 'large_tile' edge of the GEMM block
    tiles, 'slice_rows' least pixels of a weight-gradient slice, 'colsum_rows' rows above which column sums take
    two stages, 'large_min_blocks', 'max_slices'."""
    return int(L.lib().abd_largecnn_tile_info(TILE_INFO[what]))


def linear_features(H: int, W: int) -> int:
    """fc1's inputs for an (H, W) input (abd_largecnn_linear_features); -1 below 12 x 12."""
    return int(L.lib().abd_largecnn_linear_features(int(H), int(W)))


def net_handle(H: int, W: int, K: int):
    return _flat.net_handle("abd_largecnn", H, W, K)


class _Engine(_flat.FlatEngine):
    """The 16 parameters; no BatchNorm buffers.  T, F of the shared engine are the input's H, W."""

    def __init__(self, model: "largecnn", H: int, W: int, device: torch.device):
        super().__init__("abd_largecnn", N_PARAMS, H, W, model.fc3.out_features, device)


class largecnn(_flat.FlatModule, nn.Module):
    """Reference-compatible largecnn whose forward/backward run on libabd (HIP)."""

    NAME, TRANSIENT = "largecnn", ("_host_masks",)
    PARAM_ORDER, ARGS, ENGINE = PARAM_ORDER, L.LargeCnnArgs, _Engine
    BACKWARD_ORDER = ("largecnn backward must directly follow its train-mode forward (activations live in the shared "
                      "workspace)")
    STATE = _flat.DROPOUT_STATE + (("dropout_source", "device"),)

    def __init__(self, num_classes, linear_features):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels=1, out_channels=96, kernel_size=(3, 3), stride=1, padding=1)
        self.pool1 = nn.MaxPool2d(kernel_size=(2, 2))
        self.conv2 = nn.Conv2d(in_channels=96, out_channels=256, kernel_size=(3, 3), stride=1, padding=1)
        self.pool2 = nn.MaxPool2d(kernel_size=(2, 2))
        self.conv3 = nn.Conv2d(in_channels=256, out_channels=384, kernel_size=(3, 3), stride=1, padding=1)
        self.conv4 = nn.Conv2d(in_channels=384, out_channels=384, kernel_size=(3, 3), stride=1, padding=1)
        self.conv5 = nn.Conv2d(in_channels=384, out_channels=256, kernel_size=(3, 3), stride=1, padding=1)
        self.pool3 = nn.MaxPool2d(kernel_size=(3, 3), stride=(2, 2))
        self.flat = nn.Flatten()
        self.fc1 = nn.Linear(in_features=linear_features, out_features=FC1)
        self.dropout1 = nn.Dropout(0.5)
        self.fc2 = nn.Linear(in_features=FC1, out_features=FC2)
        self.dropout2 = nn.Dropout(0.5)
        self.fc3 = nn.Linear(in_features=FC2, out_features=num_classes)
        self._init_abd()

    # ------------------------------------------------------------------ settings
    def set_dropout_source(self, source: str):
        """'device' (default): the keep-masks come from the counter-based hash on the GPU.  'torch_cpu':
        bernoulli_(0.5) on (B, 256) then (B, 128) from the global CPU generator, as the reference's CPU forward
        draws them, copied to the device each step."""
        if source not in DROPOUT_SOURCES:
            raise ValueError(f"dropout source must be one of {DROPOUT_SOURCES}, got {source!r}")
        self.dropout_source = source
        return self

    def step_masks(self, batch: int, device):
        """Host-drawn masks for the next train-mode forward, or None (device hash)."""
        if getattr(self, "dropout_source", "device") != "torch_cpu":
            return None
        m1 = torch.empty((batch, FC1)).bernoulli_(0.5).to(torch.uint8)
        m2 = torch.empty((batch, FC2)).bernoulli_(0.5).to(torch.uint8)
        return m1.to(device, non_blocking=True), m2.to(device, non_blocking=True)

    # ------------------------------------------------------------------ binding
    def engine(self, x: torch.Tensor) -> _Engine:
        """Bind (or re-bind) the parameters to the flat device buffer for x's geometry."""
        H, W = int(x.shape[-2]), int(x.shape[-1])
        want = linear_features(H, W)
        if want != self.fc1.in_features:
            raise ValueError(f"input ({H}, {W}) gives fc1 {want} features but the model was built for "
                             f"linear_features {self.fc1.in_features}")
        return self._bind_dropout(H, W, x.device)

    # ------------------------------------------------------------------ launches
    def hip_forward(self, x, train: bool, seed: int | None = None, masks=None, masks_out=None):
        """The log-probabilities.  train: dropout on, every activation kept in the engine's workspace for
        hip_backward; masks: (mask1 (B, 256), mask2 (B, 128)) uint8 keep-masks in place of the hash."""
        eng = self.engine(x)
        B = x.shape[0]
        if not train:
            from . import ops  # noqa: F401  (registers torch.ops.abd)
            return torch.ops.abd.largecnn_eval(x, eng.params, eng.K)
        out = torch.empty((B, eng.K), dtype=torch.float32, device=x.device)
        ws = eng.workspace(B)
        a = self._args(eng, x, B)
        a.logits_out = out.data_ptr()
        dropout_step(self, a, x.device, seed)
        if masks is None:
            masks = self.step_masks(B, x.device)
            self._host_masks = masks  # keep alive until the launch has consumed them
        if masks is not None:
            a.mask1_in, a.mask2_in = masks[0].data_ptr(), masks[1].data_ptr()
        if masks_out is not None:
            a.mask1_out, a.mask2_out = masks_out[0].data_ptr(), masks_out[1].data_ptr()
        eng.call("forward", C.byref(a), 1, ws.data_ptr(), ws.numel(), L.stream_ptr(x.device))
        eng.token += 1
        eng.last_train_token = eng.token
        return out

    def hip_train_forward(self, x):
        return self.hip_forward(x, train=True)


# ------------------------------------------------------------------ adoption of a reference-built instance
_ADOPTED: "weakref.WeakKeyDictionary[nn.Module, largecnn]" = weakref.WeakKeyDictionary()


def _refuse(why: str):
    raise L.AbdError(f"not the reference's largecnn: {why}")


def _check_structure(m: nn.Module):
    for name, cin, cout in CONVS:
        _flat.check_conv3x3(m, name, cin, cout, 1, True, _refuse)
    for name, k, s in (("pool1", 2, 2), ("pool2", 2, 2), ("pool3", 3, 2)):
        p = getattr(m, name, None)
        if not isinstance(p, nn.MaxPool2d):
            _refuse(f"{name} is missing or no MaxPool2d")
        stride = p.stride if p.stride is not None else p.kernel_size
        if (_flat.pair(p.kernel_size) != (k, k) or _flat.pair(stride) != (s, s) or _flat.pair(p.padding) != (0, 0)
                or _flat.pair(p.dilation) != (1, 1) or p.ceil_mode or p.return_indices):
            _refuse(f"{name} is not MaxPool2d({k}, stride {s})")
    for name in ("fc1", "fc2", "fc3"):
        f = getattr(m, name, None)
        if not isinstance(f, nn.Linear) or f.bias is None:
            _refuse(f"{name} is missing or no Linear with bias")
    if m.fc1.out_features != FC1 or (m.fc2.in_features, m.fc2.out_features) != (FC1, FC2) or m.fc3.in_features != FC2:
        _refuse("the head is not fc1(-> 256), fc2(256 -> 128), fc3(128 -> classes)")
    if m.fc1.in_features % 256 or m.fc1.in_features < 256:
        _refuse(f"linear_features {m.fc1.in_features} is no multiple of conv5's 256 channels")
    for name in ("dropout1", "dropout2"):
        d = getattr(m, name, None)
        if not isinstance(d, nn.Dropout) or d.p != 0.5:
            _refuse(f"{name} is missing or no Dropout(0.5)")
    if [n for n, _ in m.named_parameters()] != list(PARAM_ORDER) or any(True for _ in m.buffers()):
        _refuse("it has other parameters or buffers than conv1..conv5, fc1..fc3")
    if any(p.dtype != torch.float32 for p in m.parameters()):
        _refuse("its parameters are not float32")


def adopt(module: nn.Module) -> largecnn:
    """The abd ``largecnn`` that runs a reference-built ``utils.models.largecnn`` instance on libabd.

    The structure is checked (type name ``largecnn``; conv1..conv5, the three pools, fc1..fc3 and the two
    dropouts with exactly the reference's shapes and hyper-parameters), anything else raises AbdError.  The
    result's submodules ARE the instance's own, so the ``Parameter`` objects the script's optimizer holds are the
    ones re-homed into the flat buffer: after training the script's object sees the trained weights and its own
    ``forward`` still works.  One adoption per instance (a weak cache; the instance itself is not touched)."""
    if isinstance(module, largecnn):
        return module
    if not adoptable(module):
        _refuse(f"got {type(module).__name__}")
    return _flat.adopt_into(
        largecnn, module, CHILDREN, _ADOPTED, _check_structure,
        lambda got, m: all(getattr(got, n) is getattr(m, n, None) for n in CHILDREN if n != "flat"),
        fill=lambda name: nn.Flatten())   # the reference's forward flattens with view(); only `flat` may be missing


def adoptable(module) -> bool:
    """A module ``adopt`` would look at: named largecnn, but not this package's class."""
    return _flat.adoptable(module, largecnn)
