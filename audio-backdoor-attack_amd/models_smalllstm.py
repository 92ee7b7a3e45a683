"""``smalllstm`` on the HIP device (drop-in for reference utils/models.py:121-178).

Same submodules, names and constructor order as the reference, so construction consumes torch's RNG alike (equal
initial weights under a seed) and ``state_dict()`` keys / shapes are the reference's, running buffers and the
unused ``fc1`` included.  ``forward`` runs libabd (csrc/smalllstm.hip): conv1 as a direct kernel, conv2 and conv3 as
implicit GEMMs on the fp32 matrix pipe, ReLU before train-mode BatchNorm, the three max pools, dropout, the 2-layer
128-wide LSTM with one launch per layer for the whole sequence, fc2 on the last step and log_softmax; it returns
log-probabilities like the reference, in both modes.

The 24 parameters are re-homed into ONE flat device buffer in ``named_parameters()`` order, the three BatchNorms'
running statistics into a 320-float buffer.  ``fc1`` is a parameter the forward never reads: in the reference its
``.grad`` stays ``None`` and Adam skips it; here its gradient is a view of exact zeros, Adam from zero moments
leaves it bit-unchanged, and the one visible difference is that ``optimizer.state`` gets entries for it.  fp32
only: there is no bf16 mode for this model.

Two ways in: build this class (``from abd_amd.models_smalllstm import smalllstm``), or hand a reference-built
``utils.models.smalllstm`` to ``training.train`` / ``test`` / ``clean_train`` / ``clean_test``, which ``adopt`` it.
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch
import torch.nn as nn

from . import _flat, _lib as L
from .models import dropout_step

HIDDEN, LAYERS, FC1_IN, DROP_P = 128, 2, 224, 0.4
# (conv, bn, Cin, Cout)
CONVS = (("conv1", "bn1", 1, 64), ("conv2", "bn2", 64, 64), ("conv3", "bn3", 64, 32))
# (pool, kernel, padding)
POOLS = (("pool1", (1, 3), (0, 0)), ("pool2", (2, 2), (1, 1)), ("pool3", (2, 2), (0, 1)))
PARAM_ORDER = tuple(f"{m}.{p}" for cv, bn, *_ in CONVS for m in (cv, bn) for p in ("weight", "bias")) + tuple(
    f"rnn.{p}_l{l}" for l in range(LAYERS) for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) + (
    "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
RUNNING_ORDER = tuple((bn, cout) for _, bn, _, cout in CONVS)
N_PARAMS = len(PARAM_ORDER)
N_RUNNING = 2 * sum(c for _, c in RUNNING_ORDER)
BUFFER_ORDER = tuple(f"{bn}.{b}" for bn, _ in RUNNING_ORDER for b in ("running_mean", "running_var",
                                                                      "num_batches_tracked"))
CHILDREN = ("conv1", "bn1", "pool1", "conv2", "bn2", "pool2", "conv3", "bn3", "pool3", "drop1", "flat", "rnn", "fc1",
            "drop2", "fc2", "softmax")
TILE_INFO = {"tile_rows": 0, "k_step": 1, "slice_rows": 2, "max_slices": 3, "stat_rows": 4, "stat_blocks": 5,
             "rec_rows": 6, "small_tile": 7, "large_tile": 8, "gemm_k_step": 9, "gemm_slices": 10, "colsum_rows": 11,
             "large_min_blocks": 12}
MIN_H, MIN_W = 6, 10


def tile_info(what: str) -> int:
    """Geometry of the built kernels (abd_smalllstm_tile_info): 'tile_rows' rows of a conv block tile, 'k_step' the
    convs' K-step, 'slice_rows' least rows of a weight-gradient slice, 'max_slices' of a conv weight gradient,
    'stat_rows' least pixels of a BatchNorm partial block, 'stat_blocks' most such blocks, 'rec_rows' batch rows of
    a recurrent workgroup, 'small_tile' / 'large_tile' / 'gemm_k_step' of the GEMMs, 'gemm_slices' most slices of
    an LSTM weight gradient, 'colsum_rows', 'large_min_blocks'."""
    return int(L.lib().abd_smalllstm_tile_info(TILE_INFO[what]))


def rnn_features(H: int, W: int) -> int:
    """The LSTM's input width for an (H, W) input (abd_smalllstm_rnn_features); -1 below 6 x 10."""
    return int(L.lib().abd_smalllstm_rnn_features(int(H), int(W)))


def net_handle(H: int, W: int, K: int):
    return _flat.net_handle("abd_smalllstm", H, W, K)


class _Engine(_flat.FlatEngine):
    """The 24 parameters, the 320 running statistics and the three num_batches_tracked counters.  T, F of the
    shared engine are the input's H, W."""

    def __init__(self, model: "smalllstm", H: int, W: int, device: torch.device):
        super().__init__("abd_smalllstm", N_PARAMS, H, W, model.fc2.out_features, device, running=N_RUNNING,
                         nbt=len(RUNNING_ORDER))


class smalllstm(_flat.FlatModule, nn.Module):
    """Reference-compatible smalllstm whose forward/backward run on libabd (HIP)."""

    NAME = "smalllstm"
    PARAM_ORDER, RUNNING_ORDER, ARGS, ENGINE = PARAM_ORDER, RUNNING_ORDER, L.SmallLstmArgs, _Engine
    BACKWARD_ORDER = ("smalllstm backward must directly follow its train-mode forward (activations live in the "
                      "shared workspace, and backward consumes them)")
    BACKWARD_CONSUMES = True   # the saved gates hold the gate gradients afterwards
    STATE = _flat.DROPOUT_STATE

    def __init__(self, num_classes, rnn_features):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels=1, out_channels=64, kernel_size=(2, 2))
        self.bn1 = nn.BatchNorm2d(num_features=64)
        self.pool1 = nn.MaxPool2d(kernel_size=(1, 3))
        self.conv2 = nn.Conv2d(in_channels=64, out_channels=64, kernel_size=(2, 2))
        self.bn2 = nn.BatchNorm2d(num_features=64)
        self.pool2 = nn.MaxPool2d(kernel_size=(2, 2), padding=(1, 1))
        self.conv3 = nn.Conv2d(in_channels=64, out_channels=32, kernel_size=(2, 2))
        self.bn3 = nn.BatchNorm2d(num_features=32)
        self.pool3 = nn.MaxPool2d(kernel_size=(2, 2), padding=(0, 1))
        self.drop1 = nn.Dropout(DROP_P)
        self.flat = nn.Flatten()
        self.rnn = nn.LSTM(rnn_features, HIDDEN, LAYERS, batch_first=True, bidirectional=False)
        self.fc1 = nn.Linear(in_features=FC1_IN, out_features=HIDDEN)
        self.drop2 = nn.Dropout(0.5)
        self.fc2 = nn.Linear(in_features=HIDDEN, out_features=num_classes)
        self.softmax = nn.Softmax()
        self._init_abd()

    # ------------------------------------------------------------------ binding
    def engine(self, x: torch.Tensor) -> _Engine:
        """Bind (or re-bind) the parameters and running statistics to flat device buffers for x's geometry."""
        H, W = int(x.shape[-2]), int(x.shape[-1])
        want = rnn_features(H, W)
        if want != self.rnn.input_size:
            raise ValueError(f"input ({H}, {W}) gives the LSTM {want} features but the model was built for "
                             f"rnn_features {self.rnn.input_size}")
        return self._bind_dropout(H, W, x.device)

    def mask_shape(self, x):
        """(B, 32, T, Wf): drop1's input in the reference, the shape of a keep mask."""
        B, H, W = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
        H3 = (H - 2) // 2 + 1 - 1
        return B, 32, (H3 - 2) // 2 + 1, rnn_features(H, W) // 32

    # ------------------------------------------------------------------ launches
    def hip_forward(self, x, train: bool, seed: int | None = None, mask=None, mask_out=None):
        """The log-probabilities.  train: batch statistics (the running ones and num_batches_tracked advance),
        dropout on, every map kept in the engine's workspace for hip_backward; mask: a (B, 32, T, Wf) uint8 keep
        mask in place of the hash."""
        x = x.contiguous()
        eng = self.engine(x)
        B = x.shape[0]
        if not train:
            from . import ops  # noqa: F401  (registers torch.ops.abd)
            return torch.ops.abd.smalllstm_eval(x, eng.params, eng.running, eng.K)
        out = torch.empty((B, eng.K), dtype=torch.float32, device=x.device)
        ws = eng.workspace(B)
        a = self._args(eng, x, B)
        a.logits_out = out.data_ptr()
        dropout_step(self, a, x.device, seed, mask, mask_out)
        eng.call("forward", C.byref(a), 1, ws.data_ptr(), ws.numel(), L.stream_ptr(x.device))
        eng.token += 1
        eng.last_train_token = eng.token
        return out

    def hip_train_forward(self, x):
        return self.hip_forward(x, train=True)


# ------------------------------------------------------------------ adoption of a reference-built instance
_ADOPTED: "weakref.WeakKeyDictionary[nn.Module, smalllstm]" = weakref.WeakKeyDictionary()


def _refuse(why: str):
    raise L.AbdError(f"not the reference's smalllstm: {why}")


def _check_structure(m: nn.Module):
    for cv, bn, cin, cout in CONVS:
        c = getattr(m, cv, None)
        if not isinstance(c, nn.Conv2d):
            _refuse(f"{cv} is missing or no Conv2d")
        if ((c.in_channels, c.out_channels) != (cin, cout) or _flat.pair(c.kernel_size) != (2, 2)
                or _flat.pair(c.stride) != (1, 1) or c.padding not in (0, (0, 0)) or _flat.pair(c.dilation) != (1, 1)
                or c.groups != 1 or c.bias is None or c.padding_mode != "zeros"):
            _refuse(f"{cv} is not Conv2d({cin}, {cout}, (2, 2), bias, no padding)")
        b = getattr(m, bn, None)
        if not isinstance(b, nn.BatchNorm2d):
            _refuse(f"{bn} is missing or no BatchNorm2d")
        if (b.num_features != cout or b.eps != 1e-5 or b.momentum != 0.1 or not b.affine
                or not b.track_running_stats):
            _refuse(f"{bn} is not BatchNorm2d({cout}) with eps 1e-5, momentum 0.1, affine, running statistics")
    for name, k, pad in POOLS:
        p = getattr(m, name, None)
        if not isinstance(p, nn.MaxPool2d):
            _refuse(f"{name} is missing or no MaxPool2d")
        stride = p.stride if p.stride is not None else p.kernel_size
        if (_flat.pair(p.kernel_size) != k or _flat.pair(stride) != k or _flat.pair(p.padding) != pad
                or _flat.pair(p.dilation) != (1, 1) or p.ceil_mode or p.return_indices):
            _refuse(f"{name} is not MaxPool2d({k}, padding {pad})")
    d = getattr(m, "drop1", None)
    if not isinstance(d, nn.Dropout) or d.p != DROP_P:
        _refuse("drop1 is missing or no Dropout(0.4)")
    r = getattr(m, "rnn", None)
    if not isinstance(r, nn.LSTM):
        _refuse("rnn is missing or no LSTM")
    if (r.hidden_size != HIDDEN or r.num_layers != LAYERS or r.bidirectional or not r.bias or not r.batch_first
            or r.dropout != 0 or r.proj_size != 0):
        _refuse("rnn is not LSTM(rnn_features, 128, 2, batch_first=True), unidirectional, with biases, dropout 0, "
                "proj_size 0")
    if r.input_size % 32 or r.input_size < 32:
        _refuse(f"rnn_features {r.input_size} is no multiple of conv3's 32 channels")
    for name, fin, fout in (("fc1", FC1_IN, HIDDEN), ("fc2", HIDDEN, None)):
        f = getattr(m, name, None)
        if not isinstance(f, nn.Linear) or f.bias is None:
            _refuse(f"{name} is missing or no Linear with bias")
        if f.in_features != fin or (fout is not None and f.out_features != fout):
            _refuse(f"{name} is not Linear({fin}, {fout if fout is not None else 'classes'})")
    if [n for n, _ in m.named_parameters()] != list(PARAM_ORDER):
        _refuse("it has other parameters than conv1..conv3, bn1..bn3, rnn, fc1 and fc2")
    if [n for n, _ in m.named_buffers()] != list(BUFFER_ORDER):
        _refuse("it has other buffers than the three BatchNorms' running statistics")
    if any(p.dtype != torch.float32 for p in m.parameters()) or any(
            b.dtype != (torch.int64 if n.endswith("num_batches_tracked") else torch.float32)
            for n, b in m.named_buffers()):
        _refuse("its parameters or running statistics are not float32")


def adopt(module: nn.Module) -> smalllstm:
    """The abd ``smalllstm`` that runs a reference-built ``utils.models.smalllstm`` instance on libabd.

    The structure is checked (type name ``smalllstm``; every conv, BatchNorm, pool, drop1, the LSTM, fc1 and fc2
    with exactly the reference's shapes and hyper-parameters, the parameter and buffer names, float32), anything
    else raises AbdError.  The result's submodules ARE the instance's own, so the ``Parameter`` objects the script's
    optimizer holds and the BatchNorm buffers are the ones re-homed into the flat buffers (the LSTM's cached weight
    list refers to them too): after training the script's object sees the trained weights and running statistics
    and its own ``forward`` still works.  One adoption per instance (a weak cache; the instance itself is not
    touched)."""
    if isinstance(module, smalllstm):
        return module
    if not adoptable(module):
        _refuse(f"got {type(module).__name__}")
    optional = ("flat", "drop2", "softmax")   # submodules the reference's forward never calls
    fill = {"flat": nn.Flatten, "drop2": lambda: nn.Dropout(0.5), "softmax": nn.Softmax}
    return _flat.adopt_into(
        smalllstm, module, CHILDREN, _ADOPTED, _check_structure,
        lambda got, m: all(getattr(got, n) is getattr(m, n, None) for n in CHILDREN if n not in optional),
        fill=lambda name: fill[name]())


def adoptable(module) -> bool:
    """A module ``adopt`` would look at: named smalllstm, but not this package's class."""
    return _flat.adoptable(module, smalllstm)
