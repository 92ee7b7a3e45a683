"""``ResNet`` on the HIP device (drop-in for reference utils/models.py:261-332).

Same submodules, names and constructor order as the reference's ``ResNet(ResidualBlock, [2, 2, 2], num_classes,
linear_features)``, so construction consumes torch's RNG alike (equal initial weights under a seed) and
``state_dict()`` keys / shapes are the reference's, running buffers included.  ``forward`` runs libabd
(csrc/resnet.hip): the stem as a direct kernel, the fourteen residual 3x3 convs (stride 1 and 2) as implicit GEMMs
on the fp32 matrix pipe, train-mode BatchNorm with fixed-order double sums, the 1x1 conv, the average pool and fc;
it returns raw logits like the reference.

The 49 parameters are re-homed into ONE flat device buffer in ``named_parameters()`` order, the fifteen BatchNorms'
running statistics into a 1120-float buffer.  fp32 only: there is no bf16 mode for this model.

Two ways in: build this class (``from abd_amd.models_resnet import ResNet, ResidualBlock``), or hand a
reference-built ``utils.models.ResNet`` to ``training.train`` / ``test`` / ``clean_train`` / ``clean_test``, which
``adopt`` it.
"""
from __future__ import annotations

import ctypes as C
import weakref

import torch
import torch.nn as nn

from . import _flat, _lib as L

# the fifteen conv + BatchNorm units in named_parameters() order: (conv, bn, Cin, Cout, stride)
UNITS = (
    ("conv", "bn", 1, 16, 1),
    ("layer1.0.conv1", "layer1.0.bn1", 16, 16, 1), ("layer1.0.conv2", "layer1.0.bn2", 16, 16, 1),
    ("layer1.1.conv1", "layer1.1.bn1", 16, 16, 1), ("layer1.1.conv2", "layer1.1.bn2", 16, 16, 1),
    ("layer2.0.conv1", "layer2.0.bn1", 16, 32, 2), ("layer2.0.conv2", "layer2.0.bn2", 32, 32, 1),
    ("layer2.0.downsample.0", "layer2.0.downsample.1", 16, 32, 2),
    ("layer2.1.conv1", "layer2.1.bn1", 32, 32, 1), ("layer2.1.conv2", "layer2.1.bn2", 32, 32, 1),
    ("layer3.0.conv1", "layer3.0.bn1", 32, 64, 2), ("layer3.0.conv2", "layer3.0.bn2", 64, 64, 1),
    ("layer3.0.downsample.0", "layer3.0.downsample.1", 32, 64, 2),
    ("layer3.1.conv1", "layer3.1.bn1", 64, 64, 1), ("layer3.1.conv2", "layer3.1.bn2", 64, 64, 1),
)
# residual blocks: (name, the unit whose output it reads, conv1 unit, conv2 unit, downsample unit or -1)
BLOCKS = (("layer1.0", 0, 1, 2, -1), ("layer1.1", 2, 3, 4, -1), ("layer2.0", 4, 5, 6, 7), ("layer2.1", 6, 8, 9, -1),
          ("layer3.0", 9, 10, 11, 12), ("layer3.1", 11, 13, 14, -1))
PARAM_ORDER = tuple(n for cv, bn, *_ in UNITS for n in (f"{cv}.weight", f"{bn}.weight", f"{bn}.bias")) + (
    "conv2d.weight", "conv2d.bias", "fc.weight", "fc.bias")
RUNNING_ORDER = tuple((bn, cout) for _, bn, _, cout, _ in UNITS)
N_PARAMS = len(PARAM_ORDER)
N_RUNNING = 2 * sum(c for _, c in RUNNING_ORDER)
BUFFER_ORDER = tuple(f"{bn}.{b}" for bn, _ in RUNNING_ORDER for b in ("running_mean", "running_var",
                                                                      "num_batches_tracked"))
CHILDREN = ("conv", "bn", "relu", "layer1", "layer2", "layer3", "conv2d", "avg_pool", "fc")
TILE_INFO = {"tile_rows": 0, "k_step": 1, "slice_rows": 2, "max_slices": 3, "stat_rows": 4, "stat_blocks": 5}
MIN_H, MIN_W = 25, 13


def tile_info(what: str) -> int:
    """Geometry of the built kernels (abd_resnet_tile_info): 'tile_rows' rows of a GEMM block tile, 'k_step',
    'slice_rows' least pixels of a weight-gradient slice, 'max_slices', 'stat_rows' least pixels of a BatchNorm
    partial block, 'stat_blocks' most such blocks."""
    return int(L.lib().abd_resnet_tile_info(TILE_INFO[what]))


def linear_features(H: int, W: int) -> int:
    """fc's inputs for an (H, W) input (abd_resnet_linear_features); -1 below 25 x 13."""
    return int(L.lib().abd_resnet_linear_features(int(H), int(W)))


def net_handle(H: int, W: int, K: int):
    return _flat.net_handle("abd_resnet", H, W, K)


def conv3x3(in_channels, out_channels, stride=1):
    return nn.Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=False)


class ResidualBlock(nn.Module):
    """The reference's block (utils/models.py:266-288).  Inside an abd ``ResNet`` it is a container: the model's
    forward runs libabd and never calls this one, which is kept for a block used on its own."""

    def __init__(self, in_channels, out_channels, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv3x3(in_channels, out_channels, stride)
        self.bn1 = nn.BatchNorm2d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3(out_channels, out_channels)
        self.bn2 = nn.BatchNorm2d(out_channels)
        self.downsample = downsample

    def forward(self, x):
        residual = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample:
            residual = self.downsample(x)
        out += residual
        return self.relu(out)


class _Engine(_flat.FlatEngine):
    """The 49 parameters, the 1120 running statistics and the fifteen num_batches_tracked counters.  T, F of the
    shared engine are the input's H, W."""

    def __init__(self, model: "ResNet", H: int, W: int, device: torch.device):
        super().__init__("abd_resnet", N_PARAMS, H, W, model.fc.out_features, device, running=N_RUNNING,
                         nbt=len(RUNNING_ORDER))


class ResNet(_flat.FlatModule, nn.Module):
    """Reference-compatible ResNet(ResidualBlock, [2, 2, 2], ...) whose forward/backward run on libabd (HIP)."""

    NAME = "ResNet"
    PARAM_ORDER, RUNNING_ORDER, ARGS, ENGINE = PARAM_ORDER, RUNNING_ORDER, L.ResNetArgs, _Engine
    BACKWARD_ORDER = ("ResNet backward must directly follow its train-mode forward (activations live in the shared "
                      "workspace)")

    def __init__(self, block, layers, num_classes, linear_features):
        super().__init__()
        if block is not ResidualBlock or list(layers) != [2, 2, 2]:
            raise L.AbdError("abd_amd runs ResNet(ResidualBlock, [2, 2, 2], ...) only, the one every attack script "
                             f"builds; got block {getattr(block, '__name__', block)!r}, layers {list(layers)!r}")
        self.in_channels = 16
        self.conv = conv3x3(1, 16)
        self.bn = nn.BatchNorm2d(16)
        self.relu = nn.ReLU(inplace=True)
        self.layer1 = self.make_layer(block, 16, layers[0])
        self.layer2 = self.make_layer(block, 32, layers[1], 2)
        self.layer3 = self.make_layer(block, 64, layers[2], 2)
        self.conv2d = nn.Conv2d(in_channels=64, out_channels=64, kernel_size=(1, 1), stride=(2, 1))
        self.avg_pool = nn.AvgPool2d(4)
        self.fc = nn.Linear(linear_features, num_classes)
        self._init_abd()

    def make_layer(self, block, out_channels, blocks, stride=1):
        downsample = None
        if (stride != 1) or (self.in_channels != out_channels):
            downsample = nn.Sequential(conv3x3(self.in_channels, out_channels, stride=stride),
                                       nn.BatchNorm2d(out_channels))
        layers = [block(self.in_channels, out_channels, stride, downsample)]
        self.in_channels = out_channels
        for _ in range(1, blocks):
            layers.append(block(out_channels, out_channels))
        return nn.Sequential(*layers)

    # ------------------------------------------------------------------ binding
    def engine(self, x: torch.Tensor) -> _Engine:
        """Bind (or re-bind) the parameters and running statistics to flat device buffers for x's geometry."""
        H, W = int(x.shape[-2]), int(x.shape[-1])
        want = linear_features(H, W)
        if want != self.fc.in_features:
            raise ValueError(f"input ({H}, {W}) gives fc {want} features but the model was built for "
                             f"linear_features {self.fc.in_features}")
        return self._bind(H, W, x.device)

    # ------------------------------------------------------------------ launches
    def hip_forward(self, x, train: bool):
        """The logits.  train: batch statistics (the running ones and num_batches_tracked advance), every map kept
        in the engine's workspace for hip_backward."""
        x = x.contiguous()
        eng = self.engine(x)
        B = x.shape[0]
        if not train:
            from . import ops  # noqa: F401  (registers torch.ops.abd)
            return torch.ops.abd.resnet_eval(x, eng.params, eng.running, eng.K)
        out = torch.empty((B, eng.K), dtype=torch.float32, device=x.device)
        ws = eng.workspace(B)
        a = self._args(eng, x, B)
        a.logits_out = out.data_ptr()
        eng.call("forward", C.byref(a), 1, ws.data_ptr(), ws.numel(), L.stream_ptr(x.device))
        eng.token += 1
        eng.last_train_token = eng.token
        return out

    def hip_train_forward(self, x):
        return self.hip_forward(x, train=True)


# ------------------------------------------------------------------ adoption of a reference-built instance
_ADOPTED: "weakref.WeakKeyDictionary[nn.Module, ResNet]" = weakref.WeakKeyDictionary()


_LEAVES = tuple(n for cv, bn, *_ in UNITS for n in (cv, bn))


def _refuse(why: str):
    raise L.AbdError(f"not the reference's ResNet(ResidualBlock, [2, 2, 2], ...): {why}")


def _check_structure(m: nn.Module):
    for name in ("layer1", "layer2", "layer3"):
        layer = getattr(m, name, None)
        if not isinstance(layer, nn.Sequential) or len(layer) != 2:
            _refuse(f"{name} is missing or no Sequential of two blocks")
    for cv, bn, cin, cout, stride in UNITS:
        _flat.check_conv3x3(m, cv, cin, cout, stride, False, _refuse)
        b = _flat.sub(m, bn)
        if not isinstance(b, nn.BatchNorm2d):
            _refuse(f"{bn} is missing or no BatchNorm2d")
        if (b.num_features != cout or b.eps != 1e-5 or b.momentum != 0.1 or not b.affine
                or not b.track_running_stats):
            _refuse(f"{bn} is not BatchNorm2d({cout}) with eps 1e-5, momentum 0.1, affine, running statistics")
    for name, _, _, _, ud in BLOCKS:
        blk = _flat.sub(m, name)
        ds = getattr(blk, "downsample", None)
        if ud < 0:
            if ds is not None:
                _refuse(f"{name} has a downsample")
        elif not isinstance(ds, nn.Sequential) or len(ds) != 2:
            _refuse(f"{name}.downsample is missing or no Sequential(conv3x3, BatchNorm2d)")
        if not isinstance(getattr(blk, "relu", None), nn.ReLU):
            _refuse(f"{name}.relu is missing or no ReLU")
    if not isinstance(getattr(m, "relu", None), nn.ReLU):
        _refuse("relu is missing or no ReLU")
    c = getattr(m, "conv2d", None)
    if not isinstance(c, nn.Conv2d):
        _refuse("conv2d is missing or no Conv2d")
    if ((c.in_channels, c.out_channels) != (64, 64) or _flat.pair(c.kernel_size) != (1, 1) or _flat.pair(c.stride) != (2, 1)
            or _flat.pair(c.padding) != (0, 0) or _flat.pair(c.dilation) != (1, 1) or c.groups != 1 or c.bias is None):
        _refuse("conv2d is not Conv2d(64, 64, (1, 1), stride (2, 1), bias)")
    p = getattr(m, "avg_pool", None)
    if not isinstance(p, nn.AvgPool2d):
        _refuse("avg_pool is missing or no AvgPool2d")
    stride = p.stride if p.stride is not None else p.kernel_size
    if (_flat.pair(p.kernel_size) != (4, 4) or _flat.pair(stride) != (4, 4) or _flat.pair(p.padding) != (0, 0) or p.ceil_mode
            or not p.count_include_pad or p.divisor_override is not None):
        _refuse("avg_pool is not AvgPool2d(4)")
    f = getattr(m, "fc", None)
    if not isinstance(f, nn.Linear) or f.bias is None:
        _refuse("fc is missing or no Linear with bias")
    if f.in_features % 64 or f.in_features < 64:
        _refuse(f"linear_features {f.in_features} is no multiple of layer3's 64 channels")
    if [n for n, _ in m.named_parameters()] != list(PARAM_ORDER):
        _refuse("it has other parameters than the fifteen conv / BatchNorm pairs, conv2d and fc")
    if [n for n, _ in m.named_buffers()] != list(BUFFER_ORDER):
        _refuse("it has other buffers than the fifteen BatchNorms' running statistics")
    if any(p.dtype != torch.float32 for p in m.parameters()) or any(
            b.dtype != (torch.int64 if n.endswith("num_batches_tracked") else torch.float32)
            for n, b in m.named_buffers()):
        _refuse("its parameters or running statistics are not float32")


def adopt(module: nn.Module) -> ResNet:
    """The abd ``ResNet`` that runs a reference-built ``utils.models.ResNet`` instance on libabd.

    The structure is checked (type name ``ResNet``; every conv, BatchNorm, the downsample Sequentials, conv2d,
    avg_pool and fc with exactly the reference's shapes and hyper-parameters, the parameter and buffer names,
    float32), anything else raises AbdError.  The result's submodules ARE the instance's own, so the ``Parameter``
    objects the script's optimizer holds and the BatchNorm buffers are the ones re-homed into the flat buffers:
    after training the script's object sees the trained weights and running statistics and its own ``forward``
    still works.  One adoption per instance (a weak cache; the instance itself is not touched)."""
    if isinstance(module, ResNet):
        return module
    if not adoptable(module):
        _refuse(f"got {type(module).__name__}")
    new = _flat.adopt_into(
        ResNet, module, CHILDREN, _ADOPTED, _check_structure,
        lambda got, m: all(getattr(got, n) is getattr(m, n, None) for n in CHILDREN) and all(
            leaf is _flat.sub(m, n) for leaf, n in zip(got._leaves, _LEAVES)))
    if not hasattr(new, "_leaves"):   # a fresh adoption; a cached one is returned as it is
        new.in_channels = 64
        # what the cache compares: a layer replaced inside a shared Sequential shows here only
        new._leaves = tuple(_flat.sub(module, n) for n in _LEAVES)
    return new


def adoptable(module) -> bool:
    """A module ``adopt`` would look at: named ResNet, but not this package's class."""
    return _flat.adoptable(module, ResNet)
