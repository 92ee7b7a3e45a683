"""The flat-buffer engine shared by ``models_lstm.lstmwithattention``, ``models_rnn.RNN``, ``models_largecnn.largecnn``,
``models_resnet.ResNet`` and ``models_smalllstm.smalllstm``.

Both models keep their parameters in ONE flat device buffer in ``PARAM_ORDER`` (and their BatchNorm running
statistics, if any, in a second one), drive a family of C entry points that differ only in their prefix
(``abd_lstmattn_*`` / ``abd_rnn_*``), and keep the activations of a train-mode forward in a shared workspace
that the backward of the same step reads.  ``models.smallcnn`` has the same shape but also carries the bf16
modes, data parallelism and the defence hooks; it keeps its own engine.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib as L
from .models import draw_dropout_nonce

# STATE of a model with device dropout: the step counter and the nonce of its mask stream
DROPOUT_STATE = (("_engine", None), ("_step", 0), ("_dropout_nonce", None), ("gemm_precision", "f32"))


def net_handle(prefix: str, T: int, F: int, K: int):
    h = C.c_void_p()
    L.check(getattr(L.lib(), f"{prefix}_create")(int(T), int(F), int(K), C.byref(h)), f"{prefix}_create")
    return h


class FlatEngine:
    """libabd network handle + flat device buffers for one (T, F, K) geometry.  running / nbt: the sizes of
    the BatchNorm running-statistics and num_batches_tracked buffers, 0 for a model without BatchNorm."""

    def __init__(self, prefix: str, n_params: int, T: int, F: int, K: int, device: torch.device, running: int = 0,
                 nbt: int = 0):
        self.prefix, self.n_params = prefix, n_params
        self.T, self.F, self.K = T, F, K
        self.device = device
        self.h = net_handle(prefix, T, F, K)
        offs = (C.c_int64 * (n_params + 1))()
        self.call("param_offsets", offs)
        self.offsets = list(offs)
        self.n = self.offsets[-1]
        self.params = torch.empty(self.n, dtype=torch.float32, device=device)
        self.grads = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.exp_avg = None
        self.exp_avg_sq = None
        self.running = torch.empty(running, dtype=torch.float32, device=device) if running else None
        self.nbt = torch.zeros(nbt, dtype=torch.int64, device=device) if nbt else None
        self._ws = None
        self.token = 0
        self.last_train_token = -1

    def call(self, name: str, *args):
        """abd_<model>_<name>(handle, *args), checked."""
        L.check(getattr(L.lib(), f"{self.prefix}_{name}")(self.h, *args), f"{self.prefix}_{name}")

    def workspace(self, batch):
        """The shared activation workspace, grown on demand (the old one is released first: RNN's is about
        5.9 KB per (row, step), 1.5 GB at B = 256, T = 100)."""
        need = getattr(L.lib(), f"{self.prefix}_workspace_bytes")(self.h, int(batch))
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def views(self, buf):
        return [buf[self.offsets[i]:self.offsets[i + 1]] for i in range(self.n_params)]

    def __del__(self):
        try:
            if self.h and self.h.value:
                getattr(L.lib(), f"{self.prefix}_destroy")(self.h)
        except Exception:
            pass


class FlatModule:
    """Mixin of an nn.Module whose parameters live in a FlatEngine.  The class sets PARAM_ORDER, RUNNING_ORDER
    (((BatchNorm name, channels), ...), empty without BatchNorm), ARGS (the C args struct), ENGINE
    ((model, T, F, device) -> FlatEngine), BACKWARD_ORDER (the message of a backward out of turn) and
    BACKWARD_CONSUMES (backward overwrites what the forward saved, so a token serves once)."""

    RUNNING_ORDER = ()
    BACKWARD_CONSUMES = False
    NAME = "model"    # the display name in messages
    TRANSIENT = ()    # attributes that live for one launch and are not pickled
    STATE = (("_engine", None), ("gemm_precision", "f32"))   # the instance attributes and what they start as

    def _init_abd(self):
        for k, v in self.STATE:
            setattr(self, k, v)

    def __setstate__(self, state):
        # also the target of reference-format checkpoints (training.reference_pickle_object)
        super().__setstate__(state)
        for k, v in self.STATE:
            if k not in self.__dict__:
                self.__dict__[k] = v

    def set_gemm_precision(self, precision: str):
        """fp32 products only ('f32', or 'f32split' which names the same accuracy class): 'bf16' raises
        AbdError."""
        if precision not in L.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(L.PRECISIONS)}, got {precision!r}")
        if precision == "bf16":
            raise L.AbdError(f"{self.NAME} has no bf16 mode: every product is fp32 (DESIGN.md §5)")
        return self

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_engine"] = None
        for k in self.TRANSIENT:
            st.pop(k, None)
        return st

    def _check_input(self, x):
        L.require_device(x, f"{self.NAME} input")
        if x.dim() != 4 or x.shape[1] != 1 or x.dtype != torch.float32:
            raise ValueError(f"{self.NAME} expects (B, 1, H, W) float32")

    def forward(self, x):
        self._check_input(x)
        self.engine(x)
        if self.training and torch.is_grad_enabled():
            return FlatFunction.apply(x, self, *self._param_list())
        return self.hip_forward(x, train=self.training)

    def _param_list(self):
        d = dict(self.named_parameters())
        return [d[n] for n in self.PARAM_ORDER]

    def _running_slots(self, eng):
        """(index, BatchNorm module, its running_mean view, its running_var view) per RUNNING_ORDER entry."""
        o = 0
        for i, (name, c) in enumerate(self.RUNNING_ORDER):
            bn = self.get_submodule(name) if "." in name else getattr(self, name)   # ResNet's nested BatchNorms
            yield i, bn, eng.running[o:o + c], eng.running[o + c:o + 2 * c]
            o += 2 * c

    def _bound(self, eng) -> bool:
        if eng is None:
            return False
        base = eng.params.data_ptr()
        for p, off in zip(self._param_list(), eng.offsets):
            if p.data.data_ptr() != base + 4 * off or p.device != eng.device:
                return False
        for _, bn, mean, var in self._running_slots(eng):
            if bn.running_mean.data_ptr() != mean.data_ptr() or bn.running_var.data_ptr() != var.data_ptr():
                return False
        return True

    def _bind(self, T: int, F: int, device):
        """The engine for this geometry and device: the bound one, or a new one the parameters, the BatchNorm
        buffers and every nn.LSTM child's cached weight list are re-homed into."""
        eng = self._engine
        if eng is not None and (eng.T, eng.F) == (T, F) and eng.device == device and self._bound(eng):
            return eng
        new = self.ENGINE(self, T, F, device)
        with torch.no_grad():
            for p, v in zip(self._param_list(), new.views(new.params)):
                v.copy_(p.data.reshape(-1))
                p.data = v.view(p.shape)
            for i, bn, mean, var in self._running_slots(new):
                mean.copy_(bn.running_mean)
                var.copy_(bn.running_var)
                bn.running_mean, bn.running_var = mean, var
                new.nbt[i].copy_(bn.num_batches_tracked)
                bn.num_batches_tracked = new.nbt[i]
        # nn.LSTM caches a flattened copy of its weights for the vendor RNN kernels; they are views now
        for rnn in self.children():
            if isinstance(rnn, torch.nn.LSTM):
                rnn._flat_weights = [getattr(rnn, n) for n in rnn._flat_weights_names]
        self._engine = new
        return new

    def _bind_dropout(self, T: int, F: int, device):
        """_bind for a model with device dropout: a model that has no nonce yet draws it when the engine was
        re-bound."""
        bound = self._engine
        eng = self._bind(T, F, device)
        if eng is not bound and getattr(self, "_dropout_nonce", None) is None:
            self._dropout_nonce = draw_dropout_nonce(device)
        return eng

    def _args(self, eng, x, B):
        a = self.ARGS()
        a.x = x.data_ptr()
        a.batch = B
        a.params = eng.params.data_ptr()
        a.grads = eng.grads.data_ptr()
        if eng.running is not None:
            a.running = eng.running.data_ptr()
            a.num_batches_tracked = eng.nbt.data_ptr()
        a.grad_scale = 1.0
        return a

    def hip_backward(self, x, dlogits, token):
        eng = self._engine
        if eng is None or token != eng.last_train_token:
            raise L.AbdError(self.BACKWARD_ORDER)
        if self.BACKWARD_CONSUMES:
            eng.last_train_token = -1
        B = x.shape[0]
        ws = eng.workspace(B)
        a = self._args(eng, x, B)
        dl = dlogits.contiguous()
        eng.call("backward", C.byref(a), dl.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr(x.device))
        return eng.views(eng.grads)


class FlatFunction(torch.autograd.Function):
    """model.hip_train_forward(x) with model.hip_backward as its gradient, for either model."""

    @staticmethod
    def forward(ctx, x, model, *params):
        out = model.hip_train_forward(x)
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


# ------------------------------------------------------------------ adoption of a reference-built instance
def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def sub(m: nn.Module, name: str):
    """m's submodule at the dotted path, or None."""
    try:
        return m.get_submodule(name)
    except AttributeError:
        return None


def check_conv3x3(module, name, cin, cout, stride, bias, refuse):
    """module's submodule `name` must be Conv2d(cin, cout, 3, stride, padding 1) with or without a bias, nothing
    else set; refuse(why) raises."""
    c = sub(module, name)
    if not isinstance(c, nn.Conv2d):
        refuse(f"{name} is missing or no Conv2d")
    if ((c.in_channels, c.out_channels) != (cin, cout) or pair(c.kernel_size) != (3, 3)
            or pair(c.stride) != (stride, stride) or c.padding not in (1, (1, 1)) or pair(c.dilation) != (1, 1)
            or c.groups != 1 or (c.bias is not None) != bias or c.padding_mode != "zeros"):
        refuse(f"{name} is not Conv2d({cin}, {cout}, 3, stride {stride}, padding 1, {'bias' if bias else 'no bias'})")


def adoptable(module, cls) -> bool:
    """A module cls's adopt would look at: named like cls, but not cls itself."""
    return isinstance(module, nn.Module) and not isinstance(module, cls) and type(module).__name__ == cls.__name__


def adopt_into(cls, module, children, cache, check, unchanged, fill=None):
    """The common body of the models' adopt(): the cached adoption of `module` while unchanged(got, module) holds;
    else check(module) (which raises on a foreign structure) and a new cls whose `children` ARE module's own
    (fill(name) stands in for one that module lacks), in module's train / eval state, cached weakly."""
    got = cache.get(module)
    if got is not None and unchanged(got, module):
        return got
    check(module)
    new = cls.__new__(cls)
    nn.Module.__init__(new)
    for name in children:
        child = getattr(module, name, None)
        new.add_module(name, child if fill is None or isinstance(child, nn.Module) else fill(name))
    new._init_abd()
    new.train(module.training)
    cache[module] = new
    return new
