"""A module's parameters as one flat float32 array in state_dict order: the views into it and the loader every language net
shares (lang_codec, lang_query, lang_encoder, lang_single_stage; hr_net packs its weights itself and uses the unwrapping and
the key check), and FlatNet / BatchNormEncoder, the classes that hold such an array on a GPU.

table: ((state_dict name, shape), ...) of _abi; who: the module's name at the head of every message.
"""
from collections import OrderedDict

import torch

from . import _abi
from ._host import Outputs, require_gpu_device

CHECKPOINT_PREFIX = "model."   # AutoencoderLight / LangSupervisedNet keep the torch module as self.model


def _numel(shape):
    n = 1
    for s_ in shape:
        n *= s_
    return n


def views(flat, table, who, what):
    """name -> view of `flat` in the module's shape, in table order.  what: the array's name in the message."""
    total = sum(_numel(shape) for _, shape in table)
    if flat.dim() != 1 or flat.numel() != total:
        raise RuntimeError(f"{who}: the {what} has {total} elements, got {tuple(flat.shape)}")
    out, off = OrderedDict(), 0
    for name, shape in table:
        n = _numel(shape)
        out[name] = flat[off:off + n].view(shape)
        off += n
    return out


def unwrap(state, who, prefix=CHECKPOINT_PREFIX, keep=""):
    """A Lightning checkpoint ({"state_dict": {...}}), its state_dict or a plain state dict -> the entries under `prefix`
    (if any key carries it) whose names start with `keep`, without num_batches_tracked."""
    if not isinstance(state, dict):
        raise RuntimeError(f"{who}: a checkpoint or state dict is expected, got {type(state).__name__}")
    if "state_dict" in state and isinstance(state["state_dict"], dict):
        state = state["state_dict"]
    if any(k.startswith(prefix) for k in state):
        state = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
    return {k: v for k, v in state.items() if k.startswith(keep) and not k.endswith("num_batches_tracked")}


def check_keys(state, table, who, what):
    want = dict(table)
    missing, extra = sorted(set(want) - set(state)), sorted(set(state) - set(want))
    if missing or extra:
        raise RuntimeError(f"{who}: {what} with missing keys {missing}, unexpected keys {extra}")
    return want


def load(flat, state, table, who, what, hint, prefix=None, keep=""):
    """Copies `state` into `flat`; keys and shapes must be the table's.  what: (the array's name, the state's name) in the
    messages; hint: why a shape is fixed.  prefix: unwrap a checkpoint first and keep the names that start with `keep`."""
    if prefix is not None:
        state = unwrap(state, who, prefix, keep)
    for k, shape in check_keys(state, table, who, what[1]).items():
        if tuple(state[k].shape) != tuple(shape):
            raise RuntimeError(f"{who}: {k} has shape {tuple(state[k].shape)}, expected {tuple(shape)} ({hint})")
    for k, v in views(flat, table, who, what[0]).items():
        v.copy_(state[k].detach().to(device=flat.device, dtype=flat.dtype))


class FlatNet:
    """A net as one flat float32 array `flat` on `device`, in the state_dict order of TABLE.  The subclass sets the class
    attributes (the arguments of views and load above) and adds its launches."""

    TABLE = WHO = WHAT = HINT = None
    PREFIX, KEEP = None, ""   # PREFIX None: load_state_dict takes a plain state dict only

    def __init__(self, device, state=None):
        self.device = require_gpu_device(device, type(self).__name__)
        self.flat = torch.zeros(sum(_numel(shape) for _, shape in self.TABLE), dtype=torch.float32, device=self.device)
        if state is not None:
            self.load_state_dict(state)

    @classmethod
    def views_of(cls, flat):
        return views(flat, cls.TABLE, cls.WHO, cls.WHAT[0])

    @classmethod
    def load_into(cls, flat, state):
        load(flat, state, cls.TABLE, cls.WHO, cls.WHAT, cls.HINT, cls.PREFIX, cls.KEEP)

    @property
    def views(self):
        """name -> view of `flat` in the module's shape."""
        return self.views_of(self.flat)

    def load_state_dict(self, state):
        self.load_into(self.flat, state)

    def state_dict(self):
        """Keys and shapes of the module's state_dict(), without num_batches_tracked; clones."""
        return OrderedDict((k, v.clone()) for k, v in self.views.items())


BN_EPS = 1e-5   # nn.BatchNorm1d's default, what the reference's module carries


class BatchNormEncoder(FlatNet):
    """An AutoencoderMLP.encoder of widths WIDTHS with its BatchNorm running statistics; PARAMS: its parameter struct."""

    WHAT = ("flat encoder array", "encoder state")
    PREFIX, KEEP = CHECKPOINT_PREFIX, "encoder."
    WIDTHS = PARAMS = None

    def __init__(self, device, state=None, eps: float = BN_EPS):
        super().__init__(device)
        self.eps = float(eps)
        self._out = Outputs(self.device)
        if state is not None:
            self.load_state_dict(state, eps)

    def load_state_dict(self, state, eps: float = BN_EPS):
        """eps: the BatchNorm1d layers' eps (a module attribute, not part of a state dict)."""
        if not float(eps) > 0.0:
            raise RuntimeError(f"{self.WHO}: eps must be positive, got {eps!r}")
        super().load_state_dict(state)
        self.eps = float(eps)

    def _params(self, in_layout, code_layout, plane_stride):
        return _abi.set_widths(self.PARAMS(in_layout=in_layout, code_layout=code_layout, plane_stride=plane_stride,
                                           bn_eps=self.eps), self.WIDTHS)
