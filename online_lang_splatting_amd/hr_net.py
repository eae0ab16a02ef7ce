"""Host side of olsr_hr_net_forward (include/olsr.h): the high-resolution language feature net between the CLIP backbone and
the general encoder.

Mirrors hr_model(clip_vis_dense, res3, res2) of utils/slam_backend.py:547-555, HighResLanguageFeatureNet in eval()
(language/supervisedNet.py:6-109), forward only: thirteen launches of one fused convolution kernel, no resized or concatenated
copy, BatchNorm / ReLU / sigmoid gate in the producing launch's epilogue.  GPU only; there is no torch fallback.
"""
import ctypes as C
from collections import OrderedDict

import torch

from . import _abi, _flat_state
from ._host import Outputs, planes, require_gpu_device, stream_ptr
from ._lib import check, lib

N_PACKED = _abi.HR_NET_PARAMS
C_FV, C_F3, C_F2, C_OUT = _abi.HR_NET_CHANNELS
BN_EPS = 1e-5   # nn.BatchNorm2d's default, what the reference's module carries


def packed_views(flat):
    """name -> view of the packed [19890816] array, in packed shapes: a conv weight as [taps, out, in], a BatchNorm's four
    vectors one after the other.  Keys are the module's state_dict names."""
    if flat.dim() != 1 or flat.numel() != N_PACKED:
        raise RuntimeError(f"hr_net: the packed array has {N_PACKED} elements, got {tuple(flat.shape)}")
    out, off = OrderedDict(), 0
    for path, kind, o, i, bn in _abi.HR_NET_LAYERS:
        taps = _abi.HR_NET_TAPS[kind]
        out[f"{path}.weight"] = flat[off:off + taps * o * i].view(taps, o, i)
        off += taps * o * i
        out[f"{path}.bias"] = flat[off:off + o]
        off += o
        if bn:
            for n in _abi.HR_NET_BN_FIELDS:
                out[f"{bn}.{n}"] = flat[off:off + o]
                off += o
    assert off == N_PACKED
    return out


def _kinds():
    return {f"{path}.weight": kind for path, kind, _, _, _ in _abi.HR_NET_LAYERS}


def _pack_weight(kind, w):
    """Conv2d [out,in,k,k] -> [k k, out, in]; ConvTranspose2d [in,out,4,4] -> [16, out, in]: a tap's slab is contiguous."""
    k = w.shape[2] * w.shape[3]
    if kind == "convT":
        return w.permute(2, 3, 1, 0).reshape(k, w.shape[1], w.shape[0])
    return w.permute(2, 3, 0, 1).reshape(k, w.shape[0], w.shape[1])


def _unpack_weight(kind, p):
    taps, o, i = p.shape
    k = {1: 1, 9: 3, 16: 4}[taps]
    if kind == "convT":
        return p.view(k, k, o, i).permute(3, 2, 0, 1).contiguous()
    return p.view(k, k, o, i).permute(2, 3, 0, 1).contiguous()


def load_hr_state(flat, state):
    """Packs a HighResLanguageFeatureNet into `flat`.  `state` is a Lightning checkpoint of LangSupervisedNet
    ({"state_dict": {"model.initial_conv.0.weight": ...}}), its state_dict, or a plain module state dict; num_batches_tracked
    is ignored, every other name and shape must be the module's."""
    state = _flat_state.unwrap(state, "hr_net")
    # (the shape check stays here: this one also names a value that is no tensor)
    for k, shape in _flat_state.check_keys(state, _abi.HR_NET_STATE, "hr_net", "state").items():
        if not isinstance(state[k], torch.Tensor) or tuple(state[k].shape) != tuple(shape):
            got = tuple(state[k].shape) if isinstance(state[k], torch.Tensor) else type(state[k]).__name__
            raise RuntimeError(f"hr_net: {k} has shape {got}, expected {tuple(shape)} (the channel widths are compiled into "
                               f"the kernels)")
    kinds = _kinds()
    for k, v in packed_views(flat).items():
        src = state[k].detach().to(device=flat.device, dtype=flat.dtype)
        v.copy_(_pack_weight(kinds[k], src) if k in kinds else src)


def unpack_hr_state(flat):
    """The module's state dict (without num_batches_tracked) out of the packed array: new tensors in the module's shapes."""
    kinds = _kinds()
    views = packed_views(flat)
    return OrderedDict((k, _unpack_weight(kinds[k], views[k]) if k in kinds else views[k].clone()) for k, _ in _abi.HR_NET_STATE)


class HighResLanguageNet:
    """HighResLanguageFeatureNet with its BatchNorm running statistics as one packed float32 array on `device`."""

    def __init__(self, device, state=None, eps: float = BN_EPS):
        self.device = require_gpu_device(device, "HighResLanguageNet")
        if not float(eps) > 0.0:
            raise RuntimeError(f"hr_net: eps must be positive, got {eps!r}")
        self.flat = torch.zeros(N_PACKED, dtype=torch.float32, device=self.device)
        self.eps = float(eps)
        self._work = {}
        self._out = Outputs(self.device)
        if state is not None:
            self.load_state_dict(state)

    def load_state_dict(self, state):
        load_hr_state(self.flat, state)

    def state_dict(self):
        return unpack_hr_state(self.flat)

    # ---- calls ---------------------------------------------------------------------------------------------------------
    def workspace(self, h, w, h3, w3, h2, w2):
        key = (h, w)
        t = self._work.get(key)
        if t is None:
            n = int(lib().olsr_hr_net_workspace_bytes(h, w, h3, w3, h2, w2))
            if n == 0:
                raise RuntimeError("hr_net: bad sizes")
            t = self._work[key] = torch.empty(n, dtype=torch.uint8, device=self.device)
        return t

    def forward(self, fv, f3, f2, out=None, launches: int = 0):
        """fv [1,768,h,w], f3 [1,384,h3,w3], f2 [1,192,h2,w2] (or without the batch dimension; B > 1 runs item by item)
        -> [B,768,8h,8w].  Without `out` the result is a reusable buffer: the next call of the same size overwrites it."""
        B, h, w, sv, pv = planes("hr_net.forward: ", "fv", fv, C_FV, self.device)
        B3, h3, w3, s3, p3 = planes("hr_net.forward: ", "f3", f3, C_F3, self.device)
        B2, h2, w2, s2, p2 = planes("hr_net.forward: ", "f2", f2, C_F2, self.device)
        if not B == B3 == B2:
            raise RuntimeError(f"hr_net.forward: batch sizes differ ({B}, {B3}, {B2})")
        shape = (B, C_OUT, 8 * h, 8 * w)
        if out is None:
            out = self._out.get(shape, shape)
        else:
            self._out.check_out(f"hr_net.forward: out must be a float32 {list(shape)} tensor", out, shape, contiguous=False)
            if (out.stride(3) != 1 and 8 * w > 1) or out.stride(2) != 8 * w or out.stride(1) < 64 * h * w:
                raise RuntimeError(f"hr_net.forward: every channel plane of out must be contiguous and the planes must not "
                                   f"overlap (strides {tuple(out.stride())})")
        work = self.workspace(h, w, h3, w3, h2, w2)
        p = _abi.OlsrHrNetParams(h=h, w=w, h3=h3, w3=w3, h2=h2, w2=w2, c_fv=C_FV, c_f3=C_F3, c_f2=C_F2, c_out=C_OUT,
                                 launches=int(launches), fv_stride=sv, f3_stride=s3, f2_stride=s2, out_stride=int(out.stride(1)),
                                 bn_eps=self.eps, workspace_bytes=work.numel())
        stream = stream_ptr(self.device)
        with torch.cuda.device(self.device):
            for b in range(B):
                check(lib().olsr_hr_net_forward(C.byref(p), pv[b], p3[b], p2[b], self.flat.data_ptr(), work.data_ptr(),
                                                out[b].data_ptr(), stream))
        return out

    __call__ = forward
