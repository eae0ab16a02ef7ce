"""The call kit of the host modules: what every entry's caller needs around the call itself — the stream pointer, the NULL
of an absent tensor, the device and tensor checks, scratch and output buffers that are reused, the in-place plane reader.

Plain functions; the only state is the scratch cache.  Messages differ between callers only in what the caller passes.
"""
import ctypes as C

import torch

from ._abi import ptr  # noqa: F401  (defined there: _abi imports no torch and make_scene needs it)


def stream_ptr(device):
    """The current stream of `device` as the entries take it."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu_device(device, who) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: a GPU device is required (there is no torch fallback)")
    return device


_scratch = {}   # (device, kind) -> uint8 tensor, grown on demand and reused


def scratch_for(device, kind, nbytes):
    buf = _scratch.get((device, kind))
    if buf is None or buf.numel() < nbytes:
        buf = _scratch[(device, kind)] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf


def gpu_float32(what, t, device):
    """`t` detached if it is a float32 tensor on `device` (no conversion: a CPU or float64 tensor is an error, not a copy).
    what: the head of the message, e.g. "encode: features"."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be a float32 tensor on the GPU")
    if t.device != device:
        raise RuntimeError(f"{what} is on {t.device}, expected {device}")
    return t.detach()


def planes(prefix, name, t, channels, device, other_forms="", plane=None):
    """A [channels,h,w] or [B,channels,h,w] map on `device`, read as it lies -> (B, h, w, plane stride, [data pointer per
    item]).  No conversion and no copy: what cannot be read in place is an error.  other_forms: forms the caller accepts
    besides, at the head of the shape message's list; plane: the plane message's subject (default: "every channel plane of
    <name>")."""
    t = gpu_float32(f"{prefix}{name}", t, device)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] != channels or min(t.shape[0], t.shape[2], t.shape[3]) < 1:
        raise RuntimeError(f"{prefix}{name} has shape {tuple(t.shape)}, expected {other_forms}[{channels},h,w] or "
                           f"[B,{channels},h,w]")
    B, _, h, w = t.shape
    if (w > 1 and t.stride(3) != 1) or (h > 1 and t.stride(2) != w) or t.stride(1) < h * w:
        raise RuntimeError(f"{prefix}{plane or f'every channel plane of {name}'} must be contiguous and the planes must not "
                           f"overlap (strides {tuple(t.stride())} for shape {tuple(t.shape)})")
    return int(B), int(h), int(w), int(t.stride(1)), [t[b].data_ptr() for b in range(B)]


class Outputs:
    """An object's reusable output buffers on `device`: the next call with the same key and shape overwrites them."""

    def __init__(self, device):
        self.device, self._cache = device, {}

    def get(self, key, shape, dtype=torch.float32):
        t = self._cache.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self._cache[key] = torch.empty(shape, dtype=dtype, device=self.device)
        return t

    def check_out(self, what, out, shape, contiguous=True):
        """The caller's own float32 output tensor.  what: the message up to the device, e.g. "encode: out must be a
        contiguous float32 [4, 15] tensor"."""
        if (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
                or tuple(out.shape) != tuple(shape) or (contiguous and not out.is_contiguous())):
            raise RuntimeError(f"{what} on {self.device}")
        return out
