"""Host side of olsr_lang_encoder_encode (include/olsr.h): the general language encoder 768 -> 512 -> 256 -> 128 -> 64 -> 32
of the reference's back end, which turns a keyframe's CLIP map into the 32-channel rows the online autoencoder trains on.

Mirrors clip_viz_dense.permute(0,2,3,1).view(-1,768) followed by AutoencoderMLP.encode in eval() (utils/slam_backend.py:
556-559 and :392-395, language/autoencoder/model.py:15-56) in one launch: the [1,768,h,w] map is read as it lies, the permuted
copy and the intermediates are never formed.  With a codec the same launch also writes the 15-channel codes of
OnlineLanguageCodec.encode.  GPU only; there is no torch fallback.
"""
import ctypes as C
from collections import OrderedDict
from typing import Tuple

import torch

from . import _abi, _flat_state
from ._lib import check, lib
from .lang_codec import OnlineLanguageCodec, _layout
from ._flat_state import CHECKPOINT_PREFIX

N_ENCODER = _abi.LANG_ENCODER_PARAMS
FEATURE_DIM = _abi.LANG_ENCODER_WIDTHS[0]
OUT_DIM = _abi.LANG_ENCODER_WIDTHS[-1]
BN_EPS = 1e-5   # nn.BatchNorm1d's default, what the reference's module carries


_WHAT = ("flat encoder array", "encoder state")


def encoder_views(flat):
    """name -> view of a flat [572128] tensor in the shapes of AutoencoderMLP.encoder, in state_dict order."""
    return _flat_state.views(flat, _abi.LANG_ENCODER_STATE, "lang_encoder", _WHAT[0])


def load_encoder_state(flat, state):
    """Copies the encoder of an AutoencoderMLP into a flat [572128] tensor.  `state` is a Lightning checkpoint
    ({"state_dict": {"model.encoder.0.weight": ...}}), its state_dict, or a plain AutoencoderMLP state dict; decoder entries
    and num_batches_tracked are ignored, the encoder's names and shapes must be the module's."""
    _flat_state.load(flat, state, _abi.LANG_ENCODER_STATE, "lang_encoder", _WHAT,
                     f"the widths {_abi.LANG_ENCODER_WIDTHS} are compiled into the kernel", CHECKPOINT_PREFIX, "encoder.")


def feature_items(device, who, t):
    """A feature tensor on `device` -> (layout, N, plane_stride, [data pointer per item]).  No conversion and no copy: what
    cannot be read in place is an error.  (Shared with lang_single_stage.SingleStageEncoder: the input forms are the same.)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"{who}: features must be a float32 tensor on the GPU")
    if t.device != device:
        raise RuntimeError(f"{who}: features is on {t.device}, expected {device}")
    t = t.detach()
    if t.dim() == 2:
        if t.shape[1] != FEATURE_DIM or t.shape[0] < 1:
            raise RuntimeError(f"{who}: features has shape {tuple(t.shape)}, expected [N,{FEATURE_DIM}] with N >= 1")
        if not t.is_contiguous():
            raise RuntimeError(f"{who}: [N,{FEATURE_DIM}] rows must be contiguous")
        return _abi.LANG_ENCODER_IN_ROWS, int(t.shape[0]), 0, [t.data_ptr()]
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] != FEATURE_DIM or min(t.shape[0], t.shape[2], t.shape[3]) < 1:
        raise RuntimeError(f"{who}: features has shape {tuple(t.shape)}, expected [N,{FEATURE_DIM}], [{FEATURE_DIM},h,w] or "
                           f"[B,{FEATURE_DIM},h,w]")
    B, _, h, w = t.shape
    if (w > 1 and t.stride(3) != 1) or (h > 1 and t.stride(2) != w) or t.stride(1) < h * w:
        raise RuntimeError(f"{who}: every channel plane must be contiguous and the planes must not overlap "
                           f"(strides {tuple(t.stride())} for shape {tuple(t.shape)})")
    return _abi.LANG_ENCODER_IN_CHANNELS, int(h * w), int(t.stride(1)), [t[b].data_ptr() for b in range(B)]


class LanguageEncoder:
    """The general encoder (AutoencoderMLP.encoder with its BatchNorm running statistics) as a flat float32 array on `device`."""

    def __init__(self, device, state=None, eps: float = BN_EPS):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("LanguageEncoder: a GPU device is required (there is no torch fallback)")
        self.flat = torch.zeros(N_ENCODER, dtype=torch.float32, device=self.device)
        self.eps = float(eps)
        self._out = {}
        if state is not None:
            self.load_state_dict(state, eps)

    @property
    def views(self):
        return encoder_views(self.flat)

    def load_state_dict(self, state, eps: float = BN_EPS):
        """eps: the BatchNorm1d layers' eps (a module attribute, not part of a state dict)."""
        if not float(eps) > 0.0:
            raise RuntimeError(f"lang_encoder: eps must be positive, got {eps!r}")
        load_encoder_state(self.flat, state)
        self.eps = float(eps)

    def state_dict(self):
        return OrderedDict((k, v.clone()) for k, v in self.views.items())

    # ---- calls ---------------------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _items(self, who, t):
        return feature_items(self.device, who, t)

    def _launch(self, lay, N, plane_stride, ptr, online, feat_ptr, codes_ptr, code_layout):
        p = _abi.OlsrLangEncoderParams(n_widths=len(_abi.LANG_ENCODER_WIDTHS), in_layout=lay, code_layout=code_layout,
                                       plane_stride=plane_stride, bn_eps=self.eps)
        for k, v in enumerate(_abi.LANG_ENCODER_WIDTHS):
            p.widths[k] = v
        check(lib().olsr_lang_encoder_encode(C.byref(p), N, ptr, self.flat.data_ptr(), online, feat_ptr, codes_ptr, self._stream()))

    def _out32(self, who, out, rows):
        if out is None:
            t = self._out.get("features32")
            if t is None or t.shape[0] != rows:
                t = self._out["features32"] = torch.empty(rows, OUT_DIM, dtype=torch.float32, device=self.device)
            return t
        if (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
                or tuple(out.shape) != (rows, OUT_DIM) or not out.is_contiguous()):
            raise RuntimeError(f"{who}: out must be a contiguous float32 [{rows},{OUT_DIM}] tensor on {self.device}")
        return out

    def encode(self, features, out=None):
        """features [N,768], [768,h,w], [1,768,h,w] or [B,768,h,w] (one launch per item) -> unit rows [N,32] ([B h w,32]).
        Without `out` the result is a reusable buffer: the next call of the same size overwrites it."""
        lay, N, stride, ptrs = self._items("encode", features)
        out = self._out32("encode", out, N * len(ptrs))
        with torch.cuda.device(self.device):
            for b, ptr in enumerate(ptrs):
                self._launch(lay, N, stride, ptr, None, out[b * N:(b + 1) * N].data_ptr(), None, _abi.LANG_AE_CODES_ROWS)
        return out

    def encode_codes(self, features, codec: OnlineLanguageCodec, layout: str = "channels") -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (features32 [N,32], codes) from one launch: codes = codec.encode(features32, layout) bit for bit, [15,N]
        ("channels") or [N,15] ("rows"); for a batch [B,15,N] or [B,N,15].  Both are reusable buffers."""
        if not isinstance(codec, OnlineLanguageCodec) or codec.device != self.device:
            raise RuntimeError(f"encode_codes: an OnlineLanguageCodec on {self.device} is expected")
        code_layout = _layout(layout)
        lay, N, stride, ptrs = self._items("encode_codes", features)
        B = len(ptrs)
        out = self._out32("encode_codes", None, N * B)
        shape = (B, _abi.LANG_AE_CODE, N) if layout == "channels" else (B, N, _abi.LANG_AE_CODE)
        codes = self._out.get("codes")
        if codes is None or tuple(codes.shape) != shape:
            codes = self._out["codes"] = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            for b, ptr in enumerate(ptrs):
                self._launch(lay, N, stride, ptr, codec.flat.data_ptr(), out[b * N:(b + 1) * N].data_ptr(), codes[b].data_ptr(),
                             code_layout)
        return out, (codes[0] if B == 1 else codes)
