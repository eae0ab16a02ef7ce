"""Host side of olsr_lang_encoder_encode (include/olsr.h): the general language encoder 768 -> 512 -> 256 -> 128 -> 64 -> 32
of the reference's back end, which turns a keyframe's CLIP map into the 32-channel rows the online autoencoder trains on.

Mirrors clip_viz_dense.permute(0,2,3,1).view(-1,768) followed by AutoencoderMLP.encode in eval() (utils/slam_backend.py:
556-559 and :392-395, language/autoencoder/model.py:15-56) in one launch: the [1,768,h,w] map is read as it lies, the permuted
copy and the intermediates are never formed.  With a codec the same launch also writes the 15-channel codes of
OnlineLanguageCodec.encode.  GPU only; there is no torch fallback.
"""
import ctypes as C
from typing import Tuple

import torch

from . import _abi
from ._flat_state import BN_EPS, BatchNormEncoder  # noqa: F401  (BN_EPS: part of this module's interface)
from ._host import gpu_float32, planes, stream_ptr
from ._lib import check, lib
from .lang_codec import OnlineLanguageCodec, _layout

N_ENCODER = _abi.LANG_ENCODER_PARAMS
FEATURE_DIM = _abi.LANG_ENCODER_WIDTHS[0]
OUT_DIM = _abi.LANG_ENCODER_WIDTHS[-1]


def feature_items(device, who, t):
    """A feature tensor on `device` -> (layout, N, plane_stride, [data pointer per item]).  No conversion and no copy: what
    cannot be read in place is an error.  (Shared with lang_single_stage.SingleStageEncoder: the input forms are the same.)"""
    t = gpu_float32(f"{who}: features", t, device)
    if t.dim() == 2:
        if t.shape[1] != FEATURE_DIM or t.shape[0] < 1:
            raise RuntimeError(f"{who}: features has shape {tuple(t.shape)}, expected [N,{FEATURE_DIM}] with N >= 1")
        if not t.is_contiguous():
            raise RuntimeError(f"{who}: [N,{FEATURE_DIM}] rows must be contiguous")
        return _abi.LANG_ENCODER_IN_ROWS, int(t.shape[0]), 0, [t.data_ptr()]
    _, h, w, stride, ptrs = planes(f"{who}: ", "features", t, FEATURE_DIM, device, other_forms=f"[N,{FEATURE_DIM}], ",
                                   plane="every channel plane")
    return _abi.LANG_ENCODER_IN_CHANNELS, h * w, stride, ptrs


class LanguageEncoder(BatchNormEncoder):
    """The general encoder (AutoencoderMLP.encoder with its BatchNorm running statistics) as a flat float32 array on `device`."""

    TABLE, WIDTHS, PARAMS = _abi.LANG_ENCODER_STATE, _abi.LANG_ENCODER_WIDTHS, _abi.OlsrLangEncoderParams
    WHO = "lang_encoder"
    HINT = f"the widths {WIDTHS} are compiled into the kernel"

    # ---- calls ---------------------------------------------------------------------------------------------------------
    def _items(self, who, t):
        return feature_items(self.device, who, t)

    def _launch(self, lay, N, plane_stride, ptr, online, feat_ptr, codes_ptr, code_layout):
        p = self._params(lay, code_layout, plane_stride)
        check(lib().olsr_lang_encoder_encode(C.byref(p), N, ptr, self.flat.data_ptr(), online, feat_ptr, codes_ptr,
                                             stream_ptr(self.device)))

    def _out32(self, who, out, rows):
        if out is None:
            return self._out.get("features32", (rows, OUT_DIM))
        return self._out.check_out(f"{who}: out must be a contiguous float32 [{rows},{OUT_DIM}] tensor", out, (rows, OUT_DIM))

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
        codes = self._out.get("codes", shape)
        with torch.cuda.device(self.device):
            for b, ptr in enumerate(ptrs):
                self._launch(lay, N, stride, ptr, codec.flat.data_ptr(), out[b * N:(b + 1) * N].data_ptr(), codes[b].data_ptr(),
                             code_layout)
        return out, (codes[0] if B == 1 else codes)


def encoder_views(flat):
    """name -> view of a flat [572128] tensor in the shapes of AutoencoderMLP.encoder, in state_dict order."""
    return LanguageEncoder.views_of(flat)


def load_encoder_state(flat, state):
    """Copies the encoder of an AutoencoderMLP into a flat [572128] tensor.  `state` is a Lightning checkpoint
    ({"state_dict": {"model.encoder.0.weight": ...}}), its state_dict, or a plain AutoencoderMLP state dict; decoder entries
    and num_batches_tracked are ignored, the encoder's names and shapes must be the module's."""
    LanguageEncoder.load_into(flat, state)
