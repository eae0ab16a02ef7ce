"""Host side of olsr_lang_query_sims / olsr_lang_query_relevancy (include/olsr.h): open-vocabulary text queries on a rendered
language map.

Mirrors the reference's evaluation path (eval/evaluate_onlinelangslam.py:266-287 with eval/openclip_encoder.py:44-107 and
the back end's perform_similarity, utils/slam_backend.py:204-218): codes -> EncoderDecoderOnline.decode -> AutoencoderMLP.decode
-> products with the CLIP text embeddings -> relevancy against the canonical negatives -> 30 x 30 smoothing -> localisation
point, mask, label map.  The 768-channel feature image is never formed: stage A keeps a pixel's activations in LDS and
stores its K similarities.  The CLIP text tower is not part of this: the caller supplies unit-norm embedding rows.
GPU only; there is no torch fallback.
"""
import ctypes as C
from collections import OrderedDict
from typing import Optional, Tuple

import torch

from . import _abi
from ._flat_state import CHECKPOINT_PREFIX, FlatNet
from ._host import Outputs, gpu_float32, stream_ptr
from ._lib import check, lib
from .lang_codec import OnlineLanguageCodec

N_DECODER = _abi.LANG_QUERY_DECODER_PARAMS
FEATURE_DIM = _abi.LANG_QUERY_FEATURE_DIM


class LanguageDecoder(FlatNet):
    """The general decoder 32 -> 192 -> 256 -> 384 -> 512 -> 768 (AutoencoderMLP.decoder) as a flat float32 array on `device`."""

    TABLE, WHO, WHAT = _abi.LANG_QUERY_STATE, "lang_query", ("flat decoder array", "decoder state")
    HINT = f"the widths {_abi.LANG_QUERY_WIDTHS} are compiled into the kernels"
    PREFIX, KEEP = CHECKPOINT_PREFIX, "decoder."


def decoder_views(flat):
    """name -> view of a flat [745536] tensor in the shapes of AutoencoderMLP.decoder, in state_dict order."""
    return LanguageDecoder.views_of(flat)


def load_decoder_state(flat, state):
    """Copies the decoder of an AutoencoderMLP into a flat [745536] tensor.  `state` is a Lightning checkpoint
    ({"state_dict": {"model.decoder.0.weight": ...}}, what load_from_checkpoint reads), its state_dict, or a plain
    AutoencoderMLP state dict; encoder and BatchNorm entries are ignored, the decoder's names and shapes must be the module's."""
    LanguageDecoder.load_into(flat, state)


def _embeds(name, t, dev, allow_empty=False):
    t = gpu_float32(name, t, dev)
    if t.dim() != 2 or t.shape[1] != FEATURE_DIM or (t.shape[0] < 1 and not allow_empty):
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected [n,{FEATURE_DIM}] with n >= 1")
    return t


class LanguageQuery:
    """Text queries against code maps [15,h,w] (render(...)["language"]).

    set_phrases / set_labels take unit-norm float32 embedding rows on the device.  similarities() is stage A alone,
    relevancy() both stages.  Outputs are reusable buffers: the next call with the same sizes overwrites them."""

    def __init__(self, decoder: LanguageDecoder, codec: OnlineLanguageCodec):
        if not isinstance(decoder, LanguageDecoder) or not isinstance(codec, OnlineLanguageCodec):
            raise RuntimeError("LanguageQuery: a LanguageDecoder and an OnlineLanguageCodec are expected")
        if decoder.device != codec.device:
            raise RuntimeError(f"LanguageQuery: the decoder is on {decoder.device}, the codec on {codec.device}")
        self.decoder, self.codec, self.device = decoder, codec, decoder.device
        self.thresh = 0.4   # the reference's mask_thresh
        self._pos = self._neg = None
        self._labels = torch.zeros(0, FEATURE_DIM, dtype=torch.float32, device=self.device)
        self._phrases = None
        self._out, self._scratch = Outputs(self.device), None

    # ---- phrases -------------------------------------------------------------------------------------------------------
    def _rebuild(self):
        if self._neg is None:
            return
        pos = self._pos if self._pos is not None else self._labels[:0]
        k = pos.shape[0] + self._labels.shape[0] + self._neg.shape[0]
        if k > _abi.LANG_QUERY_MAX_PHRASES:
            raise RuntimeError(f"lang_query: {k} phrase rows (positives + labels + negatives), at most "
                               f"{_abi.LANG_QUERY_MAX_PHRASES} are supported")
        self._phrases = torch.cat([pos, self._labels, self._neg], dim=0).contiguous()

    def set_phrases(self, pos_embeds, neg_embeds):
        """pos_embeds [P,768], neg_embeds [Q,768] (the reference: "object", "things", "stuff", "texture")."""
        pos, neg = _embeds("set_phrases: pos_embeds", pos_embeds, self.device), _embeds("set_phrases: neg_embeds", neg_embeds, self.device)
        old = (self._pos, self._neg)
        self._pos, self._neg = pos.clone(), neg.clone()
        try:
            self._rebuild()
        except RuntimeError:
            self._pos, self._neg = old
            raise

    def set_labels(self, label_embeds):
        """label_embeds [L,768] for the semantic label map (get_semantic_map); None or an empty tensor switches it off."""
        if label_embeds is None:
            lab = self._labels[:0]
        else:
            lab = _embeds("set_labels: label_embeds", label_embeds, self.device, allow_empty=True)
        old = self._labels
        self._labels = lab.clone()
        try:
            self._rebuild()
        except RuntimeError:
            self._labels = old
            raise

    @property
    def counts(self) -> Tuple[int, int, int]:
        """(positives, labels, negatives)"""
        return (0 if self._pos is None else self._pos.shape[0], self._labels.shape[0], 0 if self._neg is None else self._neg.shape[0])

    # ---- calls ---------------------------------------------------------------------------------------------------------
    def _codes(self, who, codes):
        codes = gpu_float32(f"{who}: codes", codes, self.device)
        if codes.dim() == 2:   # [15,N]: a map of one row
            codes = codes.unsqueeze(1)
        if codes.dim() != 3 or codes.shape[0] != _abi.LANG_AE_CODE or codes.shape[1] < 1 or codes.shape[2] < 1:
            raise RuntimeError(f"{who}: codes has shape {tuple(codes.shape)}, expected [15,h,w] (or [15,N])")
        return codes.contiguous()

    def _params(self, who, codes, decode_hw, out_hw, want_mask=False, want_labels=False):
        if self._phrases is None:
            raise RuntimeError(f"{who}: set_phrases first")
        h, w = int(codes.shape[1]), int(codes.shape[2])
        dh, dw = (h, w) if decode_hw is None else (int(decode_hw[0]), int(decode_hw[1]))
        oh, ow = (h, w) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        if min(dh, dw, oh, ow) < 1:
            raise RuntimeError(f"{who}: decode_hw = {decode_hw} and out_hw = {out_hw} must be positive")
        n_pos, n_lab, _ = self.counts
        p = _abi.OlsrLangQueryParams(K=self._phrases.shape[0], n_pos=n_pos, n_labels=n_lab,
                                     in_width=w, in_height=h, dec_width=dw, dec_height=dh, out_width=ow, out_height=oh,
                                     thresh=float(self.thresh),
                                     flags=(_abi.LANG_QUERY_WANT_MASK if want_mask else 0) | (_abi.LANG_QUERY_WANT_LABELS if want_labels else 0))
        return _abi.set_widths(p, _abi.LANG_QUERY_WIDTHS)

    def _sims(self, p, codes):
        sims = self._out.get("sims", (p.K, p.dec_height, p.dec_width))
        with torch.cuda.device(self.device):
            check(lib().olsr_lang_query_sims(C.byref(p), codes.data_ptr(), self.codec.flat.data_ptr(), self.decoder.flat.data_ptr(),
                                             self._phrases.data_ptr(), sims.data_ptr(), stream_ptr(self.device)))
        return sims

    def similarities(self, codes, decode_hw: Optional[Tuple[int, int]] = None):
        """codes [15,h,w] -> [K,h',w'] = <decode(codes), phrase> for the rows [positives | labels | negatives]; decode_hw
        (h', w') resamples the codes first (F.interpolate bilinear, align_corners=False)."""
        c = self._codes("similarities", codes)
        return self._sims(self._params("similarities", c, decode_hw, decode_hw), c)

    def relevancy(self, codes, out_hw: Optional[Tuple[int, int]] = None, decode_hw: Optional[Tuple[int, int]] = None):
        """codes [15,h,w] -> dict at out_hw (default (h, w)): relevancy, smoothed, blended [P,H,W]; score [P]; coord int32
        [P,2] = (x, y); minmax [P,2]; mask uint8 [P,H,W] (threshold self.thresh); labels int32 [H,W] if set_labels was given rows."""
        c = self._codes("relevancy", codes)
        n_pos, n_lab, _ = self.counts
        if n_pos < 1:
            raise RuntimeError("relevancy: set_phrases with at least one positive first")
        p = self._params("relevancy", c, decode_hw, out_hw, want_mask=True, want_labels=n_lab > 0)
        return self._stage_b(p, self._sims(p, c))

    def localise(self, sims, out_hw: Optional[Tuple[int, int]] = None):
        """Stage B alone: similarities [K,h',w'] (as similarities() returns them, for the phrases now set) -> the dict of
        relevancy() at out_hw (default (h', w'))."""
        n_pos, n_lab, n_neg = self.counts
        if n_pos < 1:
            raise RuntimeError("localise: set_phrases with at least one positive first")
        if not isinstance(sims, torch.Tensor) or not sims.is_cuda or sims.dtype != torch.float32 or sims.device != self.device:
            raise RuntimeError(f"localise: sims must be a float32 tensor on the GPU ({self.device})")
        if sims.dim() != 3 or sims.shape[0] != n_pos + n_lab + n_neg or sims.shape[1] < 1 or sims.shape[2] < 1:
            raise RuntimeError(f"localise: sims has shape {tuple(sims.shape)}, expected [{n_pos + n_lab + n_neg},h,w]")
        s_ = sims.detach().contiguous()
        p = self._params("localise", s_, None, out_hw, want_mask=True, want_labels=n_lab > 0)
        return self._stage_b(p, s_)

    def _stage_b(self, p, sims):
        n_pos, n_lab, _ = self.counts
        H, W = p.out_height, p.out_width
        L = lib()
        nbytes = L.olsr_lang_query_scratch_bytes(C.byref(p))
        scratch = self._scratch
        if scratch is None or scratch.numel() < nbytes:
            scratch = self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        out = OrderedDict(relevancy=self._out.get("relevancy", (n_pos, H, W)), smoothed=self._out.get("smoothed", (n_pos, H, W)),
                          blended=self._out.get("blended", (n_pos, H, W)), score=self._out.get("score", (n_pos,)),
                          coord=self._out.get("coord", (n_pos, 2), torch.int32), minmax=self._out.get("minmax", (n_pos, 2)),
                          mask=self._out.get("mask", (n_pos, H, W), torch.uint8))
        if n_lab > 0:
            out["labels"] = self._out.get("labels", (H, W), torch.int32)
        with torch.cuda.device(self.device):
            check(L.olsr_lang_query_relevancy(C.byref(p), sims.data_ptr(), out["relevancy"].data_ptr(), out["smoothed"].data_ptr(),
                                              out["blended"].data_ptr(), out["score"].data_ptr(), out["coord"].data_ptr(),
                                              out["minmax"].data_ptr(), out["mask"].data_ptr(),
                                              out["labels"].data_ptr() if n_lab > 0 else None, scratch.data_ptr(), stream_ptr(self.device)))
        out["similarities"] = sims
        return out
