"""Host side of olsr_ss_encoder_encode / olsr_ss_query_sims (include/olsr_single_stage.h): the language side of a
`language.single_stage_ae: True` configuration, which seven of the reference's eight Replica configs are.

There one general AutoencoderMLP goes straight to the 15-channel code and back (utils/slam_backend.py:117-119,
eval/evaluate_langslam.py:358-367; language/autoencoder/model.py:15-62) and nothing is trained online:
    encoder 768 -> 384 -> 192 -> 96 -> 48 -> 24 -> 15        decoder 15 -> 24 -> 48 -> 96 -> 192 -> 384 -> 384 -> 768
A keyframe's target is auto_model.encode(rows).T.view(15,192,192) (slam_backend.py:556-576 with :562 false): SingleStageEncoder
and SingleStageTargets.  The 2-D evaluation decodes a rendered code map with model.decode(codes) alone
(evaluate_langslam.py:266-273): SingleStageQuery, a LanguageQuery whose stage A is the single-stage decoder's, so that
QueryEvaluator and tsdf.label_points take it as it is.  GPU only; there is no torch fallback.
"""
import ctypes as C
from typing import Dict, Sequence

import torch

from . import _abi
from ._flat_state import CHECKPOINT_PREFIX, BatchNormEncoder, FlatNet
from ._host import Outputs, stream_ptr
from ._lib import OlsrError, check, lib
from .lang_codec import _layout
from .lang_encoder import feature_items
from .lang_query import FEATURE_DIM, LanguageQuery

N_ENCODER, N_DECODER = _abi.SS_ENCODER_PARAMS, _abi.SS_DECODER_PARAMS
CODE_DIM = _abi.SS_ENCODER_WIDTHS[-1]
MASK_THRESH = 0.5   # evaluate_langslam.py's --mask_thresh


class SingleStageEncoder(BatchNormEncoder):
    """AutoencoderMLP.encoder 768 -> 15 with its BatchNorm running statistics as a flat float32 array on `device`."""

    TABLE, WIDTHS, PARAMS = _abi.SS_ENCODER_STATE, _abi.SS_ENCODER_WIDTHS, _abi.OlsrSsEncoderParams
    WHO = "lang_single_stage"
    HINT = f"the widths {WIDTHS} are compiled into the kernel"

    def encode(self, features, layout: str = "channels", out=None):
        """features [N,768], [768,h,w], [1,768,h,w] or [B,768,h,w] (read in place, one launch per item) -> unit codes [15,N]
        ("channels": .view(15,h,w) is the keyframe's target) or [N,15] ("rows"); for a batch of B > 1 [B,15,N] or [B,N,15].
        Without `out` the result is a reusable buffer: the next call of the same size and layout overwrites it."""
        code_layout = _layout(layout)
        lay, N, stride, ptrs = feature_items(self.device, "encode", features)
        B = len(ptrs)
        item = (CODE_DIM, N) if code_layout == _abi.LANG_AE_CODES_CHANNELS else (N, CODE_DIM)
        shape = item if B == 1 else (B,) + item
        if out is None:
            out = self._out.get(layout, shape)
        else:
            self._out.check_out(f"encode: out must be a contiguous float32 {list(shape)} tensor", out, shape)
        p = self._params(lay, code_layout, stride)
        stream = stream_ptr(self.device)
        per = N * CODE_DIM * 4
        with torch.cuda.device(self.device):
            for b, ptr in enumerate(ptrs):
                check(lib().olsr_ss_encoder_encode(C.byref(p), N, ptr, self.flat.data_ptr(), out.data_ptr() + b * per, stream))
        return out


class SingleStageDecoder(FlatNet):
    """AutoencoderMLP.decoder 15 -> 24 -> 48 -> 96 -> 192 -> 384 -> 384 -> 768 as a flat float32 array on `device`."""

    TABLE, WHO, WHAT = _abi.SS_DECODER_STATE, "lang_single_stage", ("flat decoder array", "decoder state")
    HINT = f"the widths {_abi.SS_DECODER_WIDTHS} are compiled into the kernels"
    PREFIX, KEEP = CHECKPOINT_PREFIX, "decoder."


def encoder_views(flat):
    """name -> view of a flat [396927] tensor in the shapes of the single-stage AutoencoderMLP.encoder, in state_dict order."""
    return SingleStageEncoder.views_of(flat)


def decoder_views(flat):
    """name -> view of a flat [542544] tensor in the shapes of the single-stage AutoencoderMLP.decoder, in state_dict order."""
    return SingleStageDecoder.views_of(flat)


def load_encoder_state(flat, state):
    """Copies the encoder of a single-stage AutoencoderMLP into a flat [396927] tensor.  `state` is a Lightning checkpoint
    ({"state_dict": {"model.encoder.0.weight": ...}}), its state_dict, or a plain AutoencoderMLP state dict; decoder entries
    and num_batches_tracked are ignored, the encoder's names and shapes must be the module's."""
    SingleStageEncoder.load_into(flat, state)


def load_decoder_state(flat, state):
    """Copies the decoder of a single-stage AutoencoderMLP into a flat [542544] tensor; `state` as load_encoder_state takes it,
    encoder and BatchNorm entries are ignored."""
    SingleStageDecoder.load_into(flat, state)


class SingleStageQuery(LanguageQuery):
    """LanguageQuery for code maps of a single-stage run: stage A is olsr_ss_query_sims (codes -> model.decode -> products with
    the phrases, no online decoder), everything else (set_phrases, set_labels, similarities, relevancy, localise and stage B)
    is LanguageQuery's.  thresh is 0.5, evaluate_langslam.py's --mask_thresh."""

    def __init__(self, decoder: SingleStageDecoder):
        if not isinstance(decoder, SingleStageDecoder):
            raise RuntimeError("SingleStageQuery: a SingleStageDecoder is expected")
        self.decoder, self.codec, self.device = decoder, None, decoder.device
        self.thresh = MASK_THRESH
        self._pos = self._neg = None
        self._labels = torch.zeros(0, FEATURE_DIM, dtype=torch.float32, device=self.device)
        self._phrases = None
        self._out, self._scratch = Outputs(self.device), None

    def _sims(self, p, codes):
        # p carries the two-stage width list, which stage B validates; stage A takes the same sizes under its own list
        ps = _abi.set_widths(_abi.OlsrLangQueryParams.from_buffer_copy(p), _abi.SS_DECODER_WIDTHS)
        sims = self._out.get("sims", (p.K, p.dec_height, p.dec_width))
        with torch.cuda.device(self.device):
            check(lib().olsr_ss_query_sims(C.byref(ps), codes.data_ptr(), self.decoder.flat.data_ptr(), self._phrases.data_ptr(),
                                           sims.data_ptr(), stream_ptr(self.device)))
        return sims


class SingleStageTargets:
    """The language targets of the mapping loop in single-stage mode: a keyframe's [15,h,w] target is the encoder's codes of
    its high-resolution map, auto_model.encode(rows).T.view(15,h,w) (utils/slam_backend.py:556-576 with :562 false).  Nothing
    is trained, so nothing but the targets is kept; the interface is OnlineLanguageTargets' as MappingStep.targets uses it."""

    def __init__(self, encoder: SingleStageEncoder, hw=(192, 192)):
        if not isinstance(encoder, SingleStageEncoder):
            raise RuntimeError("SingleStageTargets: a SingleStageEncoder is expected")
        self.encoder, self.hw = encoder, (int(hw[0]), int(hw[1]))
        self.targets: Dict = {}

    def add_keyframe(self, view_id, codes: torch.Tensor) -> torch.Tensor:
        """codes [15,h,w] (or [15,h*w]) float32 on the encoder's device, e.g. labels read from file: stored as the view's
        target.  The codes are copied: the caller may reuse its buffer.  -> that target."""
        h, w = self.hw
        if (not isinstance(codes, torch.Tensor) or codes.dtype != torch.float32 or codes.device != self.encoder.device
                or codes.dim() not in (2, 3) or codes.shape[0] != CODE_DIM or codes.numel() != CODE_DIM * h * w):
            raise RuntimeError(f"add_keyframe: codes must be a float32 [{CODE_DIM},{h},{w}] tensor on {self.encoder.device} "
                               f"for hw = {self.hw}")
        self.targets[view_id] = codes.detach().reshape(CODE_DIM, h, w).clone()
        return self.targets[view_id]

    def add_keyframe_hr(self, view_id, hr_features: torch.Tensor) -> torch.Tensor:
        """hr_features [1,768,h,w] (or [768,h,w], or [h*w,768] rows) float32 on the encoder's device: the encoder writes the
        view's [15,h,w] target straight into the tensor that is kept.  -> that target."""
        h, w = self.hw
        target = torch.empty(CODE_DIM, h * w, dtype=torch.float32, device=self.encoder.device)
        try:
            self.encoder.encode(hr_features, layout="channels", out=target)
        except OlsrError:
            raise
        except RuntimeError as e:
            raise RuntimeError(f"add_keyframe_hr: features must encode to [{CODE_DIM},{h * w}] for hw = {self.hw}: {e}") from e
        self.targets[view_id] = target.view(CODE_DIM, h, w)
        return self.targets[view_id]

    def add_keyframe_backbone(self, view_id, fv: torch.Tensor, f3: torch.Tensor, f2: torch.Tensor, hr_net) -> torch.Tensor:
        """fv [1,768,h/8,w/8], f3 [1,384,.,.], f2 [1,192,.,.]: the backbone's clip_vis_dense, res3 and res2; hr_net an
        hr_net.HighResLanguageNet.  Its [1,768,h,w] map (a buffer of hr_net's) goes through add_keyframe_hr: from the
        backbone's three maps to the stored target without a torch op in between.  -> the [15,h,w] target."""
        return self.add_keyframe_hr(view_id, hr_net.forward(fv, f3, f2))

    def rehearse(self, view_ids: Sequence) -> None:
        """Nothing is trained in single-stage mode: checks the ids, as OnlineLanguageTargets.rehearse does, and returns."""
        for v in view_ids:
            if v not in self.targets:
                raise KeyError(f"rehearse: view {v!r} was never added")

    def targets_for(self, view_ids: Sequence):
        """The third slot of MappingStep.targets for these views, in order."""
        return [self.targets[v] for v in view_ids]
