"""Host side of olsr_lang_ae_train_step / olsr_lang_ae_encode / olsr_lang_ae_decode (include/olsr.h): the online language
autoencoder of the reference's back end, which turns a keyframe's 32-channel language features into the 15-channel target the
mapping loss trains the Gaussians' language codes against.

Mirrors EncoderDecoderOnline (language/autoencoder/model.py:314-354) and BackEnd.train_online_autoencoder
(utils/slam_backend.py:266-323): one call of train_step is that function's zero_grad / encode / decode / loss / backward /
Adam step, in two launches and without a host read.  GPU only; there is no torch fallback.
"""
import ctypes as C
from typing import Optional, Tuple

import torch

from . import _abi
from ._flat_state import FlatNet
from ._host import Outputs, gpu_float32, stream_ptr
from ._lib import check, lib

LAYOUTS = {"rows": _abi.LANG_AE_CODES_ROWS, "channels": _abi.LANG_AE_CODES_CHANNELS}


def _layout(layout):
    if layout not in LAYOUTS:
        raise RuntimeError(f"lang_codec: layout must be 'rows' ([N,15]) or 'channels' ([15,N]), got {layout!r}")
    return LAYOUTS[layout]


def _rows(name, t, width, dev):
    """[N, width] float32 rows on the codec's device (no conversion: a CPU or float64 tensor is an error, not a copy)."""
    t = gpu_float32(name, t, dev)
    if t.dim() != 2 or t.shape[1] != width or t.shape[0] < 1:
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected [N,{width}] with N >= 1")
    return t.contiguous()


class OnlineLanguageCodec(FlatNet):
    """The 32 -> 24 -> 15 -> 24 -> 32 autoencoder with its Adam state, all on `device`.

    flat [2351]: the parameters in state_dict order (views of it: self.views); exp_avg / exp_avg_sq: Adam's moments in the
    same order; step_dev int32[1]: the steps done, counted on the device, so that a loop of train_step calls is enqueued
    without a synchronisation.  Outputs (loss, codes) are reusable buffers: the next call of the same kind overwrites them.
    load_state_dict takes a state_dict of EncoderDecoderOnline (a reference online_15_*.pth) and leaves Adam's state as it is."""

    TABLE, WHO, WHAT = _abi.LANG_AE_STATE, "lang_codec", ("flat parameter array", "state_dict")
    HINT = "the sizes 32 / 24 / 15 are compiled into the kernels"

    def __init__(self, device, seed: Optional[int] = None):
        super().__init__(device)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.exp_avg = torch.zeros(_abi.LANG_AE_PARAMS, **f32)
        self.exp_avg_sq = torch.zeros(_abi.LANG_AE_PARAMS, **f32)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.loss = torch.zeros(4, **f32)
        self._scratch = None
        self._scratch_n = 0
        self._out = Outputs(self.device)
        self.reset_parameters(seed)

    # ---- parameters ----------------------------------------------------------------------------------------------------
    def reset_parameters(self, seed: Optional[int] = None):
        """nn.Linear's default initialisation (uniform in +-1/sqrt(fan_in) for weight and bias), drawn on the CPU."""
        g = torch.Generator()
        if seed is not None:
            g.manual_seed(seed)
        else:
            g.seed()
        fan_in = None
        for name, shape in _abi.LANG_AE_STATE:
            if name.endswith("weight"):
                fan_in = shape[1]
            bound = fan_in ** -0.5
            self.views[name].copy_((torch.rand(shape, generator=g) * 2.0 - 1.0) * bound)
        self.reset_optimizer()

    def reset_optimizer(self):
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.step_dev.zero_()

    # ---- calls ---------------------------------------------------------------------------------------------------------
    def _codes_buffer(self, key, N, layout):
        return self._out.get(key, (N, _abi.LANG_AE_CODE) if layout == "rows" else (_abi.LANG_AE_CODE, N))

    def train_step(self, features, lr: float, codes: Optional[str] = "pre", layout: str = "rows", grad_out=None,
                   step: int = 0) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """One step of train_online_autoencoder on features [N,32].  -> (loss[4] on the device = {total, L1 term,
        0.6 (1 - mean cos) term, mean cos} of the parameters before the update, codes or None).
        codes: "pre" — the codes of the forward pass (what the reference returns), "post" — re-encoded with the updated
        parameters (what it returns with viz=True; one more launch), None.  layout: "rows" [N,15] or "channels" [15,N].
        grad_out: a float32[2351] device tensor that receives the gradient (tests).  step > 0 overrides the device counter."""
        if codes not in ("pre", "post", None):
            raise RuntimeError(f"train_step: codes must be 'pre', 'post' or None, got {codes!r}")
        lay = _layout(layout)
        x = _rows("train_step: features", features, _abi.LANG_AE_IN, self.device)
        N = x.shape[0]
        L = lib()
        if self._scratch is None or self._scratch_n != N:
            self._scratch = torch.empty(L.olsr_lang_ae_scratch_bytes(N), dtype=torch.uint8, device=self.device)
            self._scratch_n = N
        out = self._codes_buffer("codes", N, layout) if codes is not None else None
        if grad_out is not None and (not grad_out.is_cuda or grad_out.device != self.device or grad_out.dtype != torch.float32
                                     or grad_out.numel() != _abi.LANG_AE_PARAMS or not grad_out.is_contiguous()):
            raise RuntimeError(f"train_step: grad_out must be a contiguous float32[2351] tensor on {self.device}")
        p = _abi.OlsrLangAeParams(lr=float(lr), beta1=0.9, beta2=0.999, eps=1e-8, step=int(step), code_layout=lay,
                                  in_dim=_abi.LANG_AE_IN, hidden_dim=_abi.LANG_AE_HIDDEN, code_dim=_abi.LANG_AE_CODE)
        with torch.cuda.device(self.device):
            check(L.olsr_lang_ae_train_step(C.byref(p), N, x.data_ptr(), self.flat.data_ptr(), self.exp_avg.data_ptr(),
                                            self.exp_avg_sq.data_ptr(), self.step_dev.data_ptr(), self.loss.data_ptr(),
                                            out.data_ptr() if codes == "pre" else None,
                                            None if grad_out is None else grad_out.data_ptr(), self._scratch.data_ptr(),
                                            stream_ptr(self.device)))
            if codes == "post":
                check(L.olsr_lang_ae_encode(N, x.data_ptr(), self.flat.data_ptr(), lay, out.data_ptr(), stream_ptr(self.device)))
        return self.loss, out

    def encode(self, features, layout: str = "rows", out=None):
        """features [N,32] -> unit-norm codes, [N,15] ("rows") or [15,N] ("channels")."""
        lay = _layout(layout)
        x = _rows("encode: features", features, _abi.LANG_AE_IN, self.device)
        N = x.shape[0]
        if out is None:
            out = self._codes_buffer("encoded", N, layout)
        with torch.cuda.device(self.device):
            check(lib().olsr_lang_ae_encode(N, x.data_ptr(), self.flat.data_ptr(), lay, out.data_ptr(), stream_ptr(self.device)))
        return out

    def decode(self, codes, layout: str = "rows"):
        """codes [N,15] ("rows") or [15,N] ("channels") -> unit-norm reconstructions [N,32]."""
        lay = _layout(layout)
        if layout == "channels":  # [15,N], passed as it is: no transpose pass, not even to read the shape
            if (not isinstance(codes, torch.Tensor) or not codes.is_cuda or codes.dtype != torch.float32
                    or codes.device != self.device):
                raise RuntimeError(f"decode: codes must be a float32 tensor on the GPU ({self.device})")
            if codes.dim() != 2 or codes.shape[0] != _abi.LANG_AE_CODE or codes.shape[1] < 1:
                raise RuntimeError(f"decode: codes has shape {tuple(codes.shape)}, expected [15,N] with N >= 1")
            c = codes.detach().contiguous()
            N = c.shape[1]
        else:
            c = _rows("decode: codes", codes, _abi.LANG_AE_CODE, self.device)
            N = c.shape[0]
        out = self._out.get("decoded", (N, _abi.LANG_AE_IN))
        with torch.cuda.device(self.device):
            check(lib().olsr_lang_ae_decode(N, c.data_ptr(), self.flat.data_ptr(), lay, out.data_ptr(), stream_ptr(self.device)))
        return out

    def language_target(self, features, hw=(192, 192)):
        """features [h*w,32] -> a new [15,h,w] tensor: low_dim.T.view(15, h, w) of the reference (utils/slam_backend.py:
        562-576), written channel-major by the encode kernel."""
        h, w = int(hw[0]), int(hw[1])
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] != h * w:
            raise RuntimeError(f"language_target: features must be [{h * w},32] for hw = {(h, w)}")
        out = torch.empty(_abi.LANG_AE_CODE, h * w, dtype=torch.float32, device=self.device)
        return self.encode(features, "channels", out=out).view(_abi.LANG_AE_CODE, h, w)


def state_views(flat):
    """name -> view of a flat [2351] tensor in the module's shape, in state_dict order."""
    return OnlineLanguageCodec.views_of(flat)


def load_state(flat, state):
    """Copies a state_dict of EncoderDecoderOnline into a flat [2351] tensor; keys and shapes must be the module's."""
    OnlineLanguageCodec.load_into(flat, state)
