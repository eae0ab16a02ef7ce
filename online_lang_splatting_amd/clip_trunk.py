"""Host side of include/olsr_clip_trunk.h: the CLIP ConvNeXt image tower, an RGB frame in, the three maps the HR net reads out.

Mirrors what the reference reaches through language/sed/sed_model.py:154-197 and open_clip's TimmModel.forward(x, dense=True)
(timm_model.py:125-146) in eval(), float32, forward only: pixel normalisation, the bilinear resize to `resolution`, stem, four
stages of ConvNeXt blocks, the dense head.  GPU only; there is no torch fallback.

The state-dict names are open_clip's around timm's ConvNeXt (`visual.trunk.stem.0.weight`, `visual.trunk.stages.2.blocks.5.mlp.
fc1.weight`, `visual.trunk.stages.1.downsample.1.weight`, `visual.trunk.head.norm.weight`, `visual.head.proj.weight`, ...),
RESTATED FROM MEMORY AND UNVERIFIED: neither timm nor a checkpoint was at hand.  load_state_dict therefore raises on any name
it expects and does not find, and on any `visual.*` entry it was given and did not use.
"""
import ctypes as C
from collections import OrderedDict

import torch

from . import _abi, _flat_state
from ._host import Outputs, planes, stream_ptr
from ._lib import check, lib

WHO = "clip_trunk"


def _pack(name, w):
    """A state-dict tensor as the kernels read it: conv_dw [C,1,7,7] -> [49,C]; downsample.1 [o,i,2,2] -> [o,4,i]; the stem's
    [d0,3,4,4] and the Linear weights lie as they are."""
    if name.endswith("conv_dw.weight"):
        return w.reshape(w.shape[0], 49).t()
    if name.endswith("downsample.1.weight"):
        return w.permute(0, 2, 3, 1)
    return w


def _unpack(name, p, shape):
    if name.endswith("conv_dw.weight"):
        return p.reshape(49, shape[0]).t().reshape(shape).contiguous()
    if name.endswith("downsample.1.weight"):
        return p.reshape(shape[0], 2, 2, shape[1]).permute(0, 3, 1, 2).contiguous()
    return p.reshape(shape).clone()


class ClipTrunk(_flat_state.FlatNet):
    """The tower's parameters as one packed float32 array `flat` on `device` (layout: include/olsr_clip_trunk.h)."""

    WHO, WHAT, HINT = WHO, ("packed tower array", "tower state"), "the widths were given to the constructor"

    def __init__(self, device, state=None, depths=_abi.CLIP_TRUNK_DEPTHS, dims=_abi.CLIP_TRUNK_DIMS,
                 embed_dim=_abi.CLIP_TRUNK_EMBED, resolution=768, mean=_abi.CLIP_PIXEL_MEAN, std=_abi.CLIP_PIXEL_STD,
                 eps: float = _abi.CLIP_LN_EPS):
        self.depths, self.dims = tuple(int(d) for d in depths), tuple(int(d) for d in dims)
        self.embed_dim, self.resolution, self.eps = int(embed_dim), int(resolution), float(eps)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(self.depths) != 4 or len(self.dims) != 4 or len(self.mean) != 3 or len(self.std) != 3:
            raise RuntimeError(f"{WHO}: four depths, four dims, three means and three stds")
        n = int(lib().olsr_clip_trunk_packed_floats(C.byref(self._params(1, 1))))
        if n == 0 or not self.eps > 0.0:
            raise RuntimeError(f"{WHO}: dims must be multiples of 64, embed_dim of 16, resolution of 32, depths >= 1 and eps "
                               f"positive (got depths {self.depths}, dims {self.dims}, embed_dim {self.embed_dim}, resolution "
                               f"{self.resolution}, eps {self.eps})")
        self.STATE = _abi.clip_trunk_state(self.depths, self.dims, self.embed_dim)
        # (the packed array holds every tensor's elements, rearranged: the base class sizes `flat` by this table)
        self.TABLE = tuple((k, (_flat_state._numel(shape),)) for k, shape in self.STATE)
        super().__init__(device)
        assert self.flat.numel() == n, (self.flat.numel(), n)
        self.n_launches = int(lib().olsr_clip_trunk_launches(C.byref(self._params(1, 1))))
        self._offset, off = {}, 0
        for k, (m,) in self.TABLE:
            self._offset[k], off = off, off + m
        self._work = None
        self._block_work = {}
        self._out = Outputs(self.device)
        if state is not None:
            self.load_state_dict(state)

    def _params(self, H, W, launches=0, workspace_bytes=0):
        p = _abi.OlsrClipTrunkParams(embed_dim=self.embed_dim, H=H, W=W, R=self.resolution, ln_eps=self.eps,
                                     workspace_bytes=workspace_bytes)
        p.depths[:], p.dims[:], p.mean[:], p.std[:] = self.depths, self.dims, self.mean, self.std
        p.launches[0], p.launches[1] = int(launches) & (2**64 - 1), int(launches) >> 64
        return p

    @property
    def views(self):
        """name -> flat view of a tensor's packed elements."""
        return _flat_state.views(self.flat, self.TABLE, WHO, self.WHAT[0])

    def load_state_dict(self, state):
        """An open_clip checkpoint as it is ({"state_dict": ...} or the plain dict, with or without a "module." prefix): every
        `visual.*` entry must be one of the tower's and every one of the tower's must be there; the text tower's entries are
        ignored.  The names are unverified (see the module's docstring)."""
        state = _flat_state.unwrap(state, WHO, prefix="module.", keep="visual.")
        shapes = _flat_state.check_keys(state, self.STATE, WHO, self.WHAT[1])
        for k, shape in shapes.items():
            if not isinstance(state[k], torch.Tensor) or tuple(state[k].shape) != tuple(shape):
                got = tuple(state[k].shape) if isinstance(state[k], torch.Tensor) else type(state[k]).__name__
                raise RuntimeError(f"{WHO}: {k} has shape {got}, expected {tuple(shape)} ({self.HINT})")
        for k, v in self.views.items():
            v.copy_(_pack(k, state[k].detach().to(device=self.device, dtype=torch.float32)).reshape(-1))

    def state_dict(self):
        """The checkpoint's `visual.*` entries out of the packed array: new tensors in the module's shapes."""
        views = self.views
        return OrderedDict((k, _unpack(k, views[k], shape)) for k, shape in self.STATE)

    # ---- calls ---------------------------------------------------------------------------------------------------------
    def workspace(self):
        if self._work is None:
            n = int(lib().olsr_clip_trunk_workspace_bytes(C.byref(self._params(1, 1))))
            self._work = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._work

    def forward(self, image, launches: int = 0):
        """image [3,H,W] float32 in [0, 1] (as ingest_frame leaves it) -> {"clip_vis_dense" [E,R/32,R/32], "res3" [d1,R/8,R/8],
        "res2" [d0,R/4,R/4]}: buffers of this object, overwritten by the next call.  launches: bit k switches launch k of
        the n_launches on (0: all)."""
        B, H, W, stride, ptrs = planes("clip_trunk.forward: ", "image", image, 3, self.device)
        if B != 1 or (stride != H * W):
            raise RuntimeError(f"clip_trunk.forward: one contiguous [3,H,W] image is expected (shape {tuple(image.shape)}, "
                               f"strides {tuple(image.stride())})")
        R, d = self.resolution, self.dims
        out = {"clip_vis_dense": self._out.get("fv", (self.embed_dim, R // 32, R // 32)),
               "res3": self._out.get("f3", (d[1], R // 8, R // 8)), "res2": self._out.get("f2", (d[0], R // 4, R // 4))}
        work = self.workspace()
        p = self._params(H, W, launches, work.numel())
        with torch.cuda.device(self.device):
            check(lib().olsr_clip_trunk_forward(C.byref(p), ptrs[0], self.flat.data_ptr(), out["res2"].data_ptr(),
                                                out["res3"].data_ptr(), out["clip_vis_dense"].data_ptr(), work.data_ptr(),
                                                stream_ptr(self.device)))
        return out

    __call__ = forward

    def block(self, x, stage: int, index: int):
        """Block `index` of stage `stage` on x [d[stage],h,w] (contiguous) -> a [d[stage],h,w] buffer of this object."""
        if not (0 <= stage < 4 and 0 <= index < self.depths[stage]):
            raise RuntimeError(f"clip_trunk.block: there is no block {index} in stage {stage} (depths {self.depths})")
        c = self.dims[stage]
        B, h, w, stride, ptrs = planes("clip_trunk.block: ", "x", x, c, self.device)
        if B != 1 or stride != h * w:
            raise RuntimeError(f"clip_trunk.block: one contiguous [{c},h,w] map is expected (shape {tuple(x.shape)}, strides "
                               f"{tuple(x.stride())})")
        n = int(lib().olsr_convnext_block_workspace_bytes(c, h, w))
        if n == 0:
            raise RuntimeError(f"clip_trunk.block: bad sizes {(c, h, w)}")
        work = self._block_work.get((c, h, w))
        if work is None:
            work = self._block_work[(c, h, w)] = torch.empty(n, dtype=torch.uint8, device=self.device)
        y = self._out.get(("block", c), (c, h, w))
        if y.data_ptr() == ptrs[0]:   # (a chain of blocks feeds a block its predecessor's buffer: out of place)
            y = self._out.get(("block'", c), (c, h, w))
        at = self._offset[f"visual.trunk.stages.{stage}.blocks.{index}.conv_dw.weight"]
        p = _abi.OlsrConvnextBlockParams(C=c, h=h, w=w, ln_eps=self.eps, workspace_bytes=n)
        with torch.cuda.device(self.device):
            check(lib().olsr_convnext_block(C.byref(p), ptrs[0], self.flat.data_ptr() + 4 * at, y.data_ptr(), work.data_ptr(),
                                            stream_ptr(self.device)))
        return y

    def feature_fn(self, hr_net, encoder=None):
        """A callable for OnlineSlam(feature_fn=...): (frame index, image [3,H,W]) -> ("add_keyframe_backbone", fv, f3, f2,
        hr_net[, encoder]), which slam.py hands to its targets object.  With `encoder` for OnlineLanguageTargets (whose
        add_keyframe_backbone takes it), without for SingleStageTargets."""
        tail = (hr_net,) if encoder is None else (hr_net, encoder)

        def fn(_idx, image):
            o = self.forward(image)
            return ("add_keyframe_backbone", o["clip_vis_dense"][None], o["res3"][None], o["res2"][None]) + tail

        return fn
