"""The CLIP ConvNeXt image tower restated in torch ops (include/olsr_clip_trunk.h): what the HIP kernels are compared with, and
what scripts/bench_clip_trunk.py times.

  block(state, x, dtype)             the reference's ConvNextBlock.forward (language/sed/modeling/transformer/convnext.py:75-88),
                                     pinned to vectors recorded from that module by tests/test_clip_trunk_ref_golden.py
  layer_norm_cf(x, w, b, dtype)      its LayerNorm in channels_first format (convnext.py:111-116)
  forward(state, image, dtype, ...)  normalise, resize, stem, stages, dense head (open_clip timm_model.py:125-146)
  trunk_state / block_state          drawn parameters that keep the activations O(1) through 36 blocks
  *_kernel_order                     the same in float32 with every sum in the kernels' order (CPU only, small sizes)
  TRUNK_CASES / BLOCK_CASES          the cases beyond one pixel tile and one neuron tile, each with a note of what it resolves;
  trunk_case_refs / block_case_refs  their references, computed once per process

State-dict names: _abi.clip_trunk_state (open_clip's around timm's ConvNeXt, unverified); a block's own entries carry the
names behind `blocks.j.`: conv_dw, norm, mlp.fc1, mlp.fc2, gamma.
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from online_lang_splatting_amd import _abi

EPS = 1e-6
MEAN, STD = _abi.CLIP_PIXEL_MEAN, _abi.CLIP_PIXEL_STD
SMALL = dict(depths=(1, 1, 2, 1), dims=(64, 128, 256, 512), embed_dim=64, resolution=32)
GOLDEN_CASES = {"c64_5x7": (64, 5, 7, 1), "c64_1x1": (64, 1, 1, 2), "c192_5x7": (192, 5, 7, 3), "c192_1x1": (192, 1, 1, 4)}
BLOCK_KEYS = tuple(k[2:] for k, _ in _abi.clip_block_state("b", 1))   # conv_dw.weight ... gamma

# ---- the cases beyond one 64-pixel tile and one 64-neuron tile (tests/test_gpu_clip_trunk_tiles.py) ---------------------------
# Every launch tiles its work over 64 pixels x 64 neurons; the cases above stay inside tile 0 of both.  A case's note says what
# it is there to resolve and names the mutants of tests/test_clip_trunk_ref_golden.py that it must tell from the truth.
MUTANTS = ("pixel-tile blind", "neuron-tile blind", "second output dropped")
_TILES = dict(depths=(1, 1, 2, 1), dims=(64, 128, 256, 512))
_SMALL = dict(depths=SMALL["depths"], dims=SMALL["dims"], embed_dim=SMALL["embed_dim"], resolution=SMALL["resolution"])
TRUNK_CASES = {
    "wide": dict(depths=(1, 1, 2, 1), dims=(192, 384, 768, 1536), embed_dim=48, resolution=64, image=(50, 75), state_seed=11,
                 image_seed=11,
                 note="real widths; stem 16x16 = 4 pixel tiles (pixel-tile blind); res3 from a three-launch block that writes "
                      "both outputs (second output dropped); downsample to 1536; head over 1536 with a partial neuron tile "
                      "(neuron-tile blind); up- and downsampling in one call"),
    "tiles96": dict(_TILES, embed_dim=80, resolution=96, image=(96, 131), state_seed=12, image_seed=12,
                    note="24x24 = 9 tiles, 12x12 = 2 1/4 tiles (pixel-tile blind); head on 3x3 with two neuron tiles, the "
                         "second partial (neuron-tile blind); H = R"),
    "tiles64": dict(_TILES, embed_dim=16, resolution=64, image=(77, 64), state_seed=13, image_seed=13,
                    note="16x16 = 4 tiles (pixel-tile blind); W = R; E = 16, three waves of the head without neurons "
                         "(neuron-tile blind)"),
    "same_size": dict(_SMALL, image=(32, 32), state_seed=1, image_seed=15, note="H = W = R: torch copies, the kernel samples "
                                                                               "with lambda = 0"),
    "one_row": dict(_SMALL, image=(1, 3), state_seed=1, image_seed=16, note="a one-row image: y0 = y1 = 0 everywhere"),
    "deep": dict(depths=(1, 1, 30, 1), dims=(64, 64, 64, 64), embed_dim=16, resolution=32, image=(32, 32), state_seed=14,
                 image_seed=14, note="72 launches: the mask's second word; E = 16 (neuron-tile blind)"),
}
# the trunk cases the suite compared before these: the small trunk at R = 32, state and image seed 1
OLD_TRUNK_CASES = {f"small_{h}x{w}": dict(_SMALL, image=(h, w), state_seed=1, image_seed=1, note="") for h, w in ((20, 27), (45, 61))}
# block_state(c, c) on make_map(c, h, w, c + h), as test_block_widths draws them.  64, 128, 256: the fused kernel's NT = 1, 2, 4
# (256 is OLSR_CLIP_TRUNK_FUSED_MAX_C); 320: the first three-launch width, 5 partial sums of 64 k, OUT = 1280.
BLOCK_CASES = {f"c{c}_{h}x{w}": dict(c=c, h=h, w=w, note=note + " (pixel-tile blind)")
               for c in (64, 128, 256, 320)
               for h, w, note in ((9, 12, "two tiles, w a multiple of 4"),
                                  (11, 13, "three tiles, w = 1 mod 4, pixels with a full 7x7 window"))}
_CASE_REFS = {}


def trunk_config(case):
    return {k: case[k] for k in ("depths", "dims", "embed_dim", "resolution")}


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_trunk.npz"))


def golden_case(key, z=None):
    """(block state, x, truth, ref32) of a recorded case; the parameters are stored once per width as int16 multiples of
    2^-grid."""
    z = golden() if z is None else z
    c, scale = GOLDEN_CASES[key][0], 2.0 ** int(z["grid"])
    state = OrderedDict((k, torch.from_numpy(z[f"p{c}_{k}"].astype(np.float32)) / scale) for k in BLOCK_KEYS)
    return state, torch.from_numpy(z[f"{key}_x"]), torch.from_numpy(z[f"{key}_out_f64"]), torch.from_numpy(z[f"{key}_out_f32"])


# ---- drawn parameters -------------------------------------------------------------------------------------------------------------
def _draw(name, shape, g, device, grid):
    """One tensor by its role: fan-in scaled weights, small biases, LayerNorm weights near 1, gamma in [0.05, 0.2].  grid: round
    to multiples of 2^-grid (exact in float32; keeps a stored copy small)."""
    r = lambda: torch.randn(shape, generator=g, device=device, dtype=torch.float32)  # noqa: E731
    if name.endswith("gamma"):
        t = 0.05 + 0.15 * torch.rand(shape, generator=g, device=device, dtype=torch.float32)
    elif name.endswith(".bias"):
        t = 0.1 * r()
    elif len(shape) == 1:                      # a LayerNorm's weight
        t = 1.0 + 0.1 * r()
    else:
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        t = r() / float(fan_in) ** 0.5
    if grid is not None:
        t = torch.round(t * 2.0 ** grid) / 2.0 ** grid + 0.0    # (+ 0.0: no negative zero, which an integer copy would lose)
    return t


def block_state(seed, c, grid=None, device="cpu"):
    g = torch.Generator(device=device).manual_seed(7000 + seed)
    return OrderedDict((k[2:], _draw(k, shape, g, device, grid)) for k, shape in _abi.clip_block_state("b", c))


def trunk_state(seed, depths, dims, embed_dim, device="cpu"):
    """The tower's `visual.*` entries, float32 on `device` (785 MB at the real sizes: draw those on the GPU)."""
    g = torch.Generator(device=device).manual_seed(8000 + seed)
    return OrderedDict((k, _draw(k, shape, g, device, None)) for k, shape in _abi.clip_trunk_state(depths, dims, embed_dim))


def make_image(h, w, seed, device="cpu"):
    """[3,h,w] in [0, 1] on the 8-bit grid, as ingest_frame leaves a frame."""
    g = torch.Generator().manual_seed(9000 + seed)
    return (torch.randint(0, 256, (3, h, w), generator=g).float() / 255.0).to(device)


def make_map(c, h, w, seed):
    g = torch.Generator().manual_seed(9500 + seed)
    x = torch.randn(c, h, w, generator=g, dtype=torch.float64) + 0.5 * torch.randn(c, 1, 1, generator=g, dtype=torch.float64)
    return (torch.round(x * 32.0) / 32.0).float()


# ---- the statement ----------------------------------------------------------------------------------------------------------------
def layer_norm_cf(x, w, b, dtype, eps=EPS):
    """[C,h,w]: the reference's channels_first LayerNorm."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    u = x.mean(0, keepdim=True)
    s = (x - u).pow(2).mean(0, keepdim=True)
    x = (x - u) / torch.sqrt(s + eps)
    return w[:, None, None] * x + b[:, None, None]


def _ln2d(x, w, b, eps):
    """[1,C,h,w]: LayerNorm over channels per pixel (timm's LayerNorm2d: F.layer_norm on the permuted map)."""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


def _block(s, p, x, eps):
    c = x.shape[1]
    t = F.conv2d(x, s[p + "conv_dw.weight"], s[p + "conv_dw.bias"], padding=3, groups=c).permute(0, 2, 3, 1)
    t = F.layer_norm(t, (c,), s[p + "norm.weight"], s[p + "norm.bias"], eps)
    t = F.linear(F.gelu(F.linear(t, s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"])), s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"])
    return x + (s[p + "gamma"] * t).permute(0, 3, 1, 2)


def block(state, x, dtype, prefix="", eps=EPS):
    """x [C,h,w] -> [C,h,w] in `dtype`; state: the block's entries under `prefix`."""
    with torch.no_grad():
        s = {k: v.to(dtype) for k, v in state.items() if k.startswith(prefix)}
        return _block(s, prefix, x.to(dtype)[None], eps)[0]


def normalised(image, dtype):
    """((image * 255) - mean) / std with the float32 constants the reference's buffers hold."""
    m = torch.tensor(MEAN, dtype=torch.float32, device=image.device).to(dtype)[:, None, None]
    s = torch.tensor(STD, dtype=torch.float32, device=image.device).to(dtype)[:, None, None]
    return (image.to(dtype) * 255.0 - m) / s


def forward(state, image, dtype, depths, dims, embed_dim, resolution, eps=EPS, last_inputs=None):
    """image [3,H,W] in [0, 1] -> {"clip_vis_dense" [E,R/32,R/32], "res3", "res2"} in `dtype` (on the image's device).
    last_inputs: a list to which the input of each stage's last block is appended ([d_i,h,w])."""
    R, t = resolution, "visual.trunk."
    with torch.no_grad():
        s = {k: v.to(dtype) for k, v in state.items()}
        x = F.interpolate(normalised(image, dtype)[None], size=(R, R), mode="bilinear", align_corners=False)
        x = _ln2d(F.conv2d(x, s[t + "stem.0.weight"], s[t + "stem.0.bias"], stride=4), s[t + "stem.1.weight"], s[t + "stem.1.bias"], eps)
        outs = []
        for i in range(4):
            p = f"{t}stages.{i}."
            if i > 0:
                x = _ln2d(x, s[p + "downsample.0.weight"], s[p + "downsample.0.bias"], eps)
                x = F.conv2d(x, s[p + "downsample.1.weight"], s[p + "downsample.1.bias"], stride=2)
            for j in range(depths[i]):
                if last_inputs is not None and j + 1 == depths[i]:
                    last_inputs.append(x[0])
                x = _block(s, f"{p}blocks.{j}.", x, eps)
            outs.append(x)
        h = F.layer_norm(x.permute(0, 2, 3, 1), (dims[3],), s[t + "head.norm.weight"], s[t + "head.norm.bias"], eps)
        fv = F.linear(h, s["visual.head.proj.weight"]).permute(0, 3, 1, 2)
        return {"clip_vis_dense": fv[0], "res3": outs[1][0], "res2": outs[0][0]}


# ---- float32 in the kernels' order ------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 tensors: the product is exact in double."""
    return (a.double() * b.double() + c.double()).float()


def _dense_ko(x, w, bias):
    """x [P,K], w [O,K], bias [O] or None -> [P,O]: a running float32 sum from the bias to which each 64 k's partial sum is
    added; a partial sum is one chain from 0, k in blocks of 16, inside a block k0 + 4 q + j for j = 0..3, q = 0..3 (one
    v_mfma_f32_16x16x4_f32 per j)."""
    P, K = x.shape
    acc = (bias if bias is not None else torch.zeros(w.shape[0]))[None].expand(P, -1).clone()
    wt = w.t().contiguous()
    for k64 in range(0, K, 64):
        part = torch.zeros_like(acc)
        for k0 in range(k64, min(k64 + 64, K), 16):
            for j in range(4):
                for q in range(4):
                    k = k0 + 4 * q + j
                    part = _fma32(x[:, k, None], wt[None, k], part)
        acc = acc + part
    return acc


def _ln_ko(x, w, b, eps):
    """x [P,C]: statistics in double, one fmaf with the weight and the bias."""
    d = x.double()
    mean = d.sum(1, keepdim=True) / x.shape[1]
    var = ((d - mean) ** 2).sum(1, keepdim=True) / x.shape[1]
    return _fma32(((d - mean) * (1.0 / torch.sqrt(var + eps))).float(), w[None], b[None])


def _gelu_ko(v):
    return 0.5 * v * (1.0 + torch.erf(v * np.float32(0.70710678118654752440)))


def _block_ko(s, p, x, eps):
    """x [h,w,C] float32, pixel-major as the kernels hold it."""
    h, w, c = x.shape
    dw = s[p + "conv_dw.weight"]
    acc = s[p + "conv_dw.bias"][None, None].expand(h, w, -1).clone()
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    for ky in range(7):
        for kx in range(7):
            acc = _fma32(dw[:, 0, ky, kx][None, None], xp[ky:ky + h, kx:kx + w], acc)
    t = _ln_ko(acc.reshape(h * w, c), s[p + "norm.weight"], s[p + "norm.bias"], eps)
    t = _gelu_ko(_dense_ko(t, s[p + "mlp.fc1.weight"], s[p + "mlp.fc1.bias"]))
    t = _dense_ko(t, s[p + "mlp.fc2.weight"], s[p + "mlp.fc2.bias"])
    return x + (s[p + "gamma"][None] * t).reshape(h, w, c)


def block_kernel_order(state, x, prefix="", eps=EPS):
    with torch.no_grad():
        return _block_ko(state, prefix, x.float().permute(1, 2, 0).contiguous(), eps).permute(2, 0, 1)


def _resize32(x, R):
    """[3,H,W] float32 -> [3,R,R]: upsample_bilinear2d(align_corners=False) as the kernels restate it."""
    _, H, W = x.shape

    def axis(n_in):
        d = torch.arange(R, dtype=torch.float32)
        s = torch.clamp(np.float32(np.float32(n_in) / np.float32(R)) * (d + 0.5) - 0.5, min=0.0)
        i0 = torch.clamp(s.to(torch.int64), max=n_in - 1)
        i1 = i0 + ((i0 < n_in - 1) & (n_in != R)).to(torch.int64)
        lam = s - i0.float()
        return i0, i1, lam, 1.0 - lam

    y0, y1, ly, hy = axis(H)
    x0, x1, lx, hx = axis(W)
    top = hx[None, None] * x[:, y0][:, :, x0] + lx[None, None] * x[:, y0][:, :, x1]
    bot = hx[None, None] * x[:, y1][:, :, x0] + lx[None, None] * x[:, y1][:, :, x1]
    return hy[None, :, None] * top + ly[None, :, None] * bot


def forward_kernel_order(state, image, depths, dims, embed_dim, resolution, eps=EPS):
    """forward() in float32 with every sum in the HIP kernels' order."""
    R, t, s = resolution, "visual.trunk.", state
    with torch.no_grad():
        x = _resize32(normalised(image.float(), torch.float32), R)
        n = R // 4
        cols = x.reshape(3, n, 4, n, 4).permute(1, 3, 0, 2, 4).reshape(n * n, 48)       # k = 16 c + 4 ky + kx
        x = _dense_ko(cols, s[t + "stem.0.weight"].reshape(dims[0], 48), s[t + "stem.0.bias"])
        x = _ln_ko(x, s[t + "stem.1.weight"], s[t + "stem.1.bias"], eps).reshape(n, n, dims[0])
        outs = []
        for i in range(4):
            p = f"{t}stages.{i}."
            if i > 0:
                c = dims[i - 1]
                x = _ln_ko(x.reshape(n * n, c), s[p + "downsample.0.weight"], s[p + "downsample.0.bias"], eps)
                n //= 2
                cols = x.reshape(n, 2, n, 2, c).permute(0, 2, 1, 3, 4).reshape(n * n, 4 * c)   # k = (2 ky + kx) Cin + c
                wd = s[p + "downsample.1.weight"].permute(0, 2, 3, 1).reshape(dims[i], 4 * c)
                x = _dense_ko(cols, wd, s[p + "downsample.1.bias"]).reshape(n, n, dims[i])
            for j in range(depths[i]):
                x = _block_ko(s, f"{p}blocks.{j}.", x, eps)
            outs.append(x.permute(2, 0, 1))
        h = _ln_ko(x.reshape(n * n, dims[3]), s[t + "head.norm.weight"], s[t + "head.norm.bias"], eps)
        fv = _dense_ko(h, s["visual.head.proj.weight"], None).reshape(n, n, embed_dim).permute(2, 0, 1)
        return {"clip_vis_dense": fv, "res3": outs[1], "res2": outs[0]}


# ---- the cases' references, computed once and shared by the CPU and the GPU tests -------------------------------------------------
def trunk_case_state(case):
    """The case's drawn state (the wide one is 32 M floats: a second on the CPU), once per seed and configuration."""
    key = ("state", case["state_seed"], case["depths"], case["dims"], case["embed_dim"])
    if key not in _CASE_REFS:
        _CASE_REFS[key] = trunk_state(case["state_seed"], case["depths"], case["dims"], case["embed_dim"])
    return _CASE_REFS[key]


def trunk_case_refs(name):
    """(image, truth, ref32, stage 1's last block's input in float32) of a TRUNK_CASES / OLD_TRUNK_CASES entry."""
    key = ("trunk", name)
    if key not in _CASE_REFS:
        case = TRUNK_CASES[name] if name in TRUNK_CASES else OLD_TRUNK_CASES[name]
        st, img, kw, ins = trunk_case_state(case), make_image(*case["image"], case["image_seed"]), trunk_config(case), []
        _CASE_REFS[key] = (img, forward(st, img, torch.float64, **kw), forward(st, img, torch.float32, last_inputs=ins, **kw), ins[1])
    return _CASE_REFS[key]


def block_case_refs(name):
    """(state, x, truth, ref32) of a BLOCK_CASES entry."""
    key = ("block", name)
    if key not in _CASE_REFS:
        c, h, w = (BLOCK_CASES[name][k] for k in ("c", "h", "w"))
        st, x = block_state(c, c), make_map(c, h, w, c + h)
        _CASE_REFS[key] = (st, x, block(st, x, torch.float64), block(st, x, torch.float32))
    return _CASE_REFS[key]
