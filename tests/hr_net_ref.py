"""Torch restatement of the reference's high-resolution language feature net, dtype-generic and on the CPU: the yardstick of
tests/test_gpu_hr_net.py (float64 = "truth", float32 = "ref32") at sizes too large to commit.

    utils/slam_backend.py:547-555        hr_model(clip_vis_dense, res3, res2) under no_grad, the module in eval()
    language/supervisedNet.py:6-43       AttentionFusion: low_res_align (1x1), fusion (3x3 over the concatenation, BN, ReLU),
                                         attention (3x3, BN, ReLU, 1x1, sigmoid), out = fused * a + fused
    language/supervisedNet.py:45-109     HighResLanguageFeatureNet: initial_conv, three ConvTranspose2d(4, 2, 1) / BN / ReLU
                                         stages with bilinear resizes (align_corners=False) of res3 and res2 in between, final 1x1

forward() is the statement in torch.nn.functional ops; forward_kernel_order() is a second float32 evaluation that adds the
products up in the order the HIP kernel does (chunks of 32 input channels, the taps inside a chunk, four channels per MFMA,
ConvTranspose2d as four 2x2 phases), which measures what that order costs against forward() in float32.  tests/test_hr_net_ref_golden.py pins forward()
to arrays recorded from the reference's own module (tests/golden/make_golden_hr_net.py -> hr_net.npz).
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

C_FV, C_F3, C_F2, C_OUT = 768, 384, 192, 768
N_PACKED = 19890816     # 19 884 928 parameters + 5 888 running statistics
BN_EPS = 1e-5           # nn.BatchNorm2d's default
BN_NAMES = ("weight", "bias", "running_mean", "running_var")
KC = 32                 # the kernel's K chunk

# (module path, kind, out, in, BatchNorm path) in forward order
LAYERS = (
    ("initial_conv.0", "conv3", 512, 768, "initial_conv.1"),
    ("upsample1.0", "convT", 512, 512, "upsample1.1"),
    ("attention_fusion1.low_res_align", "conv1", 512, 384, None),
    ("attention_fusion1.fusion.0", "conv3", 512, 1024, "attention_fusion1.fusion.1"),
    ("attention_fusion1.attention.0", "conv3", 512, 512, "attention_fusion1.attention.1"),
    ("attention_fusion1.attention.3", "conv1", 512, 512, None),
    ("upsample2.0", "convT", 256, 512, "upsample2.1"),
    ("attention_fusion2.low_res_align", "conv1", 256, 192, None),
    ("attention_fusion2.fusion.0", "conv3", 256, 512, "attention_fusion2.fusion.1"),
    ("attention_fusion2.attention.0", "conv3", 256, 256, "attention_fusion2.attention.1"),
    ("attention_fusion2.attention.3", "conv1", 256, 256, None),
    ("upsample3.0", "convT", 128, 256, "upsample3.1"),
    ("final_conv", "conv1", 768, 128, None),
)


def _state():
    out = []
    for path, kind, o, i, bn in LAYERS:
        k = {"conv1": 1, "conv3": 3, "convT": 4}[kind]
        out += [(f"{path}.weight", (i, o, k, k) if kind == "convT" else (o, i, k, k)), (f"{path}.bias", (o,))]
        if bn:
            out += [(f"{bn}.{n}", (o,)) for n in BN_NAMES]
    return tuple(out)


STATE = _state()    # the module's state_dict order, without num_batches_tracked
BN_PATHS = tuple(bn for _, _, _, _, bn in LAYERS if bn)


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hr_net.npz"))


# ---- the module in its construction order, so that the default initialisation under a seed is the reference module's ----------
def _block(conv, channels):
    return nn.Sequential(conv, nn.BatchNorm2d(channels), nn.ReLU(inplace=True))


class _Fusion(nn.Module):
    def __init__(self, high, low):
        super().__init__()
        self.low_res_align = nn.Conv2d(low, high, kernel_size=1)
        self.fusion = _block(nn.Conv2d(2 * high, high, kernel_size=3, padding=1), high)
        self.attention = nn.Sequential(nn.Conv2d(high, high, kernel_size=3, padding=1), nn.BatchNorm2d(high),
                                       nn.ReLU(inplace=True), nn.Conv2d(high, high, kernel_size=1), nn.Sigmoid())


class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.initial_conv = _block(nn.Conv2d(C_FV, 512, kernel_size=3, padding=1), 512)
        self.upsample1 = _block(nn.ConvTranspose2d(512, 512, kernel_size=4, stride=2, padding=1), 512)
        self.attention_fusion1 = _Fusion(512, C_F3)
        self.upsample2 = _block(nn.ConvTranspose2d(512, 256, kernel_size=4, stride=2, padding=1), 256)
        self.attention_fusion2 = _Fusion(256, C_F2)
        self.upsample3 = _block(nn.ConvTranspose2d(256, 128, kernel_size=4, stride=2, padding=1), 128)
        self.final_conv = nn.Conv2d(128, C_OUT, kernel_size=1)


def draw_batchnorm(seed):
    """BatchNorm entries that are not the identity (the default state would hide a wrong channel order): running_mean ~
    U(-0.2, 0.2), running_var ~ U(0.05, 1.5), weight ~ U(0.5, 1.5), bias ~ U(-0.3, 0.3), float32, in STATE order."""
    g = torch.Generator().manual_seed(7000 + seed)
    ranges = dict(running_mean=(-0.2, 0.2), running_var=(0.05, 1.5), weight=(0.5, 1.5), bias=(-0.3, 0.3))
    out = OrderedDict()
    for k, shape in STATE:
        path, name = k.rsplit(".", 1)
        if path in BN_PATHS:
            lo, hi = ranges[name]
            out[k] = (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)).float()
    return out


_STATES = {}


def net_state(seed):
    """The module's default initialisation under torch.manual_seed(seed) with draw_batchnorm(seed)'s BatchNorm entries.
    float32, cached (80 MB): treat it as read-only."""
    if seed not in _STATES:
        torch.manual_seed(seed)
        sd = _Net().state_dict()
        bn = draw_batchnorm(seed)
        out = OrderedDict()
        for k, shape in STATE:
            out[k] = bn[k] if k in bn else sd[k].clone()
            assert tuple(out[k].shape) == tuple(shape), k
        _STATES[seed] = out
    return _STATES[seed]


def make_inputs(sizes, seed):
    """sizes ((h, w), (h3, w3), (h2, w2)) -> fv [768,h,w], f3 [384,h3,w3], f2 [192,h2,w2], float32.  Multiples of 1/32 of
    randn + a per-channel offset: the backbone's maps are not centred, and the coarse grid keeps the golden file small."""
    g = torch.Generator().manual_seed(6000 + seed)
    out = []
    for c, (h, w) in zip((C_FV, C_F3, C_F2), sizes):
        x = torch.randn(c, h, w, generator=g, dtype=torch.float64) + 0.5 * torch.randn(c, 1, 1, generator=g, dtype=torch.float64)
        out.append((torch.round(x * 32.0) / 32.0).float())
    return tuple(out)


# ---- the statement ----------------------------------------------------------------------------------------------------------
def _bn_relu(s, bn, x, eps):
    return F.relu(F.batch_norm(x, s[f"{bn}.running_mean"], s[f"{bn}.running_var"], s[f"{bn}.weight"], s[f"{bn}.bias"],
                               training=False, eps=eps))


def forward(state, fv, f3, f2, dtype, eps=BN_EPS):
    """HighResLanguageFeatureNet.forward in eval() in `dtype`: [768,h,w], [384,.,.], [192,.,.] -> [768,8h,8w]."""
    s = {k: v.to(dtype) for k, v in state.items()}
    with torch.no_grad():
        x = fv.to(dtype)[None]
        x = _bn_relu(s, "initial_conv.1", F.conv2d(x, s["initial_conv.0.weight"], s["initial_conv.0.bias"], padding=1), eps)
        for n, low in ((1, f3), (2, f2)):
            up, af = f"upsample{n}", f"attention_fusion{n}"
            x = _bn_relu(s, f"{up}.1", F.conv_transpose2d(x, s[f"{up}.0.weight"], s[f"{up}.0.bias"], stride=2, padding=1), eps)
            low = F.interpolate(low.to(dtype)[None], size=(x.shape[2], x.shape[3]), mode="bilinear", align_corners=False)
            low = F.conv2d(low, s[f"{af}.low_res_align.weight"], s[f"{af}.low_res_align.bias"])
            fused = torch.cat([x, low], dim=1)
            fused = _bn_relu(s, f"{af}.fusion.1", F.conv2d(fused, s[f"{af}.fusion.0.weight"], s[f"{af}.fusion.0.bias"], padding=1),
                             eps)
            a = _bn_relu(s, f"{af}.attention.1",
                         F.conv2d(fused, s[f"{af}.attention.0.weight"], s[f"{af}.attention.0.bias"], padding=1), eps)
            a = torch.sigmoid(F.conv2d(a, s[f"{af}.attention.3.weight"], s[f"{af}.attention.3.bias"]))
            x = fused * a + fused
        x = _bn_relu(s, "upsample3.1", F.conv_transpose2d(x, s["upsample3.0.weight"], s["upsample3.0.bias"], stride=2, padding=1),
                     eps)
        return F.conv2d(x, s["final_conv.weight"], s["final_conv.bias"])[0]


# ---- ConvTranspose2d(4, 2, 1) as four parity phases ------------------------------------------------------------------------------
def phase_taps(parity):
    """Output row 2 m + parity of ConvTranspose2d(k 4, s 2, p 1) reads input rows m + d with kernel row k, from PyTorch's
    oy = 2 iy - 1 + ky:  k = parity + 1 - 2 d, d in {parity - 1, parity}.  -> ((d, k), (d, k)) in the kernel's tap order."""
    return tuple((d, parity + 1 - 2 * d) for d in (parity - 1, parity))


def _shift(x, dy, dx):
    """x[..., y + dy, x + dx] with zeros outside the image."""
    H, W = x.shape[-2:]
    return F.pad(x, (1, 1, 1, 1))[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def conv_transpose_phases(x, weight, bias):
    """F.conv_transpose2d(x, weight, bias, stride=2, padding=1) for a 4x4 kernel, written as four 2x2 convolutions:
    x [1,I,H,W], weight [I,O,4,4] -> [1,O,2H,2W]."""
    _, _, H, W = x.shape
    out = x.new_zeros(1, weight.shape[1], 2 * H, 2 * W)
    for py in (0, 1):
        for px in (0, 1):
            acc = bias.view(1, -1, 1, 1).expand(1, -1, H, W).clone()
            for dy, ky in phase_taps(py):
                for dx, kx in phase_taps(px):
                    acc = acc + torch.einsum("io,bihw->bohw", weight[:, :, ky, kx], _shift(x, dy, dx))
            out[:, :, py::2, px::2] = acc
    return out


# ---- float32 in the kernel's order -------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf(a, b, c) for float32 tensors: the product is exact in double."""
    return (a.double() * b.double() + c.double()).float()


def _fold(s, bn, eps):
    a = s[f"{bn}.weight"].double() / torch.sqrt(s[f"{bn}.running_var"].double() + eps)
    b = s[f"{bn}.bias"].double() - s[f"{bn}.running_mean"].double() * a
    return a.float().view(1, -1, 1, 1), b.float().view(1, -1, 1, 1)


def _conv_ko(srcs, taps, bias):
    """srcs: the sources along K, each [1,C,H,W]; taps: [(dy, dx, W[out, in])] with in over the concatenation.  One float32
    accumulator per output, started at the bias: chunk by chunk of 32 channels, tap by tap inside a chunk, four channels (one
    v_mfma_f32_16x16x4_f32) at a time in the kernel's interleaved order."""
    x = torch.cat(srcs, dim=1)
    acc = bias.view(1, -1, 1, 1).expand(1, -1, x.shape[2], x.shape[3]).clone()
    shifted = {(dy, dx): _shift(x, dy, dx) for dy, dx, _ in taps}
    for k0 in range(0, x.shape[1], KC):
        for dy, dx, w in taps:
            xs = shifted[(dy, dx)]
            for kb in range(k0, k0 + KC, 16):
                for j in range(4):      # one MFMA: the four channels kb + 4 q + j, q = 0..3, added to the accumulator at once
                    k = [kb + 4 * q + j for q in range(4)]
                    acc = acc + torch.einsum("oi,bihw->bohw", w[:, k], xs[:, k])
    return acc


def _conv3_ko(s, path, srcs):
    w = s[f"{path}.weight"]
    return _conv_ko(srcs, [(ky - 1, kx - 1, w[:, :, ky, kx]) for ky in range(3) for kx in range(3)], s[f"{path}.bias"])


def _conv1_ko(s, path, x):
    return _conv_ko([x], [(0, 0, s[f"{path}.weight"][:, :, 0, 0])], s[f"{path}.bias"])


def _convT_ko(s, path, x):
    w, b = s[f"{path}.weight"], s[f"{path}.bias"]
    out = x.new_zeros(1, w.shape[1], 2 * x.shape[2], 2 * x.shape[3])
    for py in (0, 1):
        for px in (0, 1):
            taps = [(dy, dx, w[:, :, ky, kx].t()) for dy, ky in phase_taps(py) for dx, kx in phase_taps(px)]
            out[:, :, py::2, px::2] = _conv_ko([x], taps, b)
    return out


def bilinear32(x, H, W):
    """upsample_bilinear2d(align_corners=False) of x [1,C,h,w] to H x W in float32, operation for operation as the kernel samples
    it: src = max(scale (dst + 0.5) - 0.5, 0) with scale = in / out in float; a dimension that keeps its size is copied."""
    _, _, h, w = x.shape

    def axis(n_in, n_out):
        d = torch.arange(n_out, dtype=torch.float32)
        scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
        src = torch.clamp(scale * (d + 0.5) - 0.5, min=0.0)
        i0 = torch.clamp(src.to(torch.int64), max=n_in - 1)
        i1 = i0 + ((i0 < n_in - 1) & (n_in != n_out)).to(torch.int64)
        lam = src - i0.float()
        return i0, i1, lam, 1.0 - lam

    y0, y1, ly, hy = axis(h, H)
    x0, x1, lx, hx = axis(w, W)
    ly, hy = ly.view(1, 1, H, 1), hy.view(1, 1, H, 1)
    lx, hx = lx.view(1, 1, 1, W), hx.view(1, 1, 1, W)
    top = hx * x[:, :, y0][:, :, :, x0] + lx * x[:, :, y0][:, :, :, x1]
    bot = hx * x[:, :, y1][:, :, :, x0] + lx * x[:, :, y1][:, :, :, x1]
    return hy * top + ly * bot


def forward_kernel_order(state, fv, f3, f2, eps=BN_EPS):
    """forward() in float32 with every sum in the HIP kernel's order and its epilogues (folded BatchNorm as one fmaf, the gate
    as one fmaf)."""
    s = state

    def bn_relu(bn, h):
        a, b = _fold(s, bn, eps)
        return torch.relu(_fma32(a, h, b))

    with torch.no_grad():
        x = bn_relu("initial_conv.1", _conv3_ko(s, "initial_conv.0", [fv[None]]))
        for n, low in ((1, f3), (2, f2)):
            up, af = f"upsample{n}", f"attention_fusion{n}"
            x = bn_relu(f"{up}.1", _convT_ko(s, f"{up}.0", x))
            low = _conv1_ko(s, f"{af}.low_res_align", bilinear32(low[None], x.shape[2], x.shape[3]))
            fused = bn_relu(f"{af}.fusion.1", _conv3_ko(s, f"{af}.fusion.0", [x, low]))
            a = bn_relu(f"{af}.attention.1", _conv3_ko(s, f"{af}.attention.0", [fused]))
            a = torch.sigmoid(_conv1_ko(s, f"{af}.attention.3", a))
            x = _fma32(fused, a, fused)
        x = bn_relu("upsample3.1", _convT_ko(s, "upsample3.0", x))
        return _conv1_ko(s, "final_conv", x)[0]


# ---- the golden cases ------------------------------------------------------------------------------------------------------
# key -> (((h, w), (h3, w3), (h2, w2)), seed): res3 / res2 resized up and down, and the back end's identity
GOLDEN_CASES = OrderedDict([("mixed2x3", (((2, 3), (5, 7), (9, 11)), 0)), ("identity3x5", (((3, 5), (6, 10), (12, 20)), 1))])
GOLDEN_CHANNELS = tuple(range(5, C_OUT, 24))    # the 32 output channels the golden keeps
assert len(GOLDEN_CHANNELS) == 32


def make_case(key):
    """-> (state, (fv, f3, f2))."""
    sizes, seed = GOLDEN_CASES[key]
    return net_state(300 + seed), make_inputs(sizes, seed)


def err(x, truth):
    """(max, rms) of |x - truth| in double."""
    d = (x.double() - truth.double()).abs()
    return float(d.max()), float((d ** 2).mean().sqrt())
