"""The raw-parameter (OLSR_ACT_*) backward chains restated for the tests, and the edge rows both suites plant.

The kernels chain a gradient with respect to an ACTIVATED parameter back to the raw one (csrc/k_preprocess_bwd.hip, the
OLSR_ACT_* branches; act_normalize4_backward in csrc/olsr_device.h).  The library is compiled without contraction and without
fast-math, and float32 multiply, add, divide and square root are correctly rounded on the GPU as in numpy, so each chain can
be restated in np.float32 — every operation rounded once, in the kernels' order — and compared for EQUALITY:

  opacity   dL/dx   = g * (o * (1 - o))                         o = sigmoid(x) as the kernel evaluated it
  scale     dL/dx_k = g_k * s_k                                 s_k = exp(x_k) as the kernel evaluated it
  rotation  n = max(sqrt(((q0^2 + q1^2) + q2^2) + q3^2), 1e-12),  h = q / n,
            dot = ((h0 g0 + h1 g1) + h2 g2) + h3 g3,  dL/dq_k = (g_k - h_k * dot) / n

The only operation a CPU cannot restate bit for bit is expf, so the activated values o and s_k are INPUTS here (on the GPU
they are read back through olsr_debug_activate; the CPU test rounds a float64 exp).  The float64 truth of each chain is autograd
through torch.sigmoid / torch.exp / torch.nn.functional.normalize in double; for opacity and scale it is taken at the raw value
whose activation IS the given float32 one (logit(o), log(s) in double), so that the quality of expf is no part of the comparison.
"""
import math

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32 (round to nearest): |fl(x) - x| <= U |x| / (1 + U)
TINY = 2.0 ** -150      # half the spacing of the subnormal range: what a rounding may err by where U |x| is below it
EPS_NORM = F32(1e-12)   # F.normalize's eps, as act_normalize4 clamps with it

# roundings x 2^-24, per chain (derived in tests/test_act_ref_cpu.py's docstrings)
K_OPACITY, K_SCALE, K_ROT_FWD, K_ROT_BWD = 3, 1, 4, 18


def _f32(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    assert a.dtype == np.float32, a.dtype
    return a


# ---- the float32 restatement ----------------------------------------------------------------------------------------------
def opacity_chain(g, o):
    """g, o: float32 [P] (o the ACTIVATED opacity).  g * (o * (1 - o)), three roundings."""
    g, o = _f32(g).reshape(-1), _f32(o).reshape(-1)
    with np.errstate(all="ignore"):
        return g * (o * (F32(1.0) - o))


def scale_chain(g, s):
    """g, s: float32 [P,3] (s the ACTIVATED scale).  g_k * s_k, one rounding."""
    with np.errstate(all="ignore"):
        return _f32(g) * _f32(s)


def _norm(q):
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    return np.fmax(n, EPS_NORM)[:, None]   # (fmaxf)


def normalize_forward(q):
    """q: float32 [P,4] raw.  act_normalize4: h = q / max(|q|, 1e-12)."""
    q = _f32(q)
    with np.errstate(all="ignore"):
        return q / _norm(q)


def rotation_chain(g, q):
    """g: float32 [P,4] gradient with respect to the normalised quaternion, q: float32 [P,4] RAW.  act_normalize4_backward."""
    g, q = _f32(g), _f32(q)
    with np.errstate(all="ignore"):
        n = _norm(q)
        h = q / n
        dot = ((h[:, 0] * g[:, 0] + h[:, 1] * g[:, 1]) + h[:, 2] * g[:, 2]) + h[:, 3] * g[:, 3]
        return (g - h * dot[:, None]) / n


def clamp_active(q):
    """Rows on which the 1e-12 clamp of the norm decides (float32 [P,4] raw)."""
    q = _f32(q)
    with np.errstate(all="ignore"):
        n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    return ~(n > EPS_NORM)


# ---- the float64 truth: autograd in double ------------------------------------------------------------------------------------
def _t64(a):
    return torch.from_numpy(np.asarray(_f32(a), dtype=np.float64))


def opacity_truth(g, o):
    """d/dx of torch.sigmoid in double at the x whose sigmoid is the given float32 o, times g.  float64 [P]."""
    x = torch.logit(_t64(o).reshape(-1)).requires_grad_(True)    # (+-inf where o is 1 or 0: sigmoid is flat there)
    torch.sigmoid(x).backward(_t64(g).reshape(-1))
    return x.grad.numpy()


def scale_truth(g, s):
    """d/dx of torch.exp in double at the x whose exp is the given float32 s, times g.  float64 [P,3]."""
    x = torch.log(_t64(s)).requires_grad_(True)
    torch.exp(x).backward(_t64(g))
    return x.grad.numpy()


def rotation_truth(g, q):
    """F.normalize(q, dim=-1) in double and its vector-Jacobian product with g: (h [P,4], dL/dq [P,4]), float64."""
    x = _t64(q).requires_grad_(True)
    h = torch.nn.functional.normalize(x, dim=-1)
    h.backward(_t64(g))
    return h.detach().numpy(), x.grad.numpy()


def rotation_condition(g, q):
    """(|g_k| + |h_k| sum_j |h_j g_j|) / n in double: what the rotation chain's rounding errors are relative to."""
    g64, q64 = np.asarray(_f32(g), np.float64), np.asarray(_f32(q), np.float64)
    n = np.maximum(np.sqrt((q64 * q64).sum(1, keepdims=True)), 1e-12)
    h = q64 / n
    return (np.abs(g64) + np.abs(h) * np.abs(h * g64).sum(1, keepdims=True)) / n


def opacity_bound(truth64):
    return K_OPACITY * (U * np.abs(truth64) + TINY)


def scale_bound(truth64):
    return K_SCALE * (U * np.abs(truth64) + TINY)


def rotation_bound(g, q):
    """K_ROT_BWD x 2^-24 of the element's condition (and the underflow of an intermediate, which the divisions by n < 1 enlarge)."""
    q64 = np.asarray(_f32(q), np.float64)
    n = np.maximum(np.sqrt((q64 * q64).sum(1, keepdims=True)), 1e-12)
    return K_ROT_BWD * (U * rotation_condition(g, q) + TINY * np.maximum(1.0, 1.0 / n) ** 2)


def same_bits(a, b):
    """Equality of float32 arrays bit for bit, the sign of a zero aside, NaN equal to NaN."""
    a, b = _f32(a).reshape(-1), _f32(b).reshape(-1)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def ulp_error(got, truth64):
    """|got - truth| in units of the float32 spacing at truth (2^-149 in the subnormal range), float64 array."""
    got64, t = np.asarray(_f32(got), np.float64), np.asarray(truth64, np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(t), 2.0 ** -126)))
    return np.abs(got64 - t) / np.exp2(e - 23)


# ---- the edge rows, the same on the CPU and on the GPU -------------------------------------------------------------------------
# The suite's small camera (scene.default_camera(160, 120)): fx = fy = 80, looking down +z from the origin.  The planted
# Gaussians stand 0.25 m in front of it (320 px per metre; the near plane is at 0.2, the scene's own Gaussians begin at 0.3,
# so nothing occludes them), 2 cm (6.4 px) apart on a grid around the optical axis.
EDGE_Z, EDGE_PITCH = 0.25, 0.02
BASE_OPACITY = 1.0                                           # sigmoid: 0.73
BASE_SCALE = (math.log(0.006), math.log(0.003), math.log(0.01))   # 1 - 3 px, anisotropic: the rotation has a gradient
BASE_ROTATION = (1.02, -1.36, 0.51, 0.85)                    # norm 1.96
FAINT_OPACITY = -3.0                                         # sigmoid: 0.047 — the rows that cover the whole image
LOGIT_FLOOR = F32(-math.log(254.0))                          # logit(1 / 255): the composite's alpha floor
# Scale range of this camera.  With the 0.3 px^2 dilation every scale down to 0 has a radius of at least 2, so the smallest
# scale is the smallest exp returns in the normal range (exp(-87) = 1.6e-38; its square underflows to 0 in the covariance, and
# the scale chain's product with it is subnormal).  The largest: at z = 0.25 the radius is ceil(3 * 320 s) and is converted to
# an int32 with saturation; it is still a number of its own up to s < 2^31 / 960 = 2.24e6, log 14.62 — exp(14.5) = 1.98e6
# gives 1 850 348 032 pixels (beyond, the radius sticks at INT_MAX, and from about exp(19) on the 2-D covariance is inf - inf).
LOG_SCALE_MIN, LOG_SCALE_MAX = -87.0, 14.5


def edge_rows():
    """dict(names, means3D [E,3], opacities [E,1], scales [E,3], rotations [E,4] (all RAW, float32 numpy), clamp [E] bool).
    One edge value per row, everything else the base values above."""
    rows = []

    def add(name, op=BASE_OPACITY, sc=BASE_SCALE, rot=BASE_ROTATION):
        rows.append((name, F32(op), tuple(F32(v) for v in sc), tuple(F32(v) for v in rot)))

    lo, hi = np.nextafter(LOGIT_FLOOR, F32(-np.inf)), np.nextafter(LOGIT_FLOOR, F32(np.inf))
    for name, x in (("op +0", 0.0), ("op -0", -0.0), ("op floor-", lo), ("op floor", LOGIT_FLOOR), ("op floor+", hi),
                    ("op 16.6", 16.6), ("op 17.4", 17.4), ("op 20", 20.0), ("op -20", -20.0), ("op -90", -90.0)):
        add(name, op=x)
    add("scale 0", op=FAINT_OPACITY, sc=(0.0, 0.0, 0.0))
    add("scale min", sc=(LOG_SCALE_MIN,) * 3)
    add("scale max", op=FAINT_OPACITY, sc=(LOG_SCALE_MAX,) * 3)
    b = math.log(0.01)
    add("scale axis -8", sc=(b, b, b - 8.0))
    u = np.array([0.5, -0.5, 0.5, 0.5])
    d = np.array(BASE_ROTATION) / np.linalg.norm(BASE_ROTATION)
    for name, q in (("rot unit", u), ("rot 1e-3", d * 1e-3), ("rot 1e3", d * 1e3), ("rot 1224", (1.0, 2.0, 2.0, 4.0)),
                    ("rot 2360", (2.0, 3.0, 6.0, 0.0)), ("rot single", (0.0, 0.0, -3.0, 0.0)), ("rot zero", (0.0, 0.0, 0.0, 0.0))):
        add(name, rot=q)
    E = len(rows)
    cols = 6
    means = np.zeros((E, 3), F32)
    for i in range(E):
        r, c = divmod(i, cols)
        means[i] = ((c - (cols - 1) / 2.0) * EDGE_PITCH, (r - (E // cols) / 2.0) * EDGE_PITCH, EDGE_Z + 1e-3 * i)  # (front to back)
    rot = np.array([r[3] for r in rows], F32)
    return dict(names=[r[0] for r in rows], means3D=means, opacities=np.array([[r[1]] for r in rows], F32),
                scales=np.array([r[2] for r in rows], F32), rotations=rot, clamp=clamp_active(rot))


N_CLAMP_PLANTED = 1   # "rot zero"


def random_raw(P, seed, s_med=0.12):
    """Raw parameters as the GPU test draws them for the random rows: opacity logits ~ 1.5 N(0,1), log-scales ~ log(s_med) +
    0.6 N(0,1), quaternions of norm 0.3 - 2.3.  float32 numpy (opacities [P,1], scales [P,3], rotations [P,4])."""
    g = torch.Generator().manual_seed(seed)
    op = 1.5 * torch.randn(P, 1, generator=g)
    sc = math.log(s_med) + 0.6 * torch.randn(P, 3, generator=g)
    q = torch.randn(P, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True) * (0.3 + 2 * torch.rand(P, 1, generator=g))
    return op.numpy(), sc.numpy(), q.contiguous().numpy()


def activate64(op, sc):
    """The stand-in for the device's activated values on a CPU: act_sigmoid's 1 / (1 + expf(-x)) and expf(x) in float32 with
    a correctly rounded expf (a float64 exp rounded once; expf(90) overflows to inf as the device's does, so sigmoid(-90) = 0)."""
    with np.errstate(over="ignore"):
        e = np.exp(-np.asarray(op, np.float64)).astype(F32)
        o = F32(1.0) / (F32(1.0) + e)
        s = np.exp(np.asarray(sc, np.float64)).astype(F32)
    return o, s
