"""Yardsticks for the point-cloud metrics (include/olsr.h, "point-cloud metrics"), in numpy.

emd_ref      the approximate earth mover's distance as the header states it, written with the dense [n,m] arrays (for small
             n * m).  dtype=float64 is the truth.  The float32 variants span what a float32 implementation may legitimately do:
             two summation orders (order="sequential": one term after the other, as the reference's loops; "pairwise": numpy's
             pairwise reduction) and two exps (exp="libm": numpy's exp of level * d; "exp2": 2^(x log2 e) with the product and
             the result rounded to float32, the form the kernel feeds the hardware's 2^x).
chamfer_ref  brute-force Chamfer: dtype=float64, or float32 with the kernel's expression (dx dx + dy dy) + dz dz for the
             squared distance, first index on ties, then sqrt and the mean in double.
cases()      the seeded clouds every test and the golden fixture share.
"""
import numpy as np

LEVELS = [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]
LOG2E = 1.4426950408889634
VARIANTS = [(o, e) for o in ("sequential", "pairwise") for e in ("libm", "exp2")]


def _dist2(x1, x2, dtype):
    a, b = x1.astype(dtype)[:, None, :], x2.astype(dtype)[None, :, :]
    dx, dy, dz = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], b[..., 2] - a[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _sum(a, axis, order, dtype):
    if order == "pairwise" or dtype == np.float64:
        return a.sum(axis=axis, dtype=dtype)
    # one term after the other in float32
    a = np.ascontiguousarray(np.moveaxis(a, axis, 0))
    acc = a[0].copy()
    for t in a[1:]:
        acc += t
    return acc


def _exp(level, d, exp, dtype):
    if dtype == np.float64:
        return np.exp(level * d)
    x = (dtype(level) * d).astype(dtype)
    if exp == "libm":
        return np.exp(x).astype(dtype)
    return np.exp2((x * dtype(LOG2E)).astype(dtype).astype(np.float64)).astype(dtype)


def emd_ref(x1, x2, dtype=np.float64, order="sequential", exp="libm", dense=False):
    """-> dict cost (sum d * w, undivided, float64), emd (cost / n), residual (sum remainL, sum remainR after the last level);
    dense=True adds cost_dense: the reference's own form, sum d * match over the matrix the levels' w accumulate into."""
    dtype = np.dtype(dtype).type
    n, m = x1.shape[0], x2.shape[0]
    multiL, multiR = (1, n // m) if n >= m else (m // n, 1)
    d = _dist2(x1, x2, dtype)
    remainL, remainR = np.full(n, multiL, dtype), np.full(m, multiR, dtype)
    eps = dtype(1e-9)
    cost = 0.0
    match = np.zeros((n, m), dtype) if dense else None
    for level in LEVELS:
        e = _exp(level, d, exp, dtype)
        ratioL = remainL / (eps + _sum(e * remainR[None, :], 1, order, dtype))
        sumr = _sum(e * ratioL[:, None], 0, order, dtype) * remainR
        ratioR = np.minimum(remainR / (sumr + eps), dtype(1)) * remainR
        remainR = np.maximum(dtype(0), remainR - sumr)
        w = e * ratioL[:, None] * ratioR[None, :]
        cost += float(_sum(d * w, 1, order, dtype).astype(np.float64).sum())
        remainL = np.maximum(dtype(0), remainL - _sum(w, 1, order, dtype))
        if dense:
            match += w
    out = dict(cost=cost, emd=cost / n, residual=(float(remainL.astype(np.float64).sum()), float(remainR.astype(np.float64).sum())))
    if dense:
        out["cost_dense"] = float((d * match).astype(np.float64).sum())
    return out


def emd_yardstick(x1, x2):
    """-> (truth dict, cost deviation, residual deviation): the largest |variant - truth| over the four float32 variants, for the
    cost and for the residuals."""
    truth = emd_ref(x1, x2)
    dev_c = dev_r = 0.0
    for order, exp in VARIANTS:
        v = emd_ref(x1, x2, np.float32, order, exp)
        dev_c = max(dev_c, abs(v["cost"] - truth["cost"]))
        dev_r = max(dev_r, abs(v["residual"][0] - truth["residual"][0]), abs(v["residual"][1] - truth["residual"][1]))
    return truth, dev_c, dev_r


def chamfer_ref(x, y, dtype=np.float64):
    """-> dict min_d2_x, nn_x, min_d2_y, nn_y (squared distances in dtype, first index on ties), x_to_y, y_to_x, bi (float64)."""
    dtype = np.dtype(dtype).type
    d = _dist2(x, y, dtype)
    nn_x, nn_y = d.argmin(axis=1), d.argmin(axis=0)
    dx, dy = d[np.arange(d.shape[0]), nn_x], d[nn_y, np.arange(d.shape[1])]
    x_to_y, y_to_x = float(np.sqrt(dx.astype(np.float64)).mean()), float(np.sqrt(dy.astype(np.float64)).mean())
    return dict(min_d2_x=dx, nn_x=nn_x.astype(np.int32), min_d2_y=dy, nn_y=nn_y.astype(np.int32), x_to_y=x_to_y, y_to_x=y_to_x,
                bi=y_to_x + x_to_y)


HAND_P1 = np.array([[1.7, -0.1, 0.1], [0.1, 1.2, 0.3]], dtype=np.float32)   # PyTorchEMD/test_emd_loss.py
HAND_P2 = np.array([[0.3, 1.8, 0.2], [1.2, -0.2, 0.3]], dtype=np.float32)
HAND_EMD = 0.355                                                            # its hand-computed 0.71 / 2 per batch item


def wall(seed=7):
    """A 50 x 50 wall patch on a 2 cm grid and a 45 x 47 patch of it with 4 mm noise and a 1 cm shift: 2 500 and 2 115 points."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(50) * 0.02, np.arange(50) * 0.02, indexing="ij")
    a = np.stack([u.ravel(), v.ravel(), np.full(2500, 0.9)], axis=1)
    u, v = np.meshgrid(np.arange(45) * 0.02 + 0.04, np.arange(47) * 0.02 + 0.02, indexing="ij")
    b = np.stack([u.ravel(), v.ravel(), np.full(45 * 47, 0.9)], axis=1) + rng.normal(0.0, 0.004, (45 * 47, 3)) + [0.01, 0.0, 0.0]
    return a.astype(np.float32), b.astype(np.float32)


def cases():
    """name -> (x1 [n,3], x2 [m,3]) float32: the smallest shapes at which tiling, tails and the multipliers can go wrong."""
    out = {}
    rng = np.random.default_rng(20240607)
    out["hand_2_2"] = (HAND_P1, HAND_P2)
    for n, m in [(1, 1), (5, 3), (3, 5), (64, 64), (65, 63), (255, 257), (256, 256), (257, 255)]:
        out[f"uniform_{n}_{m}"] = (rng.random((n, 3), dtype=np.float32), rng.random((m, 3), dtype=np.float32))
    for n, m in [(513, 1025), (1025, 513)]:
        out[f"gauss_{n}_{m}"] = (rng.normal(0.0, 1.0, (n, 3)).astype(np.float32),
                                 (rng.normal(0.0, 1.0, (m, 3)) + [0.2, 0.0, 0.0]).astype(np.float32))
    a, b = wall()
    out["wall_2500_2115"] = (a, b)
    out["wall_2115_2500"] = (b, a)
    out["wall_self"] = (a, a.copy())
    p = rng.random((257, 3), dtype=np.float32)
    out["reversed_257"] = (p, p[::-1].copy())
    return out


SELF_CASES = ("wall_self", "reversed_257")
