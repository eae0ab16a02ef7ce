"""Host model (numpy, float64) of the exact tile binning, OLSR_BINNING_ELLIPSE: which (Gaussian, tile) instances exist.

The product decides that in four functions of csrc/olsr_device.h - cull_threshold, cull_setup, cull_rows, cull_row_span - in
fp32 interval arithmetic with outward pads.  This module restates WHAT they decide, not how: from the fp32 values the
composite and the emission see (means2D, conic_opacity, radii, W, H, the tile edge) it computes, per Gaussian and per tile
row of the reference's rect, three sets of pairs, each a contiguous range of tile columns:

  rect  every tile of get_rect (restated below in the reference's fp32 operation order): the bounding-square lists.
  core  the kernel's own definition, evaluated exactly and without any pad.  t2 is cull_threshold's formula in float64, its
        margins included; the band of tile row ty is the continuous range [ty T, min(ty T + T - 1, H - 1)]; the x-projection
        of {q(d) <= t2} n band, q(d) = a dx^2 + 2 b dx dy + c dy^2, is one interval [px + lo, px + hi]; a tile column is hit
        when the interval contains an integer pixel column of the tile that is <= W - 1.  Every instance the exact lists
        may ever drop lies outside core; the composite's own alpha test passes only inside it (t2's margins).
  may   the same with t2 (1 + 1e-5) and with the band and the column interval widened by p pixels on both ends.  Every
        instance the exact lists may ever hold lies inside may.
  full  Gaussians outside cull_setup's `exact` gate (restated in `gate`) and NaN inputs keep the whole rect: core = may = rect.

t2 < 0 (cull_threshold: no pixel can pass) gives no pair.  Nothing is sampled: on the band the upper boundary of the
ellipse, dx = (-b dy + sqrt(a t2 - det dy^2)) / a, is concave in dy, so its largest value over the band is the rightmost
point (xstar, at dy = ystar) when the band holds it and else lies on the band edge nearer to it; the lower boundary
likewise.  min_q_box gives the smallest q over a box of pixels in the other closed form (the clamped centre, then the four
edges' 1-D quadratics); tests/test_tile_cull_model_cpu.py holds the two against each other.

p, from the pads of olsr_device.h.  The kernel computes the same interval from padded fp32 quantities:
  relative to the ellipse (they scale it about its centre):  t2 in fp32 (five roundings and __logf) and its 1 + 1e-6;
    A = a t2 (1 + 4e-7);  det_lo = det (1 - 4e-7) after Kahan's 2 ulp, once more (1 - 4e-7) in the discriminants, + 2e-7 A;
    sqrt (1 + 4e-7);  m = 1e-6 (|b dy| + s) / a, at most 2e-6 of the half-extent;  xstar and ymax (1 + 1e-6) (1 + 4e-7)^1/2.
    On the level of q these add up to less than 3e-6, on lengths to 1.5e-6, plus 4e-7 + 2e-6 + 1e-6 for the sqrt, m and
    the star points: under 5e-6 of the half-extent, which is what t2 (1 + 1e-5) gives.
  in y:  pad_y = 1e-3 + 2e-7 (|py| + y_hi) widens the band, and pad_s = 1e-3 + 1e-5 |ystar| widens it once more for the two
    star clauses;  |ystar| < ymax <= half-extent and y_hi <= H - 1.  cull_rows' pad (1e-2 + 4e-7 (|py| + ymax)) only selects
    rows whose span cull_row_span then evaluates: it adds nothing to the lists.
  in x:  pad_x = 1e-3 + 2e-7 (|px| + max(|hi|, |lo|)).
  The pads exist to cover the fp32 roundings of the very expressions they pad (6e-8 per operation on |px| + half-extent,
  |py| + half-extent), so pads plus roundings stay below
      p = 2.5e-3 + 1e-6 (|px| + |py| + W + H) + 1e-5 half-extent        [pixels],   half-extent = max(xstar, ymax),
  2e-3 of it absolute (pad_y + pad_s; pad_x alone is 1e-3).  That is below 0.02 + 1e-5 (|px| + |py| + half-extent) for every
  image narrower than 17 500 pixels.  The bound was derived before any test ran and is not tuned.
"""
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64
T2_WIDEN = 1.0 + 1e-5
INT_MAX, INT_MIN = 2147483647, -2147483648

Model = namedtuple("Model", "P gx gy rect core may full none t2 p row_g row_ty row_core row_may row_rect star_only")


def _f2i_sat(v):
    """float -> int, truncating and saturating, NaN -> 0 (f2i_sat, olsr_device.h)"""
    v = np.asarray(v, dtype=F32)
    out = np.zeros(v.shape, dtype=np.int64)
    ok = ~np.isnan(v)
    hi, lo = ok & (v >= F32(2147483648.0)), ok & (v <= F32(-2147483648.0))
    mid = ok & ~hi & ~lo
    out[hi], out[lo] = INT_MAX, INT_MIN
    out[mid] = np.trunc(v[mid]).astype(np.int64)
    return out


def get_rect(means2D, radii, W, H, T):
    """(x0, y0, x1, y1) per Gaussian: get_rect of olsr_device.h (CR/auxiliary.h:41-61) in its fp32 operation order - the upper
    bound is ((p + radius) + T) - 1, three operations.  A Gaussian without a radius has an empty rect."""
    m = np.asarray(means2D, dtype=F32).reshape(-1, 2)
    r = np.asarray(radii).astype(F32)
    gx, gy = (W + T - 1) // T, (H + T - 1) // T
    t = F32(T)
    with np.errstate(invalid="ignore", over="ignore"):
        x0 = np.clip(_f2i_sat((m[:, 0] - r) / t), 0, gx)
        y0 = np.clip(_f2i_sat((m[:, 1] - r) / t), 0, gy)
        x1 = np.clip(_f2i_sat((((m[:, 0] + r) + t) - F32(1.0)) / t), 0, gx)
        y1 = np.clip(_f2i_sat((((m[:, 1] + r) + t) - F32(1.0)) / t), 0, gy)
    dead = np.asarray(radii) <= 0
    x1[dead], y1[dead] = x0[dead], y0[dead]
    return x0, y0, x1, y1


def threshold(conic_opacity, radii, T):
    """cull_threshold in float64: t2 = 2 (L + 2e-3 + 1e-4 |L| + 5e-7 (|a| + |b| + |c|) D^2) (1 + 1e-6), L = ln(255 opacity),
    D = radius + T + 1.  Returns (t2, none, nan): `none` where no pixel can pass (255 opacity not above 0, or the sum
    negative), `nan` where the conic or the opacity is not a number (the whole rect is kept)."""
    co = np.asarray(conic_opacity, dtype=F64).reshape(-1, 4)
    a, b, c, op = co.T
    nan = np.isnan(a) | np.isnan(b) | np.isnan(c) | np.isnan(op)
    o255 = 255.0 * op
    pos = o255 > 0.0
    with np.errstate(all="ignore"):
        L = np.log(np.where(pos, o255, 1.0))
        D = np.asarray(radii, dtype=F64) + float(T) + 1.0
        thr = L + 2e-3 + 1e-4 * np.abs(L) + 5e-7 * (np.abs(a) + np.abs(c) + np.abs(b)) * D * D
        nan = nan | (pos & np.isnan(thr))
        none = ~nan & (~pos | ~(thr >= 0.0))
        t2 = 2.0 * thr * (1.0 + 1e-6)
    t2 = np.where(none, -1.0, np.where(nan, np.inf, t2))
    return t2, none, nan


def opacity_for_t2(t2, conic_opacity, radii, T):
    """The inverse of `threshold` in the opacity: the float32 opacity whose t2 is the wanted one (to an ulp of the opacity).
    Scenes place the kernel's own contour with it."""
    co = np.asarray(conic_opacity, dtype=F64).reshape(-1, 4)
    a, b, c = co[:, 0], co[:, 1], co[:, 2]
    D = np.asarray(radii, dtype=F64) + float(T) + 1.0
    k = 2e-3 + 5e-7 * (np.abs(a) + np.abs(c) + np.abs(b)) * D * D
    rest = np.asarray(t2, dtype=F64) / (2.0 * (1.0 + 1e-6)) - k      # L + 1e-4 |L|
    L = np.where(rest >= 0.0, rest / (1.0 + 1e-4), rest / (1.0 - 1e-4))
    return (np.exp(L) / 255.0).astype(F32)


def gate(means2D, conic_opacity, radii, t2, nan):
    """True where cull_setup's `exact` does NOT hold: every row keeps its full rect span.  exact = det_lo > 0 and a, c in
    (1e-30, 1e6) and 0 <= t2 < 1e6 and radius < 2^20 and |px|, |py| < 1e7, every comparison false for a NaN.  det_lo is
    a c - b^2 by Kahan's fused difference (2 ulp), times 1 - 4e-7: it has the sign of the exact a c - b^2, which float64 gives
    exactly enough for fp32 inputs (both products are exact)."""
    m = np.asarray(means2D, dtype=F64).reshape(-1, 2)
    co = np.asarray(conic_opacity, dtype=F64).reshape(-1, 4)
    a, b, c = co[:, 0], co[:, 1], co[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        det = a * c - b * b
        exact = ((det > 0.0) & (a > 1e-30) & (c > 1e-30) & (t2 >= 0.0) & (t2 < 1e6) & (a < 1e6) & (c < 1e6) &
                 (np.asarray(radii) < (1 << 20)) & (np.abs(m[:, 0]) < 1e7) & (np.abs(m[:, 1]) < 1e7))
    return ~exact | nan


def _row_spans(px, py, a, b, c, det, t2, ty, x0, x1, W, H, T, p):
    """Tile columns [xa, xb) of tile row ty, per element; p widens the band and the column interval (0: core).  Also
    star_only: both band-edge discriminants negative, the span exists through the rightmost / leftmost point alone."""
    y_lo = (ty * T).astype(F64)
    y_hi = np.minimum(ty * T + T - 1, H - 1).astype(F64)
    dy0, dy1 = (y_lo - py) - p, (y_hi - py) + p
    ymax = np.sqrt(a * t2 / det)
    xstar = np.sqrt(t2 * c / det)
    ystar = -b / c * xstar
    cl0, cl1 = np.maximum(dy0, -ymax), np.minimum(dy1, ymax)
    reach = cl0 <= cl1

    def chord(dy):
        s = np.sqrt(np.maximum(a * t2 - det * dy * dy, 0.0))
        return (-s - b * dy) / a, (s - b * dy) / a
    l0, h0 = chord(cl0)
    l1, h1 = chord(cl1)
    hi = np.where((cl0 <= ystar) & (ystar <= cl1), xstar, np.maximum(h0, h1))
    lo = np.where((cl0 <= -ystar) & (-ystar <= cl1), -xstar, np.minimum(l0, l1))
    Xlo = np.maximum(np.ceil(px + lo - p), 0.0)
    Xhi = np.minimum(np.floor(px + hi + p), float(W - 1))
    hit = reach & (Xlo <= Xhi)
    Xlo, Xhi = np.where(hit, Xlo, 0.0), np.where(hit, Xhi, 0.0)
    xa = np.maximum(x0, Xlo.astype(np.int64) // T)
    xb = np.minimum(x1, Xhi.astype(np.int64) // T + 1)
    xb = np.where(hit, np.maximum(xb, xa), xa)
    star_only = hit & (dy0 < -ymax) & (dy1 > ymax)
    return xa, xb, star_only


def _pairs(g, ty, xa, xb, gx, P):
    n = (xb - xa).astype(np.int64)
    tot = int(n.sum())
    if tot == 0:
        return np.zeros(0, dtype=np.int64)
    first = np.repeat(np.cumsum(n) - n, n)
    tx = np.repeat(xa, n) + (np.arange(tot) - first)
    return np.sort((np.repeat(ty, n) * gx + tx) * max(P, 1) + np.repeat(g, n))


def model(means2D, conic_opacity, radii, W, H, T):
    """The three sets for one frame.  Keys are tile * P + Gaussian (tests/parity_common.py: tile_pairs), sorted.  Per
    (Gaussian, tile row) of the rect: row_g, row_ty and the column ranges row_rect / row_core / row_may as [n, 2] arrays."""
    m = np.asarray(means2D, dtype=F32).reshape(-1, 2).astype(F64)
    co = np.asarray(conic_opacity, dtype=F32).reshape(-1, 4).astype(F64)
    rad = np.asarray(radii).astype(np.int64)
    P = rad.shape[0]
    gx, gy = (W + T - 1) // T, (H + T - 1) // T
    x0, y0, x1, y1 = get_rect(means2D, radii, W, H, T)
    t2, none, nan = threshold(co, rad, T)
    none = none & (rad > 0)
    full = gate(m, co, rad, t2, nan) & ~none & (rad > 0)
    nrow = np.where(rad > 0, y1 - y0, 0)
    g = np.repeat(np.arange(P), nrow)
    ty = np.repeat(y0, nrow) + (np.arange(int(nrow.sum())) - np.repeat(np.cumsum(nrow) - nrow, nrow))
    rx0, rx1 = x0[g], x1[g]
    a, b, c = co[g, 0], co[g, 1], co[g, 2]
    px, py = m[g, 0], m[g, 1]
    with np.errstate(all="ignore"):
        det = a * c - b * b
        ext = np.maximum(np.sqrt(t2 * T2_WIDEN * co[:, 2] / (co[:, 0] * co[:, 2] - co[:, 1] ** 2)),
                         np.sqrt(t2 * T2_WIDEN * co[:, 0] / (co[:, 0] * co[:, 2] - co[:, 1] ** 2)))
        p = 2.5e-3 + 1e-6 * (np.abs(m[:, 0]) + np.abs(m[:, 1]) + W + H) + 1e-5 * ext
        ca, cb, star = _row_spans(px, py, a, b, c, det, t2[g], ty, rx0, rx1, W, H, T, 0.0)
        ma, mb, _ = _row_spans(px, py, a, b, c, det, t2[g] * T2_WIDEN, ty, rx0, rx1, W, H, T, p[g])
    fg, ng = full[g], none[g]
    ca, cb = np.where(fg, rx0, ca), np.where(fg, rx1, np.where(ng, ca, cb))
    ma, mb = np.where(fg, rx0, ma), np.where(fg, rx1, np.where(ng, ma, mb))
    star = star & ~fg & ~ng
    return Model(P, gx, gy, _pairs(g, ty, rx0, rx1, gx, P), _pairs(g, ty, ca, cb, gx, P), _pairs(g, ty, ma, mb, gx, P),
                 full, none, t2, np.where(full | none | (rad <= 0), 0.0, p), g, ty, np.stack([ca, cb], 1), np.stack([ma, mb], 1),
                 np.stack([rx0, rx1], 1), star)


def min_q_box(px, py, a, b, c, X0, X1, Y0, Y1):
    """The smallest q(d) over the box [X0, X1] x [Y0, Y1] of positions, d = position - (px, py), for a positive definite
    conic: zero when the box holds the centre, else the least of the four edges' 1-D quadratics, each at its clamped
    vertex."""
    px, py, a, b, c, X0, X1, Y0, Y1 = (np.asarray(v, dtype=F64) for v in (px, py, a, b, c, X0, X1, Y0, Y1))
    u0, u1, v0, v1 = X0 - px, X1 - px, Y0 - py, Y1 - py
    inside = (u0 <= 0) & (0 <= u1) & (v0 <= 0) & (0 <= v1)

    def q(u, v):
        return a * u * u + 2.0 * b * u * v + c * v * v
    best = np.full(np.broadcast(px, X0).shape, np.inf)
    for u in (u0, u1):                       # vertical edges: minimise over v
        v = np.clip(-b * u / c, v0, v1)
        best = np.minimum(best, q(u, v))
    for v in (v0, v1):                       # horizontal edges: minimise over u
        u = np.clip(-b * v / a, u0, u1)
        best = np.minimum(best, q(u, v))
    return np.where(inside, 0.0, best)


def split_key(keys, P):
    keys = np.asarray(keys, dtype=np.int64)
    return keys // max(P, 1), keys % max(P, 1)


def is_subset(a, b):
    """every key of a is a key of b (both unique)"""
    return bool(np.isin(a, b, assume_unique=True).all())
