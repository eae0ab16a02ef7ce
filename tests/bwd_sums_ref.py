"""Host model (numpy, float32) of every float sum the per-Gaussian backward makes across rows and across Gaussians
(csrc/k_preprocess_bwd.hip): the row sums that turn the composite's partial-gradient rows into the six composite-level
tensors, and the reduction of dL_dtau to dL_dtau_sum.  The kernels call these sums "fixed order, bit-reproducible"; this
module writes the order down, addition by addition, so that the outputs can be held to EQUALITY on data the same call leaves
readable (tests/test_gpu_bwd_sums.py, parity_common.assert_tau_sum_fixed_order).

Every addition below is a float32 numpy addition of two arrays, in the order the kernels make it.  Nothing here uses np.sum,
np.add.reduce or reduceat (numpy sums pairwise): the model is vectorised ACROSS Gaussians and sequential WITHIN one.
No torch.cuda, no GPU: tests/test_bwd_sums_ref_cpu.py checks the model against float64 and against other orders.
"""
import math

import numpy as np

F32 = np.float32
MID_FOOTPRINT = 12   # OLSR_MID_FOOTPRINT (csrc/olsr_kernels.h): more tiles than this -> row_reduce_big_kernel, a wave per Gaussian
BIG_FOOTPRINT = 32   # OLSR_BIG_FOOTPRINT: splits the two work lists of big_list
PB_THREADS = 128     # Gaussians per block of preprocess_bwd_kernel = per tau partial
TAU_T = 256          # threads of tau_final_kernel
_LANE = np.arange(64)
EPS = 2.0 ** -24     # unit roundoff of float32


def grad_row(F):
    """floats per partial-gradient row (olsr_device.h): ten composite-level values and F language channels, padded to 4"""
    return (10 + F + 3) // 4 * 4


def rr_nwaves(P):
    """waves of row_reduce_big_kernel's persistent grid (launch_pb_t): four per block, min(8192, max(256, P / 16)) blocks"""
    return 4 * min(8192, max(256, P // 16))


def _f32(a):
    a = np.asarray(a)
    if a.dtype != F32:
        raise TypeError(f"the model adds float32 values, got {a.dtype}")
    return a


def wave_tree(v):
    """The xor butterfly over the 64 lanes of a wave, on the last axis: for m in 32, 16, 8, 4, 2, 1: v = v + v[lane ^ m].
    Returns all 64 lanes (they are equal: float addition is commutative, so lane l and lane l ^ m compute the same bits at
    every level).

    This is wave_sum of csrc/olsr_collectives.h as written.  It is also the tree of wave_reduce_rec (the multi-value
    butterfly of row_reduce_big_kernel): there, at the level with mask m, a lane keeps one half of its values and adds what
    lane ^ m sends of the same value, keep + send where wave_sum has own + other - for the lane that keeps value i that IS
    own + other, and for its partner it is other + own, the same bits by commutativity.  Which lanes end up holding which
    value (lane = value * G_LANES) and how many levels halve the value count (log2 of next_pow2(10 + F)) decide where a sum
    lies, not what it is; the levels run 32, 16, ..., 1 for every value in both forms."""
    v = _f32(v)
    assert v.shape[-1] == 64
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ m]
    return v


def _rows2d(rows):
    rows = _f32(rows)
    assert rows.ndim == 2
    return rows


def inline_row_sum(rows, first, nrows):
    """preprocess_bwd_kernel's own sum (at most OLSR_MID_FOOTPRINT tiles): acc = +0.0, then acc += rows[first + t] for
    t = 0 .. nrows - 1.  rows [L, row_floats] float32; first, nrows [N]; returns [N, row_floats]."""
    rows = _rows2d(rows)
    first, nrows = np.asarray(first, dtype=np.int64), np.asarray(nrows, dtype=np.int64)
    acc = np.zeros((first.shape[0], rows.shape[1]), dtype=F32)
    for t in range(int(nrows.max()) if nrows.size else 0):
        sel = np.nonzero(nrows > t)[0]
        acc[sel] = acc[sel] + rows[first[sel] + t]
    return acc


def wave_row_sum(rows, first, nrows):
    """row_reduce_big_kernel's sum (more than OLSR_MID_FOOTPRINT tiles), a wave per Gaussian: lane l holds +0.0 and adds rows
    first + l, first + l + 64, ... in that order; then wave_tree over the lanes, per value.  Shapes as inline_row_sum."""
    rows = _rows2d(rows)
    first, nrows = np.asarray(first, dtype=np.int64), np.asarray(nrows, dtype=np.int64)
    N, ROW = first.shape[0], rows.shape[1]
    lanes = np.zeros((N, 64, ROW), dtype=F32)
    for k in range((int(nrows.max()) + 63) // 64 if nrows.size else 0):
        t = 64 * k + _LANE[None, :]                                   # [1, 64]
        g, l = np.nonzero(t < nrows[:, None])
        lanes[g, l] = lanes[g, l] + rows[first[g] + 64 * k + l]
    return wave_tree(np.ascontiguousarray(lanes.transpose(0, 2, 1)))[..., 0]


def composite_level(rows, row_floats, F_rows, F_out, P, radii, blended, tiles_touched, inst_start, rowbase, *,
                    activations=0, conic_opacity=None):
    """preprocess_bwd_kernel up to the six composite-level tensors, restated on what the call leaves readable.

    rows          the compacted partial-gradient rows, flat float32 (at least live rows * row_floats values)
    row_floats    floats per row; must be grad_row(F_rows)
    F_rows, F_out language channels of the rows / of the scene (F_rows == 0 < F_out: no language cotangent)
    radii, blended, tiles_touched, inst_start [P]; rowbase [R + 1]: emission index -> first compact row

    ntiles = tiles_touched if radii > 0 and blended != 0 else 0; the Gaussian's rows are the run
    [rowbase[u0], rowbase[u0 + ntiles]) with u0 = inst_start[idx]; ntiles > 12: wave_row_sum, 1 .. 12: inline_row_sum, 0 or
    an empty run: zeros.  Values 0..9 and 10..10 + F_rows of a row go to the tensors in the kernel's layout.
    Returns a dict of the six tensors (float32 numpy) and `has_rows` [P] bool.

    Only for activations == 0 (the sigmoid's derivative would scale dL_dopacity) and finite conics (a NaN conic overwrites
    values 0..5 with NaN): anything else is refused."""
    if activations != 0:
        raise ValueError("composite_level models activations == 0 only")
    if conic_opacity is not None and not bool(np.isfinite(np.asarray(conic_opacity, dtype=np.float64)).all()):
        raise ValueError("composite_level models finite conics only")
    if row_floats != grad_row(F_rows):
        raise ValueError(f"rows of {row_floats} floats are not grad_row({F_rows}) = {grad_row(F_rows)}")
    if F_rows not in (0, F_out):
        raise ValueError("the rows carry either no language channel or the scene's")
    rows = _f32(rows).reshape(-1)
    radii, blended = np.asarray(radii).astype(np.int64), np.asarray(blended).astype(np.int64)
    tt, u0 = np.asarray(tiles_touched).astype(np.int64), np.asarray(inst_start).astype(np.int64)
    rowbase = np.asarray(rowbase).astype(np.int64)
    assert radii.shape == blended.shape == tt.shape == u0.shape == (P,)
    ntiles = np.where((radii > 0) & (blended != 0), tt, 0)
    live = ntiles > 0
    u0 = np.where(live, u0, 0)
    first = np.where(live, rowbase[u0], 0)
    nrows = np.where(live, rowbase[u0 + ntiles] - first, 0)
    assert (nrows >= 0).all()
    L = int((first + nrows).max()) if P else 0
    assert L * row_floats <= rows.size, "the runs end beyond the rows handed in"
    rows = rows[: L * row_floats].reshape(L, row_floats)
    acc = np.zeros((P, row_floats), dtype=F32)
    big = np.nonzero(ntiles > MID_FOOTPRINT)[0]
    small = np.nonzero(live & (ntiles <= MID_FOOTPRINT))[0]
    acc[big] = wave_row_sum(rows, first[big], nrows[big])
    acc[small] = inline_row_sum(rows, first[small], nrows[small])
    z = np.zeros(P, dtype=F32)
    out = dict(dL_dmeans2D=np.stack([acc[:, 0], acc[:, 1], z], 1),
               dL_dconic=np.stack([acc[:, 2], acc[:, 3], z, acc[:, 4]], 1),
               dL_dopacity=acc[:, 5:6].copy(), dL_dcolors=acc[:, 6:9].copy(), dL_ddepths=acc[:, 9:10].copy(),
               dL_dlanguage=acc[:, 10:10 + F_rows].copy() if F_rows > 0 else np.zeros((P, F_out), dtype=F32),
               has_rows=nrows > 0, nrows=nrows, ntiles=ntiles)
    return out


def densify_norm(acc0, acc1, radii):
    """the densification statistic of a view: sqrt(acc0 * acc0 + acc1 * acc1) in float32 (two products, one sum, one
    correctly rounded square root; no contraction) where radii > 0, else 0"""
    a0, a1 = _f32(acc0), _f32(acc1)
    n = np.sqrt(a0 * a0 + a1 * a1)
    return np.where(np.asarray(radii) > 0, n, F32(0.0)).astype(F32)


def tau_partials(dL_dtau):
    """[nb, 6]: the block partials of preprocess_bwd_kernel over 128 consecutive Gaussians (lanes past P hold +0.0):
    wave_tree per wave of 64, then 0 + w0 + w1."""
    x = _f32(dL_dtau).reshape(-1, 6)
    P = x.shape[0]
    nb = (P + PB_THREADS - 1) // PB_THREADS
    pad = np.zeros((nb * PB_THREADS, 6), dtype=F32)
    pad[:P] = x
    w = wave_tree(np.ascontiguousarray(pad.reshape(nb, PB_THREADS // 64, 64, 6).transpose(0, 1, 3, 2)))[..., 0]  # [nb, 2, 6]
    v = np.zeros((nb, 6), dtype=F32)
    for k in range(PB_THREADS // 64):
        v = v + w[:, k]
    return v


def tau_final(partials, threads=TAU_T, stride=TAU_T):
    """tau_final_kernel: thread t adds partials t, t + stride, ... from +0.0, wave_tree per wave, then 0 + w0 + w1 + ...
    (threads, stride: the kernel's are 256, 256 - other values are the mutants of tests/test_bwd_sums_ref_cpu.py)."""
    p = _f32(partials).reshape(-1, 6)
    nb = p.shape[0]
    acc = np.zeros((threads, 6), dtype=F32)
    t = np.arange(threads)
    k = 0
    while True:
        b = t + k * stride
        sel = np.nonzero(b < nb)[0]
        if sel.size == 0:
            break
        acc[sel] = acc[sel] + p[b[sel]]
        k += 1
    w = wave_tree(np.ascontiguousarray(acc.reshape(threads // 64, 64, 6).transpose(0, 2, 1)))[..., 0]  # [waves, 6]
    v = np.zeros(6, dtype=F32)
    for i in range(threads // 64):
        v = v + w[i]
    return v


def tau_sum(dL_dtau):
    """dL_dtau_sum [6] from dL_dtau [P, 6]: tau_partials, then tau_final."""
    return tau_final(tau_partials(dL_dtau))


def tau_sum_depth(P):
    """d of tau_sum_bound: additions on the longest path from one dL_dtau element to the result"""
    nb = (P + PB_THREADS - 1) // PB_THREADS
    return 8 + (nb + TAU_T - 1) // TAU_T + 10


def tau_sum_bound(dL_dtau):
    """(float64 sum [6], bound [6]): |tau_sum - float64 sum| <= bound = d * 2^-24 * sum |x| per component.

    d counts the additions on the longest path of the model from an input to the output:
      block partial   6 levels of wave_tree, then 0 + w0 and + w1                          8
      final, strided  thread t adds ceil(nb / 256) partials to its +0.0                    ceil(nb / 256)
      final, tree     6 levels of wave_tree, then 0 + w0, + w1, + w2, + w3                 10
    Every float32 addition returns (a + b)(1 + e) with |e| <= u = 2^-24 (no underflow error in an addition), so an input
    that passes through k rounded additions reaches the output times a factor within (1 +- u)^k, and the result differs
    from the exact sum by at most ((1 + u)^k - 1) sum |x|.  Three of the d additions on any path have +0.0 as one operand
    and are exact, so k <= d - 3, and (1 + u)^(d - 3) - 1 <= (d - 3) u / (1 - (d - 3) u) <= d u whenever d (d - 3) u <= 3,
    i.e. for every d below 7 000 (P below 2 * 10^8): the first-order form is rigorous here.  The float64 sums are
    math.fsum's (correctly rounded).  Derived, not measured."""
    x = _f32(dL_dtau).reshape(-1, 6).astype(np.float64)
    d = tau_sum_depth(x.shape[0])
    assert d * (d - 3) * EPS <= 3.0
    exact = np.array([math.fsum(x[:, c].tolist()) for c in range(6)], dtype=np.float64)
    mag = np.array([math.fsum(np.abs(x[:, c]).tolist()) for c in range(6)], dtype=np.float64)
    return exact, d * EPS * mag
