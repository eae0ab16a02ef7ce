"""tests/act_ref.py against the float64 truth, on a CPU: the float32 restatement of the three OLSR_ACT_* backward chains —
what tests/test_gpu_activations.py holds the kernels to bit for bit — is itself within its rounding bound of autograd in double,
on random rows and on the edge rows both suites plant.  u = 2^-24 is float32's unit roundoff, every operation rounds once,
(1 + u / (1 + u))^k <= 1 + k u for the k <= 3 roundings in a row below, and a rounding whose result is subnormal errs by at
most 2^-150 instead (act_ref.TINY; it matters only for the smallest planted scale)."""
import numpy as np
import pytest
import torch

import act_ref as A

F32 = np.float32
N_RANDOM = 20000


def _cases():
    """Raw parameters (random rows, then the edge rows) and random gradients with respect to the activated values."""
    e = A.edge_rows()
    op, sc, rot = A.random_raw(N_RANDOM, seed=77)
    op, sc, rot = (np.concatenate([a, b]) for a, b in ((op, e["opacities"]), (sc, e["scales"]), (rot, e["rotations"])))
    g = torch.Generator().manual_seed(78)
    P = op.shape[0]
    # (gradients over six decades, both signs, some exact zeros)
    mag = lambda *s: (torch.randn(*s, generator=g) * torch.exp(3.0 * torch.randn(*s, generator=g)) * 1e-5).numpy()  # noqa: E731
    g_op, g_sc, g_rot = mag(P), mag(P, 3), mag(P, 4)
    for a in (g_op, g_sc, g_rot):
        a[::97] = 0.0
    return e, op, sc, rot, g_op, g_sc, g_rot


def test_edge_rows_are_what_the_issue_lists():
    e = A.edge_rows()
    E = len(e["names"])
    assert E == 21 and len(set(e["names"])) == E
    op = e["opacities"].reshape(-1)
    floor = F32(-np.log(254.0))
    for x in (0.0, floor, np.nextafter(floor, F32(-9)), np.nextafter(floor, F32(9)), 16.6, 17.4, 20.0, -20.0, -90.0):
        assert int((op == F32(x)).sum()) >= 1, x
    assert int(((op == 0) & np.signbit(op)).sum()) == 1 and int(((op == 0) & ~np.signbit(op)).sum()) == 1
    o, _ = A.activate64(op, e["scales"])
    # the sigmoid of 17.4 is 1 in float32 and that of -90 is 0: the chain is exactly 0 there; the floor row sits on 1 / 255
    assert o[op == F32(17.4)][0] == 1.0 and o[op == F32(-90.0)][0] == 0.0 and 0 < o[op == F32(16.6)][0] < 1
    assert abs(float(o[op == floor][0]) - 1 / 255) < 4 * 2.0 ** -31   # (a few float32 spacings)
    sc = e["scales"]
    assert int((sc == 0).all(1).sum()) == 1 and int((sc == F32(A.LOG_SCALE_MIN)).all(1).sum()) == 1
    assert int((sc == F32(A.LOG_SCALE_MAX)).all(1).sum()) == 1
    assert int((np.abs((sc.max(1) - sc.min(1)) - 8.0) < 1e-6).sum()) == 1
    q = e["rotations"].astype(np.float64)
    n = np.sqrt((q * q).sum(1))
    for want in (1.0, 5.0, 7.0, 3.0, 0.0):
        assert int((n == want).sum()) >= 1, want
    assert int((np.abs(n - 1e-3) < 1e-9).sum()) == 1 and int((np.abs(n - 1e3) < 1e-3).sum()) == 1
    assert int(((q != 0).sum(1) == 1).sum()) == 1
    assert int(e["clamp"].sum()) == A.N_CLAMP_PLANTED
    # in front of the camera, near the image centre (fx = 80, 160 x 120)
    m = e["means3D"]
    assert ((m[:, 2] > 0.2) & (m[:, 2] < 0.3)).all() and (np.abs(80 * m[:, 0] / m[:, 2]) < 30).all() and (np.abs(80 * m[:, 1] / m[:, 2]) < 30).all()


def test_opacity_chain_is_within_three_roundings_of_float64():
    """g * (o * (1 - o)) with o the float32 activated opacity: 1 - o, the product with o and the product with g round once
    each, nothing else is inexact (o is the truth's own argument).  Bound: 3 x 2^-24 of the element (+ 3 x 2^-150)."""
    e, op, sc, rot, g_op, _, _ = _cases()
    o, _ = A.activate64(op, sc)
    got = A.opacity_chain(g_op, o)
    truth = A.opacity_truth(g_op, o)
    assert np.isfinite(truth).all() and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - truth)
    assert (err <= A.opacity_bound(truth)).all(), float((err / A.opacity_bound(truth)).max())
    assert (got[o.reshape(-1) == 1.0] == 0).all() and (got[o.reshape(-1) == 0.0] == 0).all()
    assert (np.count_nonzero(got) > 0.9 * got.size)


def test_scale_chain_is_within_one_rounding_of_float64():
    """g_k * s_k with s_k the float32 activated scale: one rounding.  Bound: 2^-24 of the element (+ 2^-150: the smallest
    planted scale, 1.6e-38, takes the product into the subnormal range)."""
    e, op, sc, rot, _, g_sc, _ = _cases()
    _, s = A.activate64(op, sc)
    got = A.scale_chain(g_sc, s)
    truth = A.scale_truth(g_sc, s)
    assert np.isfinite(truth).all() and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - truth)
    assert (err <= A.scale_bound(truth)).all(), float((err / A.scale_bound(truth)).max())


def test_rotation_chain_is_within_its_condition_of_float64():
    """n = max(sqrt(((q0^2 + q1^2) + q2^2) + q3^2), 1e-12), h = q / n, dot = ((h0 g0 + h1 g1) + h2 g2) + h3 g3,
    out_k = (g_k - h_k dot) / n.  To first order in u = 2^-24:
      the sum under the root: each (positive) term is squared (1) and passes at most 3 additions      -> 4 u
      n: half of that, and the root's own rounding                                                      -> 3 u
      h_k = q_k / n                                                                                     -> 4 u   (K_ROT_FWD)
      h_j g_j: 5 u each; through at most 3 additions: dot is off by                                     8 u S,  S = sum |h_j g_j|
      h_k dot: h_k (4 u) and the product (1 u) on |h_k dot| <= |h_k| S, and dot's own error             -> 13 u |h_k| S
      g_k - h_k dot: one rounding of at most |g_k| + |h_k| S                                            -> u (|g_k| + |h_k| S)
      the division by n: n (3 u) and its own rounding (1 u) on the quotient                            -> 4 u (|g_k| + |h_k| S) / n
    Sum: at most 18 x 2^-24 x (|g_k| + |h_k| S) / n (K_ROT_BWD; the element itself may be far smaller than this condition:
    g is nearly parallel to h in places).  The planted zero quaternion is left out — the clamp decides there and F.normalize
    in double divides by the same 1e-12 while float32's 1e-12 is another number — and nothing else is."""
    e, op, sc, rot, _, _, g_rot = _cases()
    clamp = A.clamp_active(rot)
    assert int(clamp.sum()) == A.N_CLAMP_PLANTED and clamp[N_RANDOM:].sum() == A.N_CLAMP_PLANTED
    got_h, got = A.normalize_forward(rot), A.rotation_chain(g_rot, rot)
    h64, truth = A.rotation_truth(g_rot, rot)
    finite = np.isfinite(truth).all(1) & np.isfinite(h64).all(1)
    assert finite.all()                                   # (no planted row's float64 chain is non-finite)
    keep = ~clamp
    assert int(keep.sum()) == rot.shape[0] - A.N_CLAMP_PLANTED
    err_h = np.abs(got_h.astype(np.float64) - h64)[keep]
    assert (err_h <= A.K_ROT_FWD * A.U * np.abs(h64[keep])).all(), float((err_h / (A.U * np.abs(h64[keep]) + 1e-300)).max())
    err = np.abs(got.astype(np.float64) - truth)[keep]
    bound = A.rotation_bound(g_rot, rot)[keep]
    assert (err <= bound).all(), float((err / bound).max())
    # the clamped row: held to the restatement's own definition, g / 1e-12f
    z = np.flatnonzero(clamp)[0]
    assert (got_h[z] == 0).all() and A.same_bits(got[z], g_rot[z] / A.EPS_NORM)
    # exact cases: norms 5 and 7 are exact in float32, so h is q / 5 and q / 7 rounded once
    for q, n in (((1, 2, 2, 4), 5.0), ((2, 3, 6, 0), 7.0)):
        h = A.normalize_forward(np.array([q], F32))
        assert A.same_bits(h, (np.array([q], F32) / F32(n)))


def test_restatement_rounds_every_operation_once():
    """The restatement must stay in float32 throughout (a float64 intermediate would round twice): hand-rounded steps."""
    g, o = F32(3e-6), F32(0.7310586)
    one_minus = F32(np.float64(1.0) - np.float64(o))
    prod = F32(np.float64(o) * np.float64(one_minus))
    assert A.opacity_chain(np.array([g]), np.array([o]))[0] == F32(np.float64(g) * np.float64(prod))
    q = np.array([[0.3, -1.1, 0.7, 0.2]], F32)
    gq = np.array([[1e-3, 2e-3, -4e-3, 5e-4]], F32)
    d = lambda x: np.float64(x)  # noqa: E731
    sq = [F32(d(v) * d(v)) for v in q[0]]
    s = F32(d(F32(d(F32(d(sq[0]) + d(sq[1]))) + d(sq[2]))) + d(sq[3]))
    n = F32(np.sqrt(d(s)))
    h = [F32(d(v) / d(n)) for v in q[0]]
    pr = [F32(d(h[k]) * d(gq[0, k])) for k in range(4)]
    dot = F32(d(F32(d(F32(d(pr[0]) + d(pr[1]))) + d(pr[2]))) + d(pr[3]))
    want = [F32(d(F32(d(gq[0, k]) - d(F32(d(h[k]) * d(dot))))) / d(n)) for k in range(4)]
    assert A.same_bits(A.rotation_chain(gq, q), np.array([want], F32))
    assert A.same_bits(A.normalize_forward(q), np.array([h], F32))


def test_same_bits_semantics():
    nan = F32("nan")
    assert A.same_bits(np.array([0.0, nan, 1.0], F32), np.array([-0.0, nan, 1.0], F32))
    assert not A.same_bits(np.array([1.0], F32), np.array([np.nextafter(F32(1), F32(2))], F32))
    assert not A.same_bits(np.array([nan], F32), np.array([0.0], F32))
    assert A.ulp_error(np.array([1.0], F32), np.array([1.0 + 2.0 ** -23]))[0] == pytest.approx(1.0)
