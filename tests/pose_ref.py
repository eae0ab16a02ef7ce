"""The float32 restatement of the geometry half of olsr_pose_step (csrc/k_pose.hip: pose_step_view after the Adam words), and
the cases of tests/test_gpu_pose_pinned.py.  numpy only; every operation is rounded once (no fused multiply-add, which is what
numpy's float32 scalars do and what the build's -ffp-contract=off gives), sums run left to right as the kernel's source writes
them.  Written from the reference's statements:

    SO3_exp / V with their small-angle branches (angle < 1e-5, a float32 comparison)       utils/pose_utils.py:25-58
    SE3_exp: R = SO3_exp(theta), t = V(theta) @ rho;  new_w2c = SE3_exp(tau) @ T_w2c,
    converged = |tau| < threshold (float32)                                                utils/pose_utils.py:61-93
    Camera.update_RT keeps R and T: the next T_w2c has a [0 0 0 1] last row                 utils/camera_utils.py:119-121
    world_view_transform = W2C^T, full_proj_transform = world_view_transform @ P^T,
    camera_center = world_view_transform.inverse()[3, :3] (here: -R^-1 t, R^-1 by cofactors) utils/camera_utils.py:103-117

sin(angle) and cos(angle) are ARGUMENTS of apply_tau: they are the only two operations whose float32 result a host cannot
state (they come from the device's math library).  The CPU users (oracle/pose_oracle.py, tests/window_ba_ref.py) pass
host_sincos(angle), the double sine and cosine rounded to float32; tests/test_gpu_pose_pinned.py passes candidates an ulp or so
around them.

`variant` names a deliberate mistake (MUTANTS): tests/test_pose_ref_cpu.py shows that the cases below tell every one of them
from the restatement by at least one output bit, so a kernel that made that mistake would fail the GPU test."""
import functools
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import adam_ref

f32 = np.float32
ZERO, ONE, HALF = f32(0.0), f32(1.0), f32(0.5)
SIXTH = f32(1.0) / f32(6.0)
SMALL_ANGLE = f32(1e-5)
CONVERGED_THRESHOLD = 1e-4

MUTANTS = ("small_b_0", "small_bV_0", "small_cV_0", "large_b_half", "large_cV_sixth", "large_bV_is_a", "t3_from_Rm", "branch_le",
           "branch_threshold_1e-4", "T_at_E", "last_row_kept", "campos_from_transpose", "proj_at_view", "N_sum_right_to_left",
           "converged_from_theta", "converged_le")


def _vec(x, n):
    x = np.ascontiguousarray(x, dtype=f32).reshape(-1)
    assert x.size == n
    return [f32(v) for v in x]


def angle_of(tau):
    """sqrt((tx*tx + ty*ty) + tz*tz) of theta = tau[3:6], float32."""
    tx, ty, tz = _vec(tau, 6)[3:]
    return f32(np.sqrt((tx * tx + ty * ty) + tz * tz))


def tau_norm(tau):
    """The six-term norm of the convergence test, in the kernel's order."""
    t = _vec(tau, 6)
    return f32(np.sqrt(((((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + t[3] * t[3]) + t[4] * t[4]) + t[5] * t[5]))


def takes_small_branch(angle, variant=""):
    if variant == "branch_le":
        return bool(angle <= SMALL_ANGLE)
    if variant == "branch_threshold_1e-4":
        return bool(angle < f32(1e-4))
    return bool(angle < SMALL_ANGLE)


def apply_tau(T16, tau, sin=None, cos=None, threshold=CONVERGED_THRESHOLD, variant=""):
    """new_w2c = SE3_exp(tau) @ T_w2c with the last row reset, and the convergence flag.  T16: the 16 pose words (row-major);
    tau = [rho | theta] float32; sin, cos: float32 sin(angle) and cos(angle), read only when angle >= float32(1e-5).
    Returns (float32[16], 0 or 1)."""
    T, tau = _vec(T16, 16), _vec(tau, 6)
    tx, ty, tz = tau[3], tau[4], tau[5]
    W = [ZERO, -tz, ty, tz, ZERO, -tx, -ty, tx, ZERO]
    W2 = [(W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c]) + W[3 * r + 2] * W[6 + c] for r in range(3) for c in range(3)]
    angle = f32(np.sqrt((tx * tx + ty * ty) + tz * tz))
    if takes_small_branch(angle, variant):
        a, b, bV, cV = ONE, HALF, HALF, SIXTH
        if variant == "small_b_0":
            b = ZERO
        elif variant == "small_bV_0":
            bV = ZERO
        elif variant == "small_cV_0":
            cV = ZERO
    else:
        s, co = f32(sin), f32(cos)
        a = s / angle
        b = (ONE - co) / (angle * angle)
        bV = b
        cV = (angle - s) / ((angle * angle) * angle)
        if variant == "large_b_half":
            b = HALF
        elif variant == "large_cV_sixth":
            cV = SIXTH
        elif variant == "large_bV_is_a":
            bV = a
    Rm, Vm = [], []
    for i in range(9):
        eye = ONE if i % 4 == 0 else ZERO
        Rm.append((eye + a * W[i]) + b * W2[i])
        Vm.append((eye + W[i] * bV) + W2[i] * cV)
    M = Rm if variant == "t3_from_Rm" else Vm
    t3 = [(M[3 * r] * tau[0] + M[3 * r + 1] * tau[1]) + M[3 * r + 2] * tau[2] for r in range(3)]
    E = [Rm[0], Rm[1], Rm[2], t3[0], Rm[3], Rm[4], Rm[5], t3[1], Rm[6], Rm[7], Rm[8], t3[2], ZERO, ZERO, ZERO, ONE]
    N = [ZERO] * 16
    for r in range(3):
        for c in range(4):
            if variant == "T_at_E":
                terms = [T[4 * r + k] * E[4 * k + c] for k in range(4)]
            else:
                terms = [E[4 * r + k] * T[4 * k + c] for k in range(4)]
            if variant == "N_sum_right_to_left":
                N[4 * r + c] = ((terms[3] + terms[2]) + terms[1]) + terms[0]
            else:
                N[4 * r + c] = ((terms[0] + terms[1]) + terms[2]) + terms[3]
    N[12:16] = T[12:16] if variant == "last_row_kept" else [ZERO, ZERO, ZERO, ONE]
    if variant == "converged_from_theta":
        nrm = angle
    else:
        t = tau
        nrm = f32(np.sqrt(((((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) + t[3] * t[3]) + t[4] * t[4]) + t[5] * t[5]))
    flag = int(nrm <= f32(threshold)) if variant == "converged_le" else int(nrm < f32(threshold))
    out = np.array(N, dtype=f32)
    assert all(type(v) is f32 for v in N)
    return out, flag


def derive(T16, proj, variant=""):
    """Words 16..51 of a pose state from its pose words: world_view_transform, full_proj_transform, camera_center and the
    zero pad.  proj: the projection matrix as the callers hold it ([4,4], the transpose of P)."""
    T = _vec(T16, 16)
    P = _vec(np.asarray(proj, dtype=f32).reshape(4, 4), 16)
    Vw = [T[4 * c + r] for r in range(4) for c in range(4)]
    full = []
    for r in range(4):
        for c in range(4):
            if variant == "proj_at_view":
                terms = [P[4 * r + k] * Vw[4 * k + c] for k in range(4)]
            else:
                terms = [Vw[4 * r + k] * P[4 * k + c] for k in range(4)]
            full.append(((terms[0] + terms[1]) + terms[2]) + terms[3])
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]
    t0, t1, t2 = T[3], T[7], T[11]
    if variant == "campos_from_transpose":
        i00, i01, i02, i10, i11, i12, i20, i21, i22 = r00, r10, r20, r01, r11, r21, r02, r12, r22
    else:
        c00, c01, c02 = r11 * r22 - r12 * r21, r12 * r20 - r10 * r22, r10 * r21 - r11 * r20
        det = (r00 * c00 + r01 * c01) + r02 * c02
        with np.errstate(all="ignore"):
            inv = ONE / det
        i00, i01, i02 = c00 * inv, (r02 * r21 - r01 * r22) * inv, (r01 * r12 - r02 * r11) * inv
        i10, i11, i12 = c01 * inv, (r00 * r22 - r02 * r20) * inv, (r02 * r10 - r00 * r12) * inv
        i20, i21, i22 = c02 * inv, (r01 * r20 - r00 * r21) * inv, (r00 * r11 - r01 * r10) * inv
    with np.errstate(all="ignore"):
        campos = [-((i00 * t0 + i01 * t1) + i02 * t2), -((i10 * t0 + i11 * t1) + i12 * t2), -((i20 * t0 + i21 * t1) + i22 * t2)]
    words = Vw + full + campos + [ZERO]
    assert all(type(v) is f32 for v in words)
    return np.array(words, dtype=f32)


def host_sincos(angle):
    """What a host can say: the correctly rounded float32 of the double sine and cosine of the float32 angle."""
    return f32(np.sin(np.float64(angle))), f32(np.cos(np.float64(angle)))


def shifted(x, ulps):
    """The float32 `ulps` places above (below, if negative) x."""
    x = f32(x)
    for _ in range(abs(int(ulps))):
        x = np.nextafter(x, f32(np.inf if ulps > 0 else -np.inf), dtype=f32)
    return x


def pose_step(state, status, grad_tau, grad_exposure, proj, lrs, step, threshold=CONVERGED_THRESHOLD, sincos=None, variant="",
              tau=None):
    """One olsr_pose_step with a gradient on an 80-float state and an int32[2] status; returns the new (state, status).  The Adam
    words are adam_ref.pose_step_adam's; tau: use this one instead (the tau a device run left in words 64..69)."""
    st, status = np.array(state, dtype=f32), np.array(status, dtype=np.int32)
    a = adam_ref.pose_step_adam(st, grad_tau, grad_exposure, lrs, step)
    st[52:58], st[58:64], st[64:70] = a["tau_m"], a["tau_v"], a["tau"] if tau is None else np.asarray(tau, dtype=f32)
    st[70:72], st[72:74], st[74:76] = a["exposure"], a["exposure_m"], a["exposure_v"]
    s, c = host_sincos(angle_of(st[64:70])) if sincos is None else sincos
    st[:16], flag = apply_tau(st[:16], st[64:70], s, c, threshold, variant)
    status[0], status[1] = flag, status[1] + 1
    st[16:52] = derive(st[:16], proj, variant)
    return st, status


# ---- the cases ----------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLASSES = ("zero", "small", "branch_threshold", "above", "large", "converged_threshold", "poses", "moments", "sheared", "last_row")
# the range of angle_of(tau) in every class that is defined by it
ANGLE_RANGE = {"small": (5e-8, 9.95e-6), "above": (1.05e-5, 1.1e-3), "large": (9e-3, 1.000001)}
NO_REFERENCE = ("sheared", "last_row")   # classes without a counterpart in the reference's run (tests/golden/pose_wide.npz)


@dataclass
class Case:
    name: str
    cls: str
    pose: str                 # key of start_poses()
    proj: int                 # which of pose.npz's four projection matrices
    lrs: Tuple[float, float, float]
    step: int
    grad_tau: np.ndarray      # [rho | theta]
    grad_exposure: Optional[np.ndarray]
    moments: Optional[Tuple[np.ndarray, np.ndarray]]   # preset words 52..57 and 58..63, or None = zeros
    tau: np.ndarray           # what adam_ref.pose_step_adam gives: the tau the step applies

    def state(self):
        st = np.zeros(80, dtype=f32)
        st[:16] = start_poses()[self.pose].reshape(16)
        if self.moments is not None:
            st[52:58], st[58:64] = self.moments
        st[70:72] = (0.25, -0.125)
        return st


def _rng(*key):
    return np.random.default_rng([20261021, *key])


@functools.lru_cache(maxsize=None)
def _pose_npz():
    return np.load(os.path.join(GOLDEN, "pose.npz"))


@functools.lru_cache(maxsize=None)
def projections():
    """The four projection matrices of pose.npz, C-contiguous [4,4] as the callers hold them."""
    G = _pose_npz()
    return tuple(np.ascontiguousarray(G[f"seq{s}_proj"], dtype=f32) for s in range(4))


def _rot(axis, deg):
    """Rodrigues in double."""
    axis = np.asarray(axis, dtype=np.float64)
    k = axis / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


@functools.lru_cache(maxsize=None)
def start_poses():
    """name -> [4,4] float32 T_w2c.  identity; seq0..seq3: the start poses of pose.npz; far: 170 degrees from the identity,
    |T| about 50; sheared: a 3x3 that is no rotation (determinant about 0.5), which is what separates the general inverse from a
    transpose; last_row: a state whose last row is not [0 0 0 1] (a caller's mistake: the step writes the row all the same)."""
    G = _pose_npz()
    out = {"identity": np.eye(4, dtype=f32)}
    for s in range(4):
        M = np.eye(4, dtype=f32)
        M[:3, :3], M[:3, 3] = G[f"seq{s}_R0"], G[f"seq{s}_T0"]
        out[f"seq{s}"] = M
    M = np.eye(4, dtype=f32)
    M[:3, :3], M[:3, 3] = _rot((0.3, -0.8, 0.52), 170.0).astype(f32), (31.0, -27.5, 28.25)
    out["far"] = M
    M = np.eye(4, dtype=f32)
    M[:3, :3] = (_rot((0.6, 0.2, -0.77), 35.0) @ np.array([[1.0, 0.3, 0.0], [0.0, 0.7, 0.2], [0.0, 0.0, 0.72]])).astype(f32)
    M[:3, 3] = (0.4, -0.3, 0.9)
    out["sheared"] = M
    M = out["seq1"].copy()
    M[3] = (0.25, -0.5, 0.125, 2.0)
    out["last_row"] = M
    return out


ORTHONORMAL = ("identity", "seq0", "seq1", "seq2", "seq3", "far")


def _tau_of(g, lrs, step, moments):
    st = np.zeros(80, dtype=f32)
    if moments is not None:
        st[52:58], st[58:64] = moments
    return adam_ref.pose_step_adam(st, g, None, lrs, step)["tau"]


def grad_for(target, lrs):
    """A gradient whose first Adam step from zero moments gives tau == target.  That step is tau_i = -lr g_i / (|g_i| + 1e-8)
    to rounding, so g_i = -sign(t_i) 1e-8 r / (1 - r) with r = |t_i| / lr < 1; the last bits come from a search over the
    neighbouring float32 gradients.  With r >= 0.5 an ulp of g moves tau by at most half an ulp: every float32 is reached."""
    target = np.asarray(target, dtype=f32)
    lr = np.array([lrs[1]] * 3 + [lrs[0]] * 3, dtype=np.float64)
    r = np.abs(target.astype(np.float64)) / lr
    assert (r < 1).all()
    g = (-np.sign(target) * 1e-8 * r / (1 - r)).astype(f32)
    for _ in range(4):   # the effective epsilon, from what the step gives
        got = np.abs(_tau_of(g, lrs, 1, None).astype(np.float64)) / lr
        with np.errstate(all="ignore"):
            e = np.where(got > 0, np.abs(g.astype(np.float64)) * (1 - got) / np.where(got > 0, got, 1), 0.0)
        g = np.where(target != 0, (-np.sign(target) * e * r / (1 - r)), 0.0).astype(f32)
    best, err = g.copy(), np.abs(_tau_of(g, lrs, 1, None).astype(np.float64) - target)
    up, down = g.copy(), g.copy()
    for _ in range(48):
        up, down = np.nextafter(up, f32(np.inf), dtype=f32), np.nextafter(down, f32(-np.inf), dtype=f32)
        for cand in (up, down):
            e2 = np.abs(_tau_of(cand, lrs, 1, None).astype(np.float64) - target)
            better = (e2 < err) & (target != 0)
            best, err = np.where(better, cand, best).astype(f32), np.where(better, e2, err)
        if not err.any():
            break
    return best


def _direction(rng):
    """A unit vector with no small component: W2 gets non-zero off-diagonals."""
    while True:
        u = rng.standard_normal(3)
        u /= np.linalg.norm(u)
        if np.abs(u).min() > 0.25:
            return u


def _lr_above(x):
    """A learning rate that puts the largest |target| at r = 0.5 ... 0.7 (no power of two: the step size rounds)."""
    return max(float(x) * 1.7, 1e-12)


def _wanted(name, cls, pose, proj, rho, theta, exposure=False, seed=0):
    target = np.concatenate([np.asarray(rho, dtype=np.float64), np.asarray(theta, dtype=np.float64)]).astype(f32)
    lrs = (_lr_above(np.abs(target[3:]).max()), _lr_above(np.abs(target[:3]).max()), 0.01)
    g = grad_for(target, lrs)
    ge = (_rng(9, seed).standard_normal(2) * 1e-2).astype(f32) if exposure else None
    return Case(name, cls, pose, proj, lrs, 1, g, ge, None, _tau_of(g, lrs, 1, None))


@functools.lru_cache(maxsize=None)
def all_cases():
    """Every case of tests/test_gpu_pose_pinned.py, in its order: one launch of one wave each."""
    out = []
    n = 0

    def nxt():   # start pose and projection cycle through the cases
        nonlocal n
        n += 1
        return ORTHONORMAL[n % len(ORTHONORMAL)], n % 4

    # zero angle with a translation; zero translation with a rotation (small branch, large branch)
    for i, (rho_len, ang) in enumerate(((1e-2, 0.0), (1.0, 0.0), (0.0, 3e-6), (0.0, 0.1))):
        rng = _rng(1, i)
        pose, proj = ("identity", i) if i in (0, 2) else nxt()
        out.append(_wanted(f"zero rho={rho_len:g} angle={ang:g}", "zero", pose, proj, rho_len * _direction(rng), ang * _direction(rng)))
    # the small branch.  Every third case starts from the identity with one rho component exactly 0: N = E there, and the row of
    # V that meets the zero shows its off-diagonal terms alone
    for i, ang in enumerate((1e-7, 3e-6, 9.9e-6)):
        for j, rho_len in enumerate((1e-6, 1e-3, 0.1, 1.0)):
            rng = _rng(2, i, j)
            rho = rho_len * _direction(rng)
            pose, proj = nxt()
            if j == 3:
                rho[i] = 0.0
                pose = "identity"
            out.append(_wanted(f"small angle={ang:g} rho={rho_len:g}", "small", pose, proj, rho, ang * _direction(rng),
                               exposure=(j == 1), seed=n))
    # consecutive float32 angles around float32(1e-5): single-axis theta, for which sqrt(fl(x * x)) == |x|
    for k in range(-4, 5):
        rng = _rng(3, k + 4)
        theta = np.zeros(3)
        theta[(k + 4) % 3] = float(shifted(SMALL_ANGLE, k)) * (1 if k % 2 else -1)
        pose, proj = ("identity", 1) if k in (-1, 0, 1) else nxt()
        out.append(_wanted(f"branch threshold {k:+d} ulp", "branch_threshold", pose, proj, 0.1 * _direction(rng), theta))
    # just above: cos rounds to 1 or its predecessor, angle - sin to 0 or an ulp
    for i, ang in enumerate((1.1e-5, 1e-4, 3e-4, 1e-3)):
        for j, rho_len in enumerate((1e-6, 1e-3, 0.1, 1.0)):
            rng = _rng(4, i, j)
            rho = rho_len * _direction(rng)
            pose, proj = nxt()
            if j == 3:
                rho[(i + 1) % 3] = 0.0
                pose = "identity"
            out.append(_wanted(f"above angle={ang:g} rho={rho_len:g}", "above", pose, proj, rho, ang * _direction(rng),
                               exposure=(j == 2), seed=n))
    for i, ang in enumerate((1e-2, 0.1, 0.5, 1.0)):
        for j, rho_len in enumerate((1e-6, 1e-3, 0.1, 1.0)):
            rng = _rng(5, i, j)
            rho = rho_len * _direction(rng)
            pose, proj = nxt()
            if j == 3:
                rho[(i + 2) % 3] = 0.0
                pose = "identity" if i % 2 else pose
            out.append(_wanted(f"large angle={ang:g} rho={rho_len:g}", "large", pose, proj, rho, ang * _direction(rng),
                               exposure=(j == 0), seed=n))
    # |tau| around float32(1e-4): one component alone (the norm is then |x|), in theta and in rho; then mixed, on both sides
    thr = f32(CONVERGED_THRESHOLD)
    for k in range(-3, 4):
        theta = np.zeros(3)
        theta[1] = -float(shifted(thr, k))
        pose, proj = nxt()
        out.append(_wanted(f"converged threshold {k:+d} ulp (theta)", "converged_threshold", pose, proj, np.zeros(3), theta))
    for k in range(-1, 2):
        rho = np.zeros(3)
        rho[2] = float(shifted(thr, k))
        pose, proj = nxt()
        out.append(_wanted(f"converged threshold {k:+d} ulp (rho)", "converged_threshold", pose, proj, rho, np.zeros(3)))
    for i, (rho_len, ang) in enumerate(((6e-5, 6e-5), (8e-5, 8e-5), (5e-4, 5e-5), (5e-5, 5e-4), (9.9e-5, 1e-5), (1e-5, 9.9e-5))):
        rng = _rng(6, i)
        pose, proj = nxt()
        out.append(_wanted(f"converged threshold rho={rho_len:g} angle={ang:g}", "converged_threshold", pose, proj,
                           rho_len * _direction(rng), ang * _direction(rng)))
    # every start pose with a tau of tracking's first iterations and with a wide one
    for i, pose in enumerate(ORTHONORMAL):
        for j, (rho_len, ang) in enumerate(((0.2, 0.3), (1e-3, 3e-3))):
            rng = _rng(7, i, j)
            out.append(_wanted(f"pose {pose} rho={rho_len:g} angle={ang:g}", "poses", pose, (i + j) % 4, rho_len * _direction(rng),
                               ang * _direction(rng), exposure=True, seed=100 + 2 * i + j))
    # preset moments and a later step count: the tau is what Adam gives (|theta_i| <= about lr_rot, |rho_i| <= about lr_trans)
    for i, (lr_rot, lr_trans, step) in enumerate(((0.003, 0.001, 7), (0.0015, 0.0005, 40), (0.3, 0.1, 2), (3e-6, 1e-5, 1000))):
        rng = _rng(8, i)
        m = (rng.standard_normal(6) * 1e-3).astype(f32)
        v = (rng.uniform(0.2, 1.0, 6) * 1e-6).astype(f32)
        g = (rng.standard_normal(6) * 1e-3).astype(f32)
        pose, proj = nxt()
        lrs = (lr_rot, lr_trans, 0.01)
        out.append(Case(f"moments step={step} lr_rot={lr_rot:g}", "moments", pose, proj, lrs, step, g,
                        (rng.standard_normal(2) * 1e-2).astype(f32), (m, v), _tau_of(g, lrs, step, (m, v))))
    # the pose that is no rotation: one full step in either branch; the state with a wrong last row
    rng = _rng(10)
    out.append(_wanted("sheared rho=0.2 angle=0.3", "sheared", "sheared", 0, 0.2 * _direction(rng), 0.3 * _direction(rng)))
    out.append(_wanted("sheared rho=1e-3 angle=3e-6", "sheared", "sheared", 2, 1e-3 * _direction(rng), 3e-6 * _direction(rng)))
    out.append(_wanted("last row rho=0.2 angle=0.3", "last_row", "last_row", 1, 0.2 * _direction(rng), 0.3 * _direction(rng)))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def run_case(case, variant="", sincos=None, tau=None):
    """The restatement's (state, status) after the case's step."""
    return pose_step(case.state(), np.zeros(2, np.int32), case.grad_tau, case.grad_exposure, projections()[case.proj], case.lrs,
                     case.step, sincos=sincos, variant=variant, tau=tau)
