"""numpy restatement of mapping's bundle adjustment (include/olsr.h: olsr_window_pose_step, olsr_isotropic_reg,
olsr_adam_step_groups_reg).  The window step is, per view, the pose step of tests/adam_ref.py (the Adam words) and of
tests/pose_ref.py (SE3_exp, the convergence flag and the camera matrices): both bit for bit what the kernel computes, given the
float32 sine and cosine of the angle — here the double ones rounded to float32 (pose_ref.host_sincos), which the device's
may miss by an ulp (tests/test_gpu_pose_pinned.py searches the neighbours); the regulariser is written from the header's
arithmetic.  Pinned to the reference's own run by tests/test_window_ba_ref_golden.py (tests/golden/window_ba.npz)."""
import numpy as np

import adam_ref
import pose_ref

f32 = np.float32
POSE, EXPOSURE = 1, 2


def make_states(R, T, exposure):
    """[V,80] float32 states from [V,3,3] rotations, [V,3] translations and [V,2] exposures; every other word zero."""
    V = len(R)
    st = np.zeros((V, 80), dtype=f32)
    for v in range(V):
        M = np.eye(4, dtype=f32)
        M[:3, :3], M[:3, 3] = R[v], T[v]
        st[v, :16] = M.reshape(16)
        st[v, 70:72] = exposure[v]
    return st


def derive_matrices(state, proj):
    """Words 16..51 of one state from its pose: pose_ref.derive, the kernel's bits."""
    state[16:52] = pose_ref.derive(state[:16], proj)


def window_step(states, status, flags, grad_tau, grad_exposure, proj, lrs, step=None, gated=None, thr=1e-4):
    """One olsr_window_pose_step on [V,80] states and [V,2] status (both updated in place).  lrs = (rot, trans, exposure);
    step: the host-side count for every view, or None = each view's own status[v][1] + 1; gated: per view, True = its frame
    was not usable."""
    for v in range(len(states)):
        st, fl = states[v], int(flags[v])
        if gated is not None and gated[v]:
            fl = 0
            status[v, 0] = 0
        k = int(step) if step is not None else int(status[v, 1]) + 1
        if fl & POSE:
            a = adam_ref.pose_step_adam(st, grad_tau[v], grad_exposure[v] if fl & EXPOSURE else None, lrs, k)
            st[52:58], st[58:64], st[64:70] = a["tau_m"], a["tau_v"], a["tau"]
            st[70:72], st[72:74], st[74:76] = a["exposure"], a["exposure_m"], a["exposure_v"]
            sn, cs = pose_ref.host_sincos(pose_ref.angle_of(a["tau"]))
            st[:16], status[v, 0] = pose_ref.apply_tau(st[:16], a["tau"], sn, cs, threshold=thr)
            status[v, 1] += 1
        elif fl & EXPOSURE:
            a = adam_ref.pose_step_adam(st, np.zeros(6, f32), grad_exposure[v], lrs, k)
            st[70:72], st[72:74], st[74:76] = a["exposure"], a["exposure_m"], a["exposure_v"]
            status[v, 0] = 0
            status[v, 1] += 1
        derive_matrices(st, proj)


def isotropic_rows(x, raw, weight, P_total=None):
    """(r [P,3] float32, d [P,3] float32): the regulariser's gradient with respect to x and s_k - m, per the header.  raw: x
    is log(scale); the exp is numpy's float32 exp, which may differ from the device's by an ulp (the activated form has no
    exp: it is the kernel's bits)."""
    x = np.asarray(x, dtype=f32)
    P = x.shape[0]
    s = np.exp(x).astype(f32) if raw else x
    m = ((s[:, 0] + s[:, 1]) + s[:, 2]) / f32(3.0)
    d = s - m[:, None]
    sg = (d > 0).astype(np.int32) - (d < 0).astype(np.int32)
    q = 3 * sg - sg.sum(axis=1, keepdims=True)
    w9 = f32(weight / (9.0 * (P if P_total is None else P_total)))
    r = w9 * q.astype(f32)
    if raw:
        r = r * s
    assert r.dtype == f32 and d.dtype == f32
    return r, d


def isotropic_loss(x, raw, weight):
    """weight / (3 P) * sum |d_k| with the sum in float64 (the order is not the kernel's: compare to rounding)."""
    _, d = isotropic_rows(x, raw, weight)
    return weight / (3.0 * d.shape[0]) * float(np.abs(d).astype(np.float64).sum())
