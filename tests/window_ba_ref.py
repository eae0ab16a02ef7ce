"""numpy restatement of mapping's bundle adjustment (include/olsr.h: olsr_window_pose_step, olsr_isotropic_reg,
olsr_adam_step_groups_reg).  The window step is, per view, the pose step of tests/adam_ref.py (the Adam words, bit for bit
what the kernel computes) and of oracle/pose_oracle.py (SE3_exp and the camera matrices, to rounding); the regulariser is
written from the header's arithmetic.  Pinned to the reference's own run by tests/test_window_ba_ref_golden.py
(tests/golden/window_ba.npz)."""
import numpy as np

import adam_ref
from oracle.pose_oracle import se3_exp

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
    """Words 16..51 of one state from its pose (the oracle's arithmetic: to rounding, not to the bit)."""
    Tm = state[:16].reshape(4, 4)
    view = Tm.T.copy()
    state[16:32] = view.reshape(16)
    state[32:48] = (view @ np.asarray(proj, dtype=f32)).astype(f32).reshape(16)
    state[48:51] = np.linalg.inv(view.astype(np.float64))[3, :3].astype(f32)
    state[51] = 0


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
            Tn = (se3_exp(a["tau"]) @ st[:16].reshape(4, 4)).astype(f32)
            Tn[3] = (0, 0, 0, 1)
            st[:16] = Tn.reshape(16)
            t = a["tau"]
            nrm = f32(np.sqrt(f32(t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3] + t[4] * t[4] + t[5] * t[5])))
            status[v, 0] = int(nrm < f32(thr))
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
