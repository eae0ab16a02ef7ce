"""The geometry half of olsr_pose_step and olsr_window_pose_step (csrc/k_pose.hip: SE3_exp(tau) @ T_w2c, the [0 0 0 1] row,
world_view_transform, full_proj_transform, the cofactor inverse for camera_center, the converged flag) against its float32
restatement tests/pose_ref.py, BIT FOR BIT, on the cases of pose_ref.all_cases() — which tests/test_pose_ref_cpu.py shows to
resolve every term (a list of deliberate mistakes, each told by at least one bit) and to follow the reference's own pose update.

The tau is the one the launch applied, read back from state words 64..69 (with the host step count it is
adam_ref.pose_step_adam's, bit for bit, which is asserted too).  sin(angle) and cos(angle) come from the device's math library:
the host can only say float32(sin64(angle)) and float32(cos64(angle)), so in the large-angle branch the test tries these two
shifted by j and k ulps, |j|, |k| <= K, and asks that ONE pair (j, k) reproduces words 0..51, 64..69 and status together.  In the
small-angle branch nothing is tried: the match is exact.

K.  The search was run with K = 4 (OpenCL's full-profile bound for sin and cos) on an MI355X.  Every one of the 92 cases matched;
the largest |j| seen was 0 (the device's sinf gave float32(sin64) everywhere) and the largest |k| was 1 (its cosf is one ulp
below float32(cos64) at the angles 0.29999998 and 0.30000001, eight cases; (0, 0) everywhere else).  K is now that measured
maximum, 1: a device sine or cosine that moved further, like any other change of a bit, fails."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as A
import pose_ref as P
import window_ba_ref as WB
from online_lang_splatting_amd import _abi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED_J, MEASURED_K = 0, 1   # largest |j| (sine) and |k| (cosine) any case needed when searched with K = 4
K = max(MEASURED_J, MEASURED_K)
CASES = P.all_cases()
POSE, EXPOSURE = _abi.WINDOW_OPT_POSE, _abi.WINDOW_OPT_EXPOSURE
PAIRS = sorted(((j, k) for j in range(-K, K + 1) for k in range(-K, K + 1)), key=lambda p: (abs(p[0]) + abs(p[1]), p))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hp(lrs, step, thr=P.CONVERGED_THRESHOLD):
    return _abi.OlsrPoseParams(lr_rot=float(lrs[0]), lr_trans=float(lrs[1]), lr_exposure=float(lrs[2]), beta1=0.9, beta2=0.999,
                               eps=1e-8, converged_threshold=thr, step=step)


def _single(hp, gt, ge, proj, state, status, frame_status=None):
    from online_lang_splatting_amd._lib import check, lib
    check(lib().olsr_pose_step_gated(C.byref(hp), gt.data_ptr() if gt is not None else None, ge.data_ptr() if ge is not None else None,
                                     proj.data_ptr(), state.data_ptr(), status.data_ptr(),
                                     frame_status.data_ptr() if frame_status is not None else None, _stream()))


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _geometry_equal(got, gstat, want, wstat):
    return bool(A.same_bits(got[:52], want[:52]).all() and A.same_bits(got[64:70], want[64:70]).all() and (gstat == wstat).all())


def _find_pair(before, sbefore, got, gstat, g, ge, proj, lrs, step):
    """The (j, k) for which the restatement, fed with the read-back tau, gives the launch's geometry words and status; (0, 0)
    without a search in the small branch; None if no pair does."""
    tau = got[64:70]
    angle = P.angle_of(tau)
    if P.takes_small_branch(angle):
        want, wstat = P.pose_step(before, sbefore, g, ge, proj, lrs, step, sincos=(None, None), tau=tau)
        return ("small", "small") if _geometry_equal(got, gstat, want, wstat) else None
    s0, c0 = P.host_sincos(angle)
    for j, k in PAIRS:
        want, wstat = P.pose_step(before, sbefore, g, ge, proj, lrs, step, sincos=(P.shifted(s0, j), P.shifted(c0, k)), tau=tau)
        if _geometry_equal(got, gstat, want, wstat):
            return j, k
    return None


@pytest.fixture(scope="module")
def projections(hip):
    return [_dev(p) for p in P.projections()]


def test_full_step_equals_the_restatement(hip, projections):
    """Every case, host step count: Adam words equal adam_ref bit for bit; words 0..51, 64..69 and status equal pose_ref for one
    pair (j, k) of ulp shifts of the sine and cosine.  Measured on an MI355X with K = 4: largest |j| 0, largest |k| 1."""
    before = np.stack([c.state() for c in CASES])
    before[:, 16:52] = np.nan       # the derived words are written, whatever they held
    before[:, 76:80] = (1.5, -2.5, 3.5, -4.5)   # the pad keeps its bits
    state = _dev(before)
    status = torch.zeros(len(CASES), 2, dtype=torch.int32, device=DEV)
    for i, c in enumerate(CASES):
        _single(_hp(c.lrs, c.step), _dev(c.grad_tau), _dev(c.grad_exposure) if c.grad_exposure is not None else None,
                projections[c.proj], state[i], status[i])
    got, gstat = state.cpu().numpy(), status.cpu().numpy()
    sbefore = np.zeros(2, np.int32)
    failures, worst = [], [0, 0]
    for i, c in enumerate(CASES):
        a = A.pose_step_adam(before[i], c.grad_tau, c.grad_exposure, c.lrs, c.step)
        for name, sl in (("tau", slice(64, 70)), ("tau_m", slice(52, 58)), ("tau_v", slice(58, 64)), ("exposure", slice(70, 72)),
                         ("exposure_m", slice(72, 74)), ("exposure_v", slice(74, 76))):
            assert A.same_bits(got[i, sl], a[name]).all(), (c.name, name)
        assert A.same_bits(got[i, 64:70], c.tau).all() and got[i, 76:80].tobytes() == before[i, 76:80].tobytes(), c.name
        pair = _find_pair(before[i], sbefore, got[i], gstat[i], c.grad_tau, c.grad_exposure, P.projections()[c.proj], c.lrs, c.step)
        print(f"{c.name:55s} angle {float(P.angle_of(c.tau)):.9g}  (j, k) = {pair}")
        if pair is None:
            failures.append(c.name)
        elif pair[0] != "small":
            worst = [max(worst[0], abs(pair[0])), max(worst[1], abs(pair[1]))]
    print(f"largest |j| {worst[0]}, largest |k| {worst[1]} (searched |j|, |k| <= {K}; measured with K = 4: {MEASURED_J}, {MEASURED_K})")
    assert not failures, failures


def test_derive_half_and_gating(hip, projections):
    """A call without gradients and a gated call with them (frame_status[1] != 0), on every start pose — the one that is no
    rotation and the one with a wrong last row included: words 0..15 and 52..79 keep their bits, words 16..51 are pose_ref.derive,
    the ungated status is untouched, the gated one is {0, the count it had}."""
    rng = np.random.default_rng(20261021)
    names = sorted(P.start_poses())
    before = np.zeros((2 * len(names), 80), dtype=np.float32)
    for i, n in enumerate(names):
        before[2 * i:2 * i + 2, :16] = P.start_poses()[n].reshape(16)
    before[:, 16:52] = np.nan
    before[:, 52:80] = (rng.standard_normal((len(before), 28)) * 1e-3).astype(np.float32)
    before[:, 58:64] = np.abs(before[:, 58:64])
    state = _dev(before)
    status = torch.tensor([[1, 5]] * len(before), dtype=torch.int32, device=DEV)
    gt, ge = _dev(np.full(6, 0.25, np.float32)), _dev(np.full(2, -0.5, np.float32))
    unusable = torch.tensor([7, 3], dtype=torch.int32, device=DEV)
    for i in range(len(names)):
        _single(_hp((0.003, 0.001, 0.01), 4), None, None, projections[i % 4], state[2 * i], status[2 * i])
        _single(_hp((0.003, 0.001, 0.01), 0), gt, ge, projections[i % 4], state[2 * i + 1], status[2 * i + 1], unusable)
    got, gstat = state.cpu().numpy(), status.cpu().numpy()
    for i, n in enumerate(names):
        want = P.derive(before[2 * i, :16], P.projections()[i % 4])
        for r, what in ((2 * i, "no gradient"), (2 * i + 1, "gated")):
            assert got[r, :16].tobytes() == before[r, :16].tobytes() and got[r, 52:].tobytes() == before[r, 52:].tobytes(), (n, what)
            assert A.same_bits(got[r, 16:52], want).all(), (n, what, got[r, 16:52].tolist(), want.tolist())
        assert gstat[2 * i].tolist() == [1, 5] and gstat[2 * i + 1].tolist() == [0, 5], n


WINDOW = ("small angle=9.9e-06 rho=1", "large angle=0.5 rho=0.1", "above angle=0.001 rho=0.001")


def test_window_step_equals_the_restatement(hip, projections):
    """One olsr_window_pose_step, V = 3, flags {POSE|EXPOSURE, POSE, EXPOSURE}, host count 1: the start poses and taus of three cases
    from different classes under shared rates (the gradients are solved again for them).  Views 0 and 1 equal the restatement of
    the full step, pair search included; view 2 takes its exposure step alone, keeps its pose words and re-derives its matrices
    (its pose gradient is NaN: it is not read)."""
    from online_lang_splatting_amd._lib import check, lib
    by_name = {c.name: c for c in CASES}
    cases = [by_name[n] for n in WINDOW]
    assert len({c.cls for c in cases}) == 3
    taus = np.stack([c.tau for c in cases[:2]])
    lrs = (1.7 * float(np.abs(taus[:, 3:]).max()), 1.7 * float(np.abs(taus[:, :3]).max()), 0.01)
    grad = np.stack([P.grad_for(cases[0].tau, lrs), P.grad_for(cases[1].tau, lrs), np.full(6, np.nan, np.float32)])
    gexp = np.array([[0.01, -0.02], [np.nan, np.nan], [-0.03, 0.005]], dtype=np.float32)
    flags = [POSE | EXPOSURE, POSE, EXPOSURE]
    before = np.stack([c.state() for c in cases])
    before[:, 16:52] = np.nan
    state, status = _dev(before), torch.zeros(3, 2, dtype=torch.int32, device=DEV)
    hp, dgrad, dgexp = _hp(lrs, 1), _dev(grad), _dev(gexp)
    check(lib().olsr_window_pose_step(C.byref(hp), 3, (C.c_int32 * 3)(*flags), dgrad.data_ptr(), dgexp.data_ptr(),
                                      projections[1].data_ptr(), state.data_ptr(), status.data_ptr(), None, _stream()))
    got, gstat = state.cpu().numpy(), status.cpu().numpy()
    proj = P.projections()[1]
    for v in (0, 1):
        ge = gexp[v] if flags[v] & EXPOSURE else None
        a = A.pose_step_adam(before[v], grad[v], ge, lrs, 1)
        assert A.same_bits(got[v, 64:70], a["tau"]).all() and A.same_bits(got[v, 70:76], np.concatenate(
            [a["exposure"], a["exposure_m"], a["exposure_v"]])).all(), v
        assert P.takes_small_branch(P.angle_of(got[v, 64:70])) == (v == 0)   # one view in either branch
        pair = _find_pair(before[v], np.zeros(2, np.int32), got[v], gstat[v], grad[v], ge, proj, lrs, 1)
        print(f"view {v} ({cases[v].name}): (j, k) = {pair}")
        assert pair is not None, cases[v].name
    want, wstat = before[2:3].copy(), np.zeros((1, 2), np.int32)
    WB.window_step(want, wstat, [EXPOSURE], grad[2:3], gexp[2:3], proj, lrs, step=1)
    assert A.same_bits(got[2], want[0]).all() and (gstat[2] == wstat[0]).all() and gstat[2].tolist() == [0, 1]
    assert got[2, :16].tobytes() == before[2, :16].tobytes()


DEVICE_COUNT = WINDOW + ("moments step=7 lr_rot=0.003",)


def test_device_step_count_geometry_equals_the_restatement(hip, projections):
    """params->step = 0: the count is status[1] + 1 and the bias corrections come from the device's pow, so the Adam words are held
    to adam_ref within the existing tolerance of that path (rtol 1e-6) — and the geometry words to the restatement, bit for bit,
    fed with the tau the launch itself left in words 64..69."""
    by_name = {c.name: c for c in CASES}
    for n in DEVICE_COUNT:
        c = by_name[n]
        before, sbefore = c.state(), np.array([1, c.step - 1], dtype=np.int32)
        state, status = _dev(before), _dev(sbefore)
        _single(_hp(c.lrs, 0), _dev(c.grad_tau), _dev(c.grad_exposure) if c.grad_exposure is not None else None, projections[c.proj],
                state, status)
        got, gstat = state.cpu().numpy(), status.cpu().numpy()
        a = A.pose_step_adam(before, c.grad_tau, c.grad_exposure, c.lrs, c.step)
        np.testing.assert_allclose(got[64:70], a["tau"], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(got[52:64], np.concatenate([a["tau_m"], a["tau_v"]]), rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(got[70:76], np.concatenate([a["exposure"], a["exposure_m"], a["exposure_v"]]), rtol=1e-6, atol=1e-12)
        assert gstat[1] == c.step
        pair = _find_pair(before, sbefore, got, gstat, c.grad_tau, c.grad_exposure, P.projections()[c.proj], c.lrs, c.step)
        print(f"{c.name}: (j, k) = {pair}")
        assert pair is not None, c.name
