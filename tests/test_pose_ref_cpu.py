"""tests/pose_ref.py on the CPU: that its case list can tell the restatement from every mistake it names, by bits (the GPU
comparison of tests/test_gpu_pose_pinned.py is by bits, so a term no case resolves would not be pinned); that the list covers
both thresholds from both sides; and that the restatement is the reference's pose update, against tests/golden/pose_wide.npz
(tests/golden/make_golden_pose_wide.py: one update_pose + update_RT + camera properties per case, in float32 and on float64
tensors).

The yardstick against the reference is the project's ratio rule, per class and pooled over the class's cases, for each of R, T,
view, full and campos: the largest and the root-mean-square |restatement - truth| are at most max(4 x the same of the
reference's float32 run, 4 * 2^-24 * max|truth|).  The pose that is no rotation has no counterpart in the reference's runs: it
is held to the float64 statement by the floor alone."""
import os

import numpy as np
import pytest

import adam_ref
import pose_ref as P

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_wide.npz"))
CASES = P.all_cases()
QUANTITIES = ("R", "T", "view", "full", "campos")


@pytest.fixture(scope="module")
def restated():
    """(state, status) of every case, once."""
    return [P.run_case(c) for c in CASES]


def _quantities(state):
    T = state[:16].reshape(4, 4)
    return dict(R=T[:3, :3], T=T[:3, 3], view=state[16:32].reshape(4, 4), full=state[32:48].reshape(4, 4), campos=state[48:51])


# ---- coverage -------------------------------------------------------------------------------------------------------------------
def test_the_list_covers_what_it_names():
    assert 80 <= len(CASES) <= 120 and {c.cls for c in CASES} == set(P.CLASSES)
    angle = {c.name: P.angle_of(c.tau) for c in CASES}
    assert all(a.dtype == np.float32 and a <= 1.000001 for a in angle.values())   # the list stops at 1 rad (to rounding)
    for cls, (lo, hi) in P.ANGLE_RANGE.items():
        got = [float(angle[c.name]) for c in CASES if c.cls == cls]
        assert got and all(lo <= a <= hi for a in got), (cls, got)
    zero = [c for c in CASES if c.cls == "zero"]
    assert any(angle[c.name] == 0 and c.tau[:3].any() for c in zero) and any(angle[c.name] > 0 and not c.tau[:3].any() for c in zero)
    # every range of |rho| in either branch, and an exactly-zero rho component beside non-zero ones
    for cls in ("small", "large"):
        rho = [float(np.linalg.norm(c.tau[:3].astype(np.float64))) for c in CASES if c.cls == cls]
        assert min(rho) < 2e-6 and max(rho) > 0.5, (cls, rho)
        assert any((c.tau[:3] == 0).sum() == 1 for c in CASES if c.cls == cls)
    # mixed axes: W2 has off-diagonals everywhere but at the single-axis thresholds
    for c in CASES:
        if c.cls in ("small", "above", "large", "poses", "sheared"):
            assert (c.tau[3:] != 0).all(), c.name
    assert {c.pose for c in CASES} == set(P.start_poses()) and {c.proj for c in CASES} == {0, 1, 2, 3}
    far, sheared = P.start_poses()["far"].astype(np.float64), P.start_poses()["sheared"].astype(np.float64)
    assert np.degrees(np.arccos((np.trace(far[:3, :3]) - 1) / 2)) > 169 and 45 < np.linalg.norm(far[:3, 3]) < 55
    assert 0.45 < np.linalg.det(sheared[:3, :3]) < 0.55 and np.abs(sheared[:3, :3] @ sheared[:3, :3].T - np.eye(3)).max() > 0.2
    assert any(c.moments is not None and c.step > 1 for c in CASES)


def test_the_branch_threshold_is_met_from_both_sides_and_exactly():
    run = [P.angle_of(c.tau) for c in CASES if c.cls == "branch_threshold"]
    assert any(a < P.SMALL_ANGLE for a in run) and any(a > P.SMALL_ANGLE for a in run) and any(a == P.SMALL_ANGLE for a in run)
    # consecutive float32 values: nothing between two neighbours of the run
    srt = sorted(run)
    assert all(np.nextafter(a, np.float32(1), dtype=np.float32) == b for a, b in zip(srt, srt[1:])), srt
    assert P.SMALL_ANGLE.dtype == np.float32 and float(P.SMALL_ANGLE) != 1e-5


def test_the_converged_threshold_is_met_from_both_sides_and_exactly():
    thr = np.float32(P.CONVERGED_THRESHOLD)
    for part in (slice(3, 6), slice(0, 3)):   # carried by theta alone, by rho alone
        run = [P.tau_norm(c.tau) for c in CASES if c.cls == "converged_threshold" and c.tau[part].any() and np.count_nonzero(c.tau) == 1]
        assert any(n < thr for n in run) and any(n > thr for n in run) and any(n == thr for n in run), run
    mixed = [P.tau_norm(c.tau) for c in CASES if c.cls == "converged_threshold" and np.count_nonzero(c.tau) == 6]
    assert any(n < thr for n in mixed) and any(n > thr for n in mixed)
    # |theta| below the threshold and |tau| above it: what tells the flag from one that looked at theta alone
    assert any(P.angle_of(c.tau) < thr < P.tau_norm(c.tau) for c in CASES)


def test_the_tau_of_every_case_is_adams():
    """The tau a case records is adam_ref.pose_step_adam's on its state, gradient, rates and count: the GPU test reads the same
    bits back from words 64..69."""
    for c in CASES:
        a = adam_ref.pose_step_adam(c.state(), c.grad_tau, c.grad_exposure, c.lrs, c.step)
        assert adam_ref.same_bits(a["tau"], c.tau).all(), c.name


# ---- resolving power ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_some_case_tells_the_mutant_by_a_bit(restated, mutant):
    caught = []
    for c, (state, status) in zip(CASES, restated):
        mstate, mstatus = P.run_case(c, variant=mutant)
        if not adam_ref.same_bits(state, mstate).all() or (status != mstatus).any():
            caught.append(c.name)
    print(f"{mutant}: {len(caught)} of {len(CASES)} cases")
    assert caught, f"no case resolves the mutant {mutant}"


def test_the_candidates_of_the_gpu_test_differ(restated):
    """An ulp of the sine or of the cosine shows in the pose words of every large-branch case that starts from the identity
    (N = E there) with mixed axes and a translation: on those the pair the GPU test finds is the only one."""
    seen = 0
    for c, (state, _) in zip(CASES, restated):
        angle = P.angle_of(c.tau)
        if P.takes_small_branch(angle) or c.pose != "identity" or not c.tau[:3].any() or not c.tau[3:].all():
            continue
        s, co = P.host_sincos(angle)
        for sc in ((P.shifted(s, 1), co), (s, P.shifted(co, -1))):
            other, _ = P.run_case(c, sincos=sc)
            assert not adam_ref.same_bits(state[:16], other[:16]).all(), (c.name, sc)
        seen += 1
    assert seen >= 8


# ---- against the reference ------------------------------------------------------------------------------------------------------
def test_the_golden_file_is_the_list():
    names = [c.name for c in CASES if c.cls != "last_row"]
    assert [str(n) for n in GOLD["names"]] == names
    by_name = {c.name: c for c in CASES}
    for i, n in enumerate(names):
        c = by_name[n]
        assert str(GOLD["classes"][i]) == c.cls and int(GOLD["proj_index"][i]) == c.proj
        assert adam_ref.same_bits(GOLD["tau"][i], c.tau).all(), n
        T0 = P.start_poses()[c.pose]
        assert GOLD["R0"][i].tobytes() == T0[:3, :3].tobytes() and GOLD["T0"][i].tobytes() == T0[:3, 3].tobytes()
    assert all(GOLD[f"ref32_{q}"].dtype == np.float32 and GOLD[f"truth_{q}"].dtype == np.float64 for q in QUANTITIES)


def _pooled(cls, restated):
    idx = {str(n): i for i, n in enumerate(GOLD["names"])}
    rows = [(idx[c.name], _quantities(state)) for c, (state, _) in zip(CASES, restated) if c.cls == cls]
    assert rows
    for q in QUANTITIES:
        truth = np.concatenate([GOLD[f"truth_{q}"][i].reshape(-1) for i, _ in rows])
        ref = np.concatenate([GOLD[f"ref32_{q}"][i].reshape(-1) for i, _ in rows]).astype(np.float64)
        mine = np.concatenate([m[q].reshape(-1) for _, m in rows]).astype(np.float64)
        yield q, mine, ref, truth


def _rms(e):
    return float(np.sqrt(np.mean(e * e)))


@pytest.mark.parametrize("cls", [c for c in P.CLASSES if c not in P.NO_REFERENCE])
def test_ratio_rule_per_class(restated, cls):
    bad = []
    for q, mine, ref, truth in _pooled(cls, restated):
        e_got, e_ref = np.abs(mine - truth), np.abs(ref - truth)
        floor = 4 * 2.0 ** -24 * np.max(np.abs(truth))
        allow_max, allow_rms = max(4 * e_ref.max(), floor), max(4 * _rms(e_ref), floor)
        print(f"{cls:20s} {q:7s} max {e_got.max():.3e} / {e_ref.max():.3e} ratio {e_got.max() / allow_max:.3f}   "
              f"rms {_rms(e_got):.3e} / {_rms(e_ref):.3e} ratio {_rms(e_got) / allow_rms:.3f}   floor {floor:.3e}")
        if not (e_got.max() <= allow_max and _rms(e_got) <= allow_rms):
            bad.append(q)
    assert not bad, (cls, bad)


def test_the_pose_that_is_no_rotation_against_float64(restated):
    """The floor alone: 4 * 2^-24 * max|truth|, truth being the reference's functions on float64 tensors (a general inverse)."""
    bad = []
    for q, mine, _, truth in _pooled("sheared", restated):
        e, floor = np.abs(mine - truth), 4 * 2.0 ** -24 * np.max(np.abs(truth))
        print(f"sheared {q:7s} max {e.max():.3e} rms {_rms(e):.3e} floor {floor:.3e} ratio {e.max() / floor:.3f}")
        if not e.max() <= floor:
            bad.append(q)
    assert not bad, bad


def test_flags_away_from_the_threshold_are_the_references(restated):
    """Where |tau| is further than four ulps from float32(1e-4) the flag is the reference's; at the threshold the reference's norm
    (another summation order) may round to the other side: those cases are printed."""
    idx = {str(n): i for i, n in enumerate(GOLD["names"])}
    thr = np.float32(P.CONVERGED_THRESHOLD)
    compared = 0
    for c, (_, status) in zip(CASES, restated):
        if c.cls == "last_row":
            continue
        ref, truth = bool(GOLD["ref32_converged"][idx[c.name]]), bool(GOLD["truth_converged"][idx[c.name]])
        if abs(float(P.tau_norm(c.tau)) - float(thr)) > 4 * float(np.spacing(thr)):
            assert bool(status[0]) == ref == truth, c.name
            compared += 1
        else:
            print(f"{c.name}: restatement {int(status[0])}, reference {int(ref)}, float64 {int(truth)}")
    assert compared >= 70


@pytest.mark.parametrize("pose", sorted(P.start_poses()))
def test_derive_against_the_float64_inverse(pose):
    """Words 16..51 from a start pose: the transpose is exact, full_proj and camera_center are within 4 * 2^-24 of the largest
    float64 value — the general inverse, also where R is no rotation.  (The state with a wrong last row: R and T are seq1's.)"""
    T = P.start_poses()[pose]
    for k, proj in enumerate(P.projections()):
        d = P.derive(T.reshape(16), proj)
        assert d[:16].tobytes() == np.ascontiguousarray(T.T).tobytes() and d[35] == 0 and not np.signbit(d[35])
        full64 = T.T.astype(np.float64) @ proj.astype(np.float64)
        campos64 = -np.linalg.inv(T[:3, :3].astype(np.float64)) @ T[:3, 3].astype(np.float64)
        for name, got, want in (("full", d[16:32], full64.reshape(16)), ("campos", d[32:35], campos64)):
            e, floor = np.abs(got - want).max(), 4 * 2.0 ** -24 * np.abs(want).max()
            print(f"{pose} proj {k} {name}: {e:.3e} floor {floor:.3e}")
            assert e <= floor or e == 0, (pose, k, name)
