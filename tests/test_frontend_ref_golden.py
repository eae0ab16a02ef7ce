"""The numpy restatement of the front end's frame step (tests/frontend_ref.py) against what the reference computes on the CPU
(tests/golden/frontend.npz, recorded by tests/golden/make_golden_frontend.py from Camera.compute_grad_mask, get_median_depth,
FrontEnd.is_keyframe and FrontEnd.add_to_window).

Tolerances.  Discrete values (the 0 / 1 mask, decisions, windows), the median depth, the counts and the ratios: equal.  The one
exception are mask pixels whose float64 intensity lies within 2^-20 (relative, strictly) of the float64 threshold; at most 0.1 %
of a case's pixels may be such near-ties.  Continuous values (margin intensities, dist, scores) follow the project's rule:
|restatement - truth| <= max(4 |reference - truth|, 4 * 2^-24 * max|truth|), truth being the float64 restatement; over an
array the errors are its largest and its root-mean-square one."""
import os

import numpy as np
import pytest

import frontend_ref as R

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend.npz"))
MASKS = [str(n) for n in GOLD["mask_names"]]
MEDIANS = [str(n) for n in GOLD["med_names"]]
KFS = [str(n) for n in GOLD["kf_names"]]


def _near(I64, th64):
    with np.errstate(invalid="ignore"):
        return np.abs(I64 - th64) < 2.0 ** -20 * np.abs(th64)


def _four_times(mine, ref, truth):
    """Over an array the rule holds for the largest and for the root-mean-square error, as in the other *_ref_golden tests."""
    truth = np.atleast_1d(np.asarray(truth, dtype=np.float64))
    e_got, e_ref = np.abs(np.atleast_1d(mine).astype(np.float64) - truth), np.abs(np.atleast_1d(ref).astype(np.float64) - truth)
    floor = 4 * 2.0 ** -24 * np.max(np.abs(truth))
    rms = lambda e: float(np.sqrt(np.mean(e * e)))  # noqa: E731
    print(f"max {e_got.max():.3e} / {e_ref.max():.3e}, rms {rms(e_got):.3e} / {rms(e_ref):.3e}, floor {floor:.3e}")
    assert e_got.max() <= max(4 * e_ref.max(), floor) and rms(e_got) <= max(4 * rms(e_ref), floor)


def test_golden_covers_the_cases_the_contract_names():
    shapes = {tuple(GOLD[f"mask_{n}_image"].shape[1:]) for n in MASKS}
    assert {(32, 32), (64, 96), (96, 160), (85, 131)} <= shapes
    assert {float(GOLD[f"mask_{n}_thr"]) for n in MASKS} == {4.0, 1.1}
    assert {"ties", "zeros", "inf", "one", "two", "even"} <= set(MEDIANS)
    assert {int(GOLD[f"kf_{n}_kf_poses"].shape[0]) for n in KFS} == {1, 3, 10}
    assert any(GOLD[f"kf_{n}_removed"].size == 2 for n in KFS)
    # every branch of the boolean: neither term, the overlap-and-minimum term alone, the distance term
    assert {(int(GOLD[f"kf_{n}_is_kf"]), int(GOLD[f"kf_{n}_create"])) for n in KFS} == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize("name", MASKS)
def test_mask_blocks(name):
    img, thr, gold = GOLD[f"mask_{name}_image"], float(GOLD[f"mask_{name}_thr"]), GOLD[f"mask_{name}_blocks"]
    mine, _, th = R.grad_mask_blocks(img, thr, np.float32)
    _, I64, th64 = R.grad_mask_blocks(img, thr, np.float64)
    inblock = ~np.isnan(th64)
    near = inblock & _near(I64, th64)
    assert near.sum() <= 1e-3 * near.size
    sel = inblock & ~near
    assert np.array_equal(mine[sel], gold[sel])
    assert set(np.unique(gold[inblock])) <= {0.0, 1.0}
    if (~inblock).any():   # the margins: the raw intensity
        _four_times(mine[~inblock], gold[~inblock], I64[~inblock])
    if name == "x8":       # th >= 1 occurs, and zeroes its blocks
        assert (th[inblock] >= 1).any() and np.all(mine[inblock & (th >= 1)] == 0)
    if name == "flat":
        assert np.all(th[inblock] == 0) and np.all(mine == 0)


@pytest.mark.parametrize("name", MASKS)
def test_mask_global(name):
    img, thr, gold = GOLD[f"mask_{name}_image"], float(GOLD[f"mask_{name}_thr"]), GOLD[f"mask_{name}_global"]
    mine, _, _ = R.grad_mask_global(img, thr, np.float32)
    _, I64, th64 = R.grad_mask_global(img, thr, np.float64)
    near = _near(I64, th64)
    assert near.sum() <= 1e-3 * near.size
    assert np.array_equal(mine[~near], gold[~near])


@pytest.mark.parametrize("name", MEDIANS)
def test_median_depth(name):
    m = GOLD[f"med_{name}_mask"]
    med, n = R.median_depth(GOLD[f"med_{name}_depth"], GOLD[f"med_{name}_opacity"], m if m.size else None)
    assert n == int(GOLD[f"med_{name}_count"])
    assert np.float32(med).tobytes() == np.float32(GOLD[f"med_{name}_median"]).tobytes()


def kf_inputs(name):
    ws, check_time, single = (int(v) for v in GOLD[f"kf_{name}_params"])
    kt, kmt, ko, kc = (float(v) for v in GOLD["kf_train"])
    params = dict(window_size=ws, check_time=check_time, single_thread=single, kf_translation=kt, kf_min_translation=kmt,
                  kf_overlap=ko, kf_cutoff=kc)
    return (params, GOLD[f"kf_{name}_n_touched"], GOLD[f"kf_{name}_vis"], GOLD[f"kf_{name}_cur_pose"], GOLD[f"kf_{name}_kf_poses"],
            np.float32(GOLD[f"kf_{name}_median"]))


@pytest.mark.parametrize("name", KFS)
def test_keyframe_decision(name):
    params, n_touched, vis, cur_pose, kf_poses, median = kf_inputs(name)
    cur, counts = R.covisibility(n_touched, vis)
    assert counts[0] == np.count_nonzero(n_touched > 0) and np.array_equal(cur != 0, n_touched > 0)
    mine = R.decide(params, counts, median, cur_pose, kf_poses, np.float32)
    truth = R.decide(params, counts, median, cur_pose, kf_poses, np.float64)
    assert mine["is_kf"] == bool(GOLD[f"kf_{name}_is_kf"]) and mine["create"] == bool(GOLD[f"kf_{name}_create"])
    assert mine["keep"] == [int(v) for v in GOLD[f"kf_{name}_keep"]]
    assert sorted(p for p in (mine["removed_a"], mine["removed_b"]) if p >= 0) == [int(v) for v in GOLD[f"kf_{name}_removed"]]
    assert np.float32(mine["ratio_u"]).tobytes() == np.float32(GOLD[f"kf_{name}_ratio_u"]).tobytes()
    assert mine["cut"].tobytes() == GOLD[f"kf_{name}_cut"].tobytes()
    _four_times(mine["dist"], GOLD[f"kf_{name}_dist"], truth["dist"])
    scores = GOLD[f"kf_{name}_scores"]
    if scores.size:   # add_to_window scored the positions left after the cut, in window order
        left = [k for k in range(1, len(kf_poses)) if k != mine["removed_a"]]
        assert len(left) == scores.size
        _four_times(mine["score"][left], scores, truth["score"][left])
