"""The online session's host-side pieces without a GPU: ate_rmse against its own definition and against an independent
Kabsch alignment (scipy), the configuration's required keys, and the schedule model's own arithmetic."""
import copy

import numpy as np
import pytest
import torch

import slam_schedule_ref as S
from online_lang_splatting_amd import OnlineSlam, ate_rmse
from online_lang_splatting_amd.slam import REQUIRED_KEYS, parse_config


def random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def trajectory(rng, n, extent=3.0):
    """n world-to-camera poses whose centres spread over `extent` metres."""
    T = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        R = random_rotation(rng)
        c = extent * (rng.random(3) - 0.5)
        T[i, :3, :3], T[i, :3, 3] = R, -R @ c
    return T


def centres(T):
    return np.stack([np.linalg.inv(t)[:3, 3] for t in T])


def test_ate_is_zero_for_a_rigid_transform_of_the_trajectory():
    rng = np.random.default_rng(1)
    for n in (3, 12, 40):
        gt = trajectory(rng, n)
        c = centres(gt)
        extent = float(np.linalg.norm(c.max(axis=0) - c.min(axis=0)))
        tol = 1e-9 * extent   # float64 rounding of a 3 x 3 SVD: a condition, not a measurement
        assert ate_rmse(gt, gt) <= tol
        G = np.eye(4)
        G[:3, :3], G[:3, 3] = random_rotation(rng), 5.0 * rng.standard_normal(3)
        moved = gt @ G          # the same cameras seen from a world moved rigidly: centres G^-1 c
        assert ate_rmse(moved, gt) <= tol, n
        assert ate_rmse(torch.from_numpy(moved), torch.from_numpy(gt)) <= tol


def test_ate_equals_an_independent_kabsch_alignment():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(2)
    gt = trajectory(rng, 12)
    est = gt.copy()
    G = np.eye(4)
    G[:3, :3], G[:3, 3] = random_rotation(rng), rng.standard_normal(3)
    est = est @ G
    for i in range(12):   # noise on the estimate's centres
        R = est[i, :3, :3]
        c = -R.T @ est[i, :3, 3] + 0.05 * rng.standard_normal(3)
        est[i, :3, 3] = -R @ c
    x, y = centres(est), centres(gt)
    xc, yc = x - x.mean(axis=0), y - y.mean(axis=0)
    rot, _ = Rotation.align_vectors(yc, xc)          # the rotation that takes the estimate's centred centres onto the truth's
    err = rot.apply(xc) - yc
    want = float(np.sqrt(np.mean(np.sum(err * err, axis=1))))
    extent = float(np.linalg.norm(y.max(axis=0) - y.min(axis=0)))
    got = ate_rmse(est, gt)
    print(f"ate {got:.12f}, kabsch {want:.12f}")
    assert 0.01 < got < 0.2 and abs(got - want) <= 1e-9 * extent


def test_ate_argument_errors():
    with pytest.raises(ValueError):
        ate_rmse(np.tile(np.eye(4), (3, 1, 1)), np.tile(np.eye(4), (4, 1, 1)))


def _without(config, path):
    c = copy.deepcopy(config)
    node = c
    parts = path.split(".")
    for p in parts[:-1]:
        node = node[p]
    del node[parts[-1]]
    return c


@pytest.mark.parametrize("path", REQUIRED_KEYS + ("language.lang_code_size", "language.single_stage_ae", "opt_params.language_lr"))
def test_a_missing_required_key_raises_keyerror_naming_it(path):
    with pytest.raises(KeyError) as e:
        OnlineSlam(_without(S.SMALL_CONFIG, path), (90.0, 90.0, 89.5, 59.5), 120, 180)   # raises before any GPU work
    assert path in str(e.value)


def test_config_is_parsed_without_a_gpu_and_ignores_unknown_keys():
    c = copy.deepcopy(S.SMALL_CONFIG)
    c["Results"] = {"save_dir": "nowhere"}
    c["Training"]["something_else"] = 3
    del c["Training"]["alpha"]          # optional: the reference's default
    flat = parse_config(c)
    assert flat["Training.alpha"] == 0.95 and flat["Training.lr.cam_rot_delta"] == 0.003
    s = OnlineSlam(c, (90.0, 90.0, 89.5, 59.5), 120, 180, feature_fn=lambda i, im: None, device="cuda")
    assert s.F == 15 and s.mask_mode == "blocks" and s.events == [] and s.map is None
    assert OnlineSlam(c, (90.0, 90.0, 89.5, 59.5), 120, 180).F == 0
    off = copy.deepcopy(c)
    off["language"] = {"language_train": False}
    assert OnlineSlam(off, (90.0, 90.0, 89.5, 59.5), 120, 180, feature_fn=lambda i, im: None).F == 0
    bad = copy.deepcopy(c)
    bad["Training"]["prune_mode"] = "other"
    with pytest.raises(ValueError):
        OnlineSlam(bad, (90.0, 90.0, 89.5, 59.5), 120, 180)


def test_schedule_model():
    frames = [dict(idx=0, iterations=0, is_keyframe=True, window=[0]),
              dict(idx=1, iterations=20, is_keyframe=False, window=[0]),
              dict(idx=2, iterations=7, is_keyframe=True, window=[2, 0]),
              dict(idx=4, iterations=20, is_keyframe=True, window=[4, 2, 0]),
              dict(idx=6, iterations=20, is_keyframe=True, window=[6, 4, 2, 0]),
              dict(idx=7, iterations=3, is_keyframe=False, window=[6, 4, 2, 0]),
              dict(idx=8, iterations=20, is_keyframe=True, window=[8, 6, 4, 0])]
    ev = S.schedule(S.SMALL_CONFIG, frames, language=True)
    assert ev[0] == ("init", 0) and ev[1:3] == [("map", 1, 1), ("densify", 1)]
    assert [e[1] for e in ev if e[0] == "densify"] == [1, 21, 41, 65, 75, 85, 95]
    assert [e[1] for e in ev if e[0] == "reset_opacity"] == [63, 70, 77, 84, 91, 98]
    assert [e for e in ev if e[0] == "removed"] == [("removed", 2)]
    assert [e[1] for e in ev if e[0] == "language"] == [2, 0, 4, 6, 8]
    assert sum(1 for e in ev if e[0] == "prune") == 2
    maps = [e for e in ev if e[0] == "map"]
    assert maps[60] == ("map", 61, 2) and maps[70] == ("map", 72, 3) and maps[80] == ("map", 83, 4) and maps[90] == ("map", 94, 5) and len(maps) == 100
    assert S.normalise([("prune", 10, 8), ("map", 1, 1)]) == [("prune",), ("map", 1, 1)]
    with pytest.raises(AssertionError):
        S.schedule(S.SMALL_CONFIG, frames[:2] + [dict(idx=1, iterations=1, is_keyframe=True, window=[1, 0])], language=False)
