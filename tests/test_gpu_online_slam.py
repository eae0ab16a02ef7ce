"""The online SLAM session (online_lang_splatting_amd.slam.OnlineSlam) on a ray-cast room sequence, at the smallest shape that
still takes every branch: 180 x 120 pixels (12 x 8 tiles), 10 frames one degree apart on the room's keyframe loop,
kf_interval 2, window_size 4, pose_window 2, 60 initialisation, 20 tracking and 10 mapping iterations, densification every 10
and the non-visible opacity reset every 7 iteration counts, F = 15 code maps from the room's surface codes handed in through
feature_fn (tests/slam_schedule_ref.py: SMALL_CONFIG).

The shape is raised from the suggested 8 frames and window_size 3, because the prune condition cannot be met there without
emptying the map: the "slam" co-visibility prune drops every Gaussian of the window's three newest keyframes that at most
three views see, which in a window of three is the whole map (measured: P 13379 -> 0).  A window of four keeps the
Gaussians all four views see, and needs five keyframes, hence ten frames, for a removal.  Two thresholds follow from the
iteration counts: an opacity moves by at most opacity_lr = 0.05 in logit per step, so a keyframe's new Gaussians (opacity
0.5) cannot reach the reference's gaussian_th = 0.7 within the 5 steps before the next densification (the reference gives
them 50 to 150): gaussian_th is 0.3 here.  For the same reason initialize_map's own reset_opacity (to 0.01) is taken in the
use_gt_pose run only, at iteration 2 and with a prune threshold of 0.005.

One module-scoped set of runs is shared by the tests: the session (twice, for determinism), the same sequence without
tracking iterations, with ground-truth poses, and without language.  The coverage conditions on `events` are asserted first,
in the fixture, so that no branch is skipped silently."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

import slam_schedule_ref as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, F, FRAMES, STEP_DEG = 180, 120, 15, 10, 1.0
DEPTH_SCALE = 6553.5
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "online_slam_small.json")


def path_cameras():
    """FRAMES poses on scene.room_keyframe_cameras' loop, STEP_DEG apart: consecutive frames overlap."""
    from online_lang_splatting_amd.scene import ROOM_HALF, Camera
    cams = []
    for k in range(FRAMES):
        a = math.radians(STEP_DEG * k)
        R = torch.tensor([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])
        c = torch.tensor([0.9 * math.sin(a) * ROOM_HALF[0] / 3.5, 0.1, 0.9 * math.cos(a) * ROOM_HALF[2] / 3.5])
        cams.append(Camera(W, H, W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0, R, -(R @ c)))
    return cams


def make_sequence():
    """Per frame: rgb uint8 [H,W,3], depth uint16 [H,W] (both on the device), the ground-truth w2c and the [F,h,w] code map."""
    from online_lang_splatting_amd.scene import _raycast_room, _room_colour, _surface_codes, world2view2
    codes = _surface_codes(F)
    seq = []
    for cam in path_cameras():
        depth, hitp, sid = _raycast_room(cam, W, H)
        rgb = (_room_colour(hitp, sid) * 255.0).round().clamp(0, 255).to(torch.uint8)
        d16 = (depth.double() * DEPTH_SCALE).round().clamp(0, 65535).to(torch.int32).numpy().astype(np.uint16)
        _, _, sid_l = _raycast_room(cam, 48, 32)
        seq.append(dict(rgb=rgb.contiguous().to(DEV), depth=torch.from_numpy(d16).to(DEV), w2c=world2view2(cam.R, cam.T),
                        codes=codes[sid_l].permute(2, 0, 1).contiguous().to(DEV)))
    return seq


def config(**training):
    c = copy.deepcopy(S.SMALL_CONFIG)
    c["Training"].update(training)
    return c


def run(seq, cfg, language=True, probe=None):
    """The whole sequence through one session.  probe(slam, k, result): called after frame k."""
    from online_lang_splatting_amd import OnlineSlam
    fx = W / 2.0
    slam = OnlineSlam(cfg, (fx, fx, (W - 1) / 2.0, (H - 1) / 2.0), H, W,
                      feature_fn=(lambda i, image: seq[i]["codes"]) if language else None, device=DEV)
    results = []
    for k, f in enumerate(seq):
        r = slam.track(k, f["rgb"], f["depth"], DEPTH_SCALE, gt_w2c=f["w2c"] if (k == 0 or cfg["Training"]["use_gt_pose"]) else None)
        results.append(r)
        if probe is not None:
            probe(slam, k, r)
    torch.cuda.synchronize()
    return slam, results


def kf0_loss(slam, seq):
    """Keyframe 0's mapping loss (RGB + depth + language L1) as the map renders it now; frame 0's pose and exposure are fixed."""
    from online_lang_splatting_amd import losses
    from online_lang_splatting_amd.frontend import ingest_frame
    image, depth = ingest_frame(seq[0]["rgb"], seq[0]["depth"], DEPTH_SCALE)
    out = slam.render(seq[0]["w2c"])
    lo = losses.mapping_loss(out["color"], out["depth"], out["language"], image, depth, seq[0]["codes"],
                             torch.zeros(2, device=DEV))
    return [float(v) for v in lo["loss"].cpu()]


@pytest.fixture(scope="module")
def runs():
    seq = make_sequence()
    seen = {}

    def probe(slam, k, r):
        if k == 0:
            seen["params0"] = {n: (v.clone() if v is not None else None) for n, v in slam.map.params.items()}
            seen["pose0"] = slam.poses[0].clone()
            seen["vis0"] = (slam.selector.visibility[0].clone(), slam.map.P)
            seen["fresh0"] = slam.render(slam.poses[0])["n_touched"] > 0
            seen["loss_init"] = kf0_loss(slam, seq)
        if k > 0 and r["is_keyframe"] and "vis_kf" not in seen:
            seen["vis_kf"] = (k, slam.selector.visibility[k].clone(), slam.map.P, list(r["window"]))
            seen["fresh_kf"] = slam.render(slam.poses[k])["n_touched"] > 0
    a, ra = run(seq, config(), probe=probe)
    ev = a.events
    print("events:", [e for e in ev if e[0] != "map"])
    # ---- coverage conditions: no branch is skipped silently
    kinds = [e[0] for e in ev]
    n_kf = 1 + kinds.count("keyframe")
    assert any(not r["is_keyframe"] for r in ra[1:]), "no tracked frame that is no keyframe"
    assert n_kf >= S.SMALL_CONFIG["Training"]["window_size"] + 1 and "removed" in kinds, ("too few keyframes", n_kf)
    assert "densify" in kinds and any(e[0] == "densify" and e[1] > 60 for e in ev)
    assert any(e[0] == "reset_opacity" and e[1] > 60 for e in ev)
    assert "prune" in kinds
    seen["loss_end"] = kf0_loss(a, seq)
    b, rb = run(seq, config())
    still, rs = run(seq, config(tracking_itr_num=0))
    gt, rg = run(seq, config(use_gt_pose=True, init_gaussian_reset=2, gaussian_th=0.005))
    plain, rp = run(seq, config(), language=False)
    return dict(seq=seq, seen=seen, a=(a, ra), b=(b, rb), still=(still, rs), gt=(gt, rg), plain=(plain, rp))


def frames_of(results):
    return [dict(idx=k, iterations=r["iterations"], is_keyframe=r["is_keyframe"], window=r["window"]) for k, r in enumerate(results)]


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu().numpy().tobytes()


def test_schedule(runs):
    """1. `events` equals the schedule model's trace, fed the run's own keyframe decisions and windows."""
    for name, language in (("a", True), ("still", True), ("gt", True), ("plain", False)):
        slam, results = runs[name]
        cfg = slam_config(name)
        want = S.schedule(cfg, frames_of(results), language=language)
        assert S.normalise(slam.events) == want, name
        for e in slam.events:
            if e[0] == "prune":
                assert 0 < e[2] <= e[1]
    assert any(e[0] == "reset_opacity" and e[1] == 2 for e in runs["gt"][0].events)   # initialize_map's own reset


def slam_config(name):
    return {"a": config(), "still": config(tracking_itr_num=0), "gt": config(use_gt_pose=True, init_gaussian_reset=2, gaussian_th=0.005),
            "plain": config()}[name]


def test_wiring_of_tracking(runs):
    """2. The first tracked frame's pose equals, bit for bit, a TrackingLoop built by hand on the session's map snapshot, the
    ingested image, the mask and the previous pose."""
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    from online_lang_splatting_amd.frontend import ingest_frame, tracking_mask
    from online_lang_splatting_amd.slam_iterations import PoseState, TrackingLoop
    seq, seen = runs["seq"], runs["seen"]
    slam, results = runs["a"]
    T = S.SMALL_CONFIG["Training"]
    image, depth = ingest_frame(seq[1]["rgb"], seq[1]["depth"], DEPTH_SCALE)
    mask = tracking_mask(image, T["edge_threshold"], "blocks")
    params = seen["params0"]
    P = params["means3D"].shape[0]
    ws = RasterWorkspace(P, W, H, F, 1, slam.capacity, DEV)
    pose = PoseState(seen["pose0"], slam.proj, slam.tanfovx, slam.tanfovy, lr_rot=T["lr"]["cam_rot_delta"],
                     lr_trans=T["lr"]["cam_trans_delta"], lr_exposure=0.01)
    loop = TrackingLoop(ws, dict(params, bg=torch.zeros(3, device=DEV), activations=_abi.ACT_ALL), 0, pose, image, depth, mask,
                        alpha=T["alpha"], rgb_boundary_threshold=T["rgb_boundary_threshold"])
    n = 0
    for k in range(T["tracking_itr_num"]):
        n += 1
        if loop.iteration(read_convergence=True, write_images=(k == T["tracking_itr_num"] - 1)):
            break
    assert not results[1]["is_keyframe"] and results[1]["iterations"] == n
    assert bits(pose.T_w2c) == bits(results[1]["w2c"])
    assert bits(results[1]["w2c"]) != bits(seen["pose0"])   # it moved


def test_wiring_of_a_keyframe(runs):
    """3. After the first frame and after the first tracked keyframe the selector's stored visibility has the map's current
    rows and equals n_touched > 0 of a fresh render of that keyframe's pose."""
    seen = runs["seen"]
    vis0, P0 = seen["vis0"]
    assert vis0.numel() == P0 and vis0.dtype == torch.uint8 and torch.equal(vis0.bool(), seen["fresh0"]) and int(vis0.sum()) > 0
    k, vis, P, window = seen["vis_kf"]
    assert len(window) < S.SMALL_CONFIG["Training"]["window_size"]     # (no prune yet: the stored rows are the rendered ones)
    assert vis.numel() == P and P != P0 and torch.equal(vis.bool(), seen["fresh_kf"]) and int(vis.sum()) > 0


def test_determinism(runs):
    """4. A second identical run: the same poses, events and map parameters, bit for bit."""
    (a, ra), (b, rb) = runs["a"], runs["b"]
    assert a.events == b.events
    assert [r["is_keyframe"] for r in ra] == [r["is_keyframe"] for r in rb] and [r["window"] for r in ra] == [r["window"] for r in rb]
    assert bits(a.trajectory()[1]) == bits(b.trajectory()[1])
    assert a.map.P == b.map.P
    for n, v in a.map.params.items():
        if v is not None:
            assert bits(v) == bits(b.map.params[n]), n


def test_it_tracks(runs):
    """5. The estimated trajectory's ATE is strictly below that of the same sequence without tracking iterations (every frame
    keeps its predecessor's pose).  Both are written to profiles/online_slam_small.json when OLSR_WRITE_PROFILES=1."""
    from online_lang_splatting_amd import ate_rmse
    gt = torch.stack([f["w2c"] for f in runs["seq"]])
    ids, est = runs["a"][0].trajectory()
    ids0, est0 = runs["still"][0].trajectory()
    assert ids == ids0 == list(range(FRAMES))
    ate, ate0 = ate_rmse(est, gt), ate_rmse(est0, gt)
    print(f"ATE RMSE: tracked {ate:.6f} m, without tracking iterations {ate0:.6f} m")
    if os.environ.get("OLSR_WRITE_PROFILES") == "1":
        a = runs["a"][0]
        with open(PROFILE, "w") as f:
            json.dump(dict(shape=[W, H], frames=FRAMES, step_deg=STEP_DEG, F=F, ate_rmse_m=ate, ate_rmse_no_tracking_m=ate0,
                           keyframes=a.keyframes, gaussians=a.map.P, loss_kf0_after_init=runs["seen"]["loss_init"],
                           loss_kf0_after_run=runs["seen"]["loss_end"],
                           tracking_iterations=[r["iterations"] for r in runs["a"][1]]), f, indent=1)
    assert ate < ate0


def test_it_maps(runs):
    """6. Keyframe 0's mapping loss (RGB + depth + language L1) after the run is below the same loss right after
    initialize_map; every keyframe of the final window owns Gaussians."""
    seen = runs["seen"]
    print("keyframe 0 loss {total, rgb, depth, language}: after init", seen["loss_init"], "after the run", seen["loss_end"])
    assert seen["loss_end"][0] < seen["loss_init"][0]
    a = runs["a"][0]
    owners = set(torch.unique(a.map.kf_id).cpu().tolist())
    assert set(a.selector.window) <= owners, (a.selector.window, owners)


def test_use_gt_pose(runs):
    """7. With use_gt_pose the given poses come back exactly."""
    slam, results = runs["gt"]
    for f, r in zip(runs["seq"], results):
        assert bits(r["w2c"].cpu()) == bits(f["w2c"].to(torch.float32))
    ids, est = slam.trajectory()
    assert bits(est.cpu()) == bits(torch.stack([f["w2c"] for f in runs["seq"]]))


def test_without_language(runs):
    """8. targets=None and no feature_fn: the same sequence on an F = 0 workspace, no language event."""
    slam, results = runs["plain"]
    assert slam.F == 0 and slam.lanes.lanes[0][0].F == 0 and slam.map.params["language"] is None
    assert not any(e[0] == "language" for e in slam.events) and any(e[0] == "keyframe" for e in slam.events)
    assert any(e[0] == "language" for e in runs["a"][0].events)
    assert slam.render(runs["seq"][0]["w2c"])["language"].numel() == 0


def test_finish_refines(runs):
    """finish(refine_iters): the colour-refinement loop runs on the session's map and keyframes (last: it changes the map)."""
    slam, _ = runs["plain"]
    before = slam.map.params["shs"].clone()
    assert slam.finish(0) is None and bits(before) == bits(slam.map.params["shs"])
    loss = slam.finish(refine_iters=3)
    assert loss is not None and bool(torch.isfinite(loss).all())
    assert bits(before) != bits(slam.map.params["shs"]) and slam.map.P == before.shape[0]
