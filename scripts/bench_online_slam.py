"""Runs the online SLAM session (online_lang_splatting_amd.slam.OnlineSlam) on the ray-cast room at 1200 x 680; prints one JSON
line and writes profiles/online_slam_bench.json.

The sequence: --frames poses on scene.room_keyframe_cameras' loop, --step-deg degrees apart (consecutive frames overlap),
ray-cast with scene._raycast_room / _room_colour into uint8 images and uint16 depths, F = 15 code maps from _surface_codes
handed in through feature_fn.  The configuration is the reference's configs/rgbd/replicav2/base_config.yaml with the
iteration counts given on the command line (its own 1050 / 100 / 150 are --init / --tracking / --mapping).
Rows:
  tracked_frames_per_s   tracked frames (keyframes included, their mapping excluded) per second of track() time outside
                         the keyframe handling, host clock around a synchronise
  ms_per_keyframe        seed + mapping + prune of a keyframe, host clock around a synchronise
  ingest_ms / torch_ingest_ms   frontend.ingest_frame against the same statements in torch ops on the device (uint8 -> float64
                         / 255 -> clamp -> permute -> float32; uint16 -> float64 / scale -> float32), medians of --reps between
                         device events, alternating inside one repetition
  ate_rmse_m             slam.ate_rmse of the estimated trajectory against the ray-caster's poses
Nothing is asserted: the numbers are what they are.
usage: bench_online_slam.py [--frames N] [--step-deg D] [--init N] [--tracking N] [--mapping N] [--reps N] [--out PATH]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=12)
ap.add_argument("--step-deg", type=float, default=0.5)
ap.add_argument("--init", type=int, default=300)
ap.add_argument("--tracking", type=int, default=100)
ap.add_argument("--mapping", type=int, default=50)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_slam_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_online_slam.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd import OnlineSlam, ate_rmse, ingest_frame  # noqa: E402
from online_lang_splatting_amd.scene import (ROOM_HALF, Camera, _raycast_room, _room_colour, _surface_codes,  # noqa: E402
                                             world2view2)

dev = torch.device("cuda:0")
W, H, F, SCALE = 1200, 680, 15, 6553.5
CONFIG = {
    "Dataset": {"type": "replica", "pcd_downsample": 64, "pcd_downsample_init": 32, "point_size": 0.05, "adaptive_pointsize": True},
    "Training": {"init_itr_num": args.init, "init_gaussian_update": 100, "init_gaussian_reset": 500, "init_gaussian_th": 0.005,
                 "init_gaussian_extent": 30, "tracking_itr_num": args.tracking, "mapping_itr_num": args.mapping,
                 "gaussian_update_every": 150, "gaussian_update_offset": 50, "gaussian_th": 0.7, "gaussian_extent": 1.0,
                 "gaussian_reset": 2001, "size_threshold": 20, "kf_interval": 4, "window_size": 10, "pose_window": 5,
                 "edge_threshold": 4, "rgb_boundary_threshold": 0.01, "use_gt_pose": False, "kf_translation": 0.04,
                 "kf_min_translation": 0.02, "kf_overlap": 0.95, "prune_mode": "slam", "single_thread": True,
                 "lr": {"cam_rot_delta": 0.003, "cam_trans_delta": 0.001}},
    "opt_params": {"position_lr_init": 0.00016, "position_lr_final": 0.0000016, "position_lr_max_steps": 30000,
                   "feature_lr": 0.0025, "language_lr": 0.0025, "opacity_lr": 0.05, "scaling_lr": 0.001, "rotation_lr": 0.001,
                   "percent_dense": 0.01, "lambda_dssim": 0.2, "densify_from_iter": 500, "densify_grad_threshold": 0.0002},
    "language": {"language_train": True, "single_stage_ae": True, "lang_code_size": F, "labels_from_file": True},
}

codes = _surface_codes(F)
seq = []
for k in range(args.frames):
    a = math.radians(args.step_deg * k)
    R = torch.tensor([[math.cos(a), 0.0, -math.sin(a)], [0.0, 1.0, 0.0], [math.sin(a), 0.0, math.cos(a)]])
    c = torch.tensor([0.9 * math.sin(a) * ROOM_HALF[0] / 3.5, 0.1, 0.9 * math.cos(a) * ROOM_HALF[2] / 3.5])
    cam = Camera(W, H, W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0, R, -(R @ c))
    depth, hitp, sid = _raycast_room(cam, W, H)
    rgb = (_room_colour(hitp, sid) * 255.0).round().clamp(0, 255).to(torch.uint8)
    d16 = (depth.double() * SCALE).round().clamp(0, 65535).to(torch.int32).numpy().astype(np.uint16)
    _, _, sid_l = _raycast_room(cam, 192, 192)
    seq.append(dict(rgb=rgb.contiguous().to(dev), depth=torch.from_numpy(d16).to(dev), w2c=world2view2(cam.R, cam.T),
                    codes=codes[sid_l].permute(2, 0, 1).contiguous().to(dev)))

slam = OnlineSlam(CONFIG, (W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0), H, W, feature_fn=lambda i, image: seq[i]["codes"], device=dev)
kf_clock = {"s": 0.0}
inner = slam._keyframe


def timed_keyframe(*a, **k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    inner(*a, **k)
    torch.cuda.synchronize()
    kf_clock["s"] += time.perf_counter() - t0


slam._keyframe = timed_keyframe
torch.cuda.synchronize()
t0 = time.perf_counter()
slam.track(0, seq[0]["rgb"], seq[0]["depth"], SCALE, gt_w2c=seq[0]["w2c"])
torch.cuda.synchronize()
init_s = time.perf_counter() - t0
track_s, kf_s, kfs = 0.0, [], 0
for k in range(1, args.frames):
    kf_clock["s"] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = slam.track(k, seq[k]["rgb"], seq[k]["depth"], SCALE)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    track_s += dt - kf_clock["s"]
    if r["is_keyframe"]:
        kf_s.append(kf_clock["s"])
ids, est = slam.trajectory()
ate = ate_rmse(est, torch.stack([f["w2c"] for f in seq]))

# ---- the ingest alone, against the same statements in torch ops
rgb, d16 = seq[0]["rgb"], seq[0]["depth"]
out_i, out_d = torch.empty(3, H, W, device=dev), torch.empty(H, W, device=dev)


def torch_ingest():
    image = (rgb.to(torch.float64) / 255.0).clamp(0.0, 1.0).permute(2, 0, 1).to(torch.float32).contiguous()
    return image, (d16.to(torch.float64) / SCALE).to(torch.float32)


def between_events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


for _ in range(5):
    ingest_frame(rgb, d16, SCALE, out_image=out_i, out_depth=out_d)
    torch_ingest()
mine, theirs = [], []
for _ in range(args.reps):
    mine.append(between_events(lambda: ingest_frame(rgb, d16, SCALE, out_image=out_i, out_depth=out_d)))
    theirs.append(between_events(torch_ingest))
ti, td = torch_ingest()
res = dict(shape=[W, H], frames=args.frames, step_deg=args.step_deg, init_itr_num=args.init, tracking_itr_num=args.tracking,
           mapping_itr_num=args.mapping, init_s=round(init_s, 3), tracked_frames_per_s=round((args.frames - 1) / track_s, 3),
           ms_per_keyframe=round(1e3 * statistics.median(kf_s), 2) if kf_s else None, keyframes=slam.keyframes,
           gaussians=slam.map.P, ate_rmse_m=ate, ingest_ms=round(statistics.median(mine), 4),
           torch_ingest_ms=round(statistics.median(theirs), 4),
           ingest_equals_torch=bool(torch.equal(ti, out_i) and torch.equal(td, out_d)),
           tracking_iterations=[e[2] for e in slam.events if e[0] == "track"], device=torch.cuda.get_device_name(0))
print(json.dumps(res))
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
