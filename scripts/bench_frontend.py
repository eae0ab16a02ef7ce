"""Times the front end's frame step on the GPU; prints one JSON line and writes profiles/frontend_bench.json.

The workload: one 1200 x 680 frame, a map of --gaussians rows, a full window of --window keyframes.  Rows, medians of --reps
after warm-up, both sides in the same run, alternating inside one repetition:
  tracking_mask_blocks / _global   frontend.tracking_mask, between device events
  observe                          KeyframeSelector.observe end to end — median depth, covisibility, decision and its one
                                   host read — between device events and, since it ends with a host read, on the host clock
  torch_*                          the same statements in torch ops on the device: the 32 x 32 Python loop over image blocks
                                   (median, compare, two masked writes per block), boolean gather + median, count_nonzero per
                                   window keyframe, 4 x 4 inverses, the .item() reads — on the host clock around a synchronise,
                                   since their cost is host-side
`share_of_tracking_frame`: each time against 100 dependent tracking iterations at the 0.30 and 0.50 ms the README states for
the room map (not measured by this script).  Nothing is asserted: the numbers are what they are.
usage: bench_frontend.py [--reps N] [--warmup N] [--gaussians P] [--window K] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--gaussians", type=int, default=500_000)
ap.add_argument("--window", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontend_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_frontend.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd import KeyframeSelector, tracking_mask  # noqa: E402

dev = torch.device("cuda:0")
W, H, P, K = 1200, 680, int(args.gaussians), int(args.window)
EDGE, KT, KMT, KO, KC = 4.0, 0.08, 0.05, 0.9, 0.4
g = torch.Generator().manual_seed(7)
image = (torch.randint(0, 256, (3, H, W), generator=g).float() / 255.0).to(dev)
depth = (torch.rand(1, H, W, generator=g) * 5.7 + 0.3).to(dev)
opacity = (0.9 + 0.1 * torch.rand(1, H, W, generator=g)).to(dev)
n_touched = (torch.randint(0, 5, (P,), generator=g) * (torch.rand(P, generator=g) < 0.7)).to(torch.int32).to(dev)
vis = [(torch.rand(P, generator=g) < 0.6).to(dev) for _ in range(K)]


def pose(i):
    T = torch.eye(4)
    T[:3, 3] = torch.tensor([0.3 * i, 0.1 * (i % 3), 0.05 * i])
    return T.to(dev)


poses = [pose(i + 1) for i in range(K)]
cur_pose = pose(0)
SCHARR_V = torch.tensor([[3., 10., 3.], [0., 0., 0.], [-3., -10., -3.]], device=dev).view(1, 1, 3, 3)
SCHARR_H = torch.tensor([[3., 0., -3.], [10., 0., -10.], [3., 0., -3.]], device=dev).view(1, 1, 3, 3)
ONES = torch.ones(1, 1, 3, 3, device=dev)


def torch_intensity():
    gray = image.mean(dim=0, keepdim=True)
    p = F.pad(gray, (1, 1, 1, 1), mode="reflect")[None]
    gv, gh = F.conv2d(p, SCHARR_V) / 32.0, F.conv2d(p, SCHARR_H) / 32.0
    ok = F.conv2d((p.abs() > 0.01).float(), ONES) == 9.0
    return torch.sqrt((gv * ok) ** 2 + (gh * ok) ** 2)[0]


def torch_mask_blocks():
    I = torch_intensity()
    bh, bw = H // 32, W // 32
    for r in range(32):
        for c in range(32):
            block = I[:, r * bh:(r + 1) * bh, c * bw:(c + 1) * bw]
            th = block.median() * EDGE
            block[block > th] = 1
            block[block <= th] = 0
    return I


def torch_mask_global():
    I = torch_intensity()
    return I > I.median() * EDGE


def rel_t(A, B):
    return torch.norm((A @ torch.linalg.inv(B))[0:3, 3])


def torch_observe():
    valid = torch.logical_and(depth > 0, opacity > 0.95)
    median = depth[valid].median()
    cur = (n_touched > 0).long()
    dist = rel_t(cur_pose, poses[0])
    union = torch.logical_or(cur, vis[0]).count_nonzero()
    inter = torch.logical_and(cur, vis[0]).count_nonzero()
    ratio = inter / union
    create = bool((ratio < KO and dist > KMT * median) or dist > KT * median)
    window, to_remove = [-1] + list(range(K)), []
    for i in range(2, len(window)):
        k = window[i]
        inter = torch.logical_and(cur, vis[k]).count_nonzero()
        if inter / min(cur.count_nonzero(), vis[k].count_nonzero()) <= KC:
            to_remove.append(k)
    if to_remove:
        window.remove(to_remove[-1])
    if len(window) > K:
        scores = []
        for i in range(2, len(window)):
            inv = [1.0 / (rel_t(poses[window[i]], poses[window[j]]) + 1e-6).item() for j in range(2, len(window)) if j != i]
            scores.append(torch.sqrt(rel_t(poses[window[i]], cur_pose)).item() * sum(inv))
        window.remove(window[2 + max(range(len(scores)), key=scores.__getitem__)])
    return create, window


sel = KeyframeSelector(K, 4, KT, KMT, KO, KC)
for i in reversed(range(K)):
    sel.add_keyframe(100 - 3 * i, poses[i], vis[i])
saved = (list(sel.window), dict(sel.visibility), dict(sel.poses))


def observe():
    r = sel.observe(104, n_touched, cur_pose, depth, opacity)
    sel.window, sel.visibility, sel.poses = list(saved[0]), dict(saved[1]), dict(saved[2])   # (a created keyframe is put back)
    return r


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


rows = {"tracking_mask_blocks": (device_ms, lambda: tracking_mask(image, EDGE, "blocks")),
        "tracking_mask_global": (device_ms, lambda: tracking_mask(image, EDGE, "global")),
        "observe": (device_ms, observe), "observe_host_clock": (host_ms, observe),
        "tracking_mask_blocks_host_clock": (host_ms, lambda: tracking_mask(image, EDGE, "blocks")),
        "torch_mask_blocks": (host_ms, torch_mask_blocks), "torch_mask_global": (host_ms, torch_mask_global),
        "torch_observe": (host_ms, torch_observe)}
ts = {k: [] for k in rows}
for rep in range(args.warmup + args.reps):
    for k, (clock, fn) in rows.items():
        t = clock(fn)
        if rep >= args.warmup:
            ts[k].append(t)
out = {"what": "the front end's frame step: tracking mask, median depth, keyframe test and window policy, fused HIP against the "
               "same statements in torch ops on the device", "reps": args.reps, "warmup": args.warmup,
       "device": torch.cuda.get_device_name(0), "image": [W, H], "gaussians": P, "window": K, "rows": {}}
for k, v in ts.items():
    v = sorted(v)
    med = statistics.median(v)
    out["rows"][k] = {"ms_median": round(med, 4), "ms_min": round(v[0], 4), "ms_max": round(v[-1], 4),
                      "clock": "host" if rows[k][0] is host_ms else "device events",
                      "share_of_tracking_frame": {"at_0.30_ms_per_iteration": round(med / 30.0, 4),
                                                  "at_0.50_ms_per_iteration": round(med / 50.0, 4)}}
out["host_reads"] = {"observe": 1, "tracking_mask": 0}
print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(out, indent=1) + "\n")
