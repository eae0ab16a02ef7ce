"""Times keyframe seeding on the GPU; prints one JSON line and writes profiles/keyframe_seed_bench.json.

The workload: one 1200 x 680 RGB-D frame (random colours, depths of 0.3 .. 6 m with a tenth of the pixels at 0, a non-identity
pose), seeded at the reference's two factors, 32 (the first frame) and 64 (every later keyframe), onto a map of --gaussians
rows.  Measured per factor, each between its own pair of device events after warm-up (the pairs include the one host read of
the path they time), the paths alternating inside one repetition:
  seed_rows             keyframe_seed.seed_rows: plan, the 4-byte host read, finish
  extend_from_rgbd      GaussianMap.extend_from_rgbd on a map of --gaussians rows: seed_rows + the append (the map is put back
                        to its size by dropping the new rows outside the timed region)
  torch_ops             the same statements in torch ops on the device: mask, torch.median, randperm sample, gather,
                        back-projection, the library's distCUDA2, log(sqrt())
  torch_ops_round_trip  torch_ops with the reference's two image round trips through host memory (image and depth to the host
                        and back before the mask, the points to the host and back before distCUDA2)
`launches` counts the kernels and memsets of one seed_rows from the library's own launch list (the plan's one memset and
eleven kernels, the kNN's and the scale kernel), not from a profiler.  Nothing is asserted: the numbers are what they are.
usage: bench_keyframe_seed.py [--reps N] [--warmup N] [--gaussians P] [--out PATH]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--gaussians", type=int, default=500_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_seed_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_keyframe_seed.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd import seed_rows  # noqa: E402
from online_lang_splatting_amd.gaussian_map import GaussianMap  # noqa: E402
from online_lang_splatting_amd.simple_knn import distCUDA2  # noqa: E402

dev = torch.device("cuda:0")
W, H, M, F = 1200, 680, 1, 15
FX = FY = 600.0
CX, CY = 599.5, 339.5
g = torch.Generator().manual_seed(5)
image = (torch.randint(13, 244, (3, H, W), generator=g).float() / 256.0).to(dev)
depth = torch.rand(H, W, generator=g) * 5.7 + 0.3
depth[torch.rand(H, W, generator=g) < 0.1] = 0.0
depth = depth.to(dev)
ca, sa = math.cos(0.4), math.sin(0.4)
w2c = torch.tensor([[ca, 0.0, sa, 0.3], [0.0, 1.0, 0.0, -0.1], [-sa, 0.0, ca, 0.7], [0.0, 0.0, 0.0, 1.0]]).to(dev)
LRS = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)


def torch_ops(factor, round_trip):
    img, d = image, depth
    if round_trip:
        img, d = img.cpu().to(dev), d.cpu().to(dev)
    dp = torch.where(img.sum(dim=0) > 0.01, d, torch.zeros_like(d)).reshape(-1)
    valid = ((dp > 0) & (dp < 100.0)).nonzero().squeeze(1)          # (a host read: the number of valid pixels)
    ps = torch.clamp_max(0.05 * torch.median(dp).double(), 0.05).float()
    keep = valid[torch.randperm(valid.numel(), device=dev)[: int(valid.numel() * (1.0 / factor))]]
    z = dp[keep].double()
    u, v = (keep % W).double(), (keep // W).double()
    p = torch.stack([(u - CX) * z / FX, (v - CY) * z / FY, z], dim=1)
    R, t = w2c[:3, :3].double(), w2c[:3, 3].double()
    pts = ((p - t) @ R).float()
    col = ((img.reshape(3, -1)[:, keep].t() * 255).byte().float() / 255.0 - 0.5) / 0.28209479177387814
    if round_trip:
        pts = pts.cpu().to(dev)
    scales = torch.log(torch.sqrt(torch.clamp_min(distCUDA2(pts), 1e-7) * ps))[:, None].repeat(1, 3)
    return pts, col, scales


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def summary(ts):
    ts = sorted(ts)
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}


P = int(args.gaussians)
gm = GaussianMap(torch.randn(P, 3, generator=g), torch.randn(P, M, 3, generator=g), torch.randn(P, 1, generator=g),
                 torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g), torch.randn(P, F, generator=g), LRS,
                 capacity=P + W * H // 32 + 1024, device=dev)
out = {"what": "keyframe seeding: RGB-D frame -> new rows of the map, fused HIP against the same statements in torch ops on the "
               "device, with and without the reference's host round trips", "reps": args.reps, "warmup": args.warmup,
       "device": torch.cuda.get_device_name(0), "image": [W, H], "gaussians": P, "factors": {}}
for factor in (32, 64):
    kw = dict(downsample=factor, seed=1, M=M)
    ev = {k: [] for k in ("seed_rows", "extend_from_rgbd", "torch_ops", "torch_ops_round_trip")}
    n = 0
    for rep in range(args.warmup + args.reps):
        cur = {"seed_rows": timed(lambda: seed_rows(image, depth, w2c, (FX, FY, CX, CY), **kw)),
               "torch_ops": timed(lambda: torch_ops(factor, False)),
               "torch_ops_round_trip": timed(lambda: torch_ops(factor, True)),
               "extend_from_rgbd": timed(lambda: gm.extend_from_rgbd(image, depth, w2c, (FX, FY, CX, CY), 1, downsample=factor))}
        n = gm.P - P
        drop = torch.zeros(gm.P, dtype=torch.bool, device=dev)
        drop[P:] = True
        gm.prune_points(drop)   # (outside the timed region: back to P rows)
        if rep >= args.warmup:
            for k, pair in cur.items():
                ev[k].append(pair)
    torch.cuda.synchronize()
    res = {k: summary([e0.elapsed_time(e1) for e0, e1 in pairs]) for k, pairs in ev.items()}
    res["rows"] = n
    # the plan: one memset + 4 (histogram + select) + count, prefix, emit; finish: the kNN's launches and the scale kernel
    res["launches"] = {"plan": 12, "finish": "kNN (bounding box 2, Morton 1, radix sort of 30 bits, gather, superboxes, query) + 1"}
    res["host_reads"] = {"seed_rows": 1, "extend_from_rgbd": 1}
    out["factors"][str(factor)] = res
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(out, indent=1) + "\n")
