"""Times the point-cloud metrics (cloud_metrics.emd_segments / chamfer_segments) on the GPU; prints one JSON line and writes
profiles/cloud_metrics_bench.json.

Cases: EMD and Chamfer at n = m in {4 096, 16 384, 65 536} with one segment, and a ten-segment ragged batch (segments of 500 ..
20 000 points, the sizes of the evaluation's per-class clouds after its stride of 8) in one call.  Clouds are seeded uniform
points in a 4 x 3 x 2.5 m box, the second cloud the first plus 1 cm noise.

Baseline: the same statements in torch ops on the device with the dense [n,m] arrays (float32), at the sizes whose dozen or so
[n,m] temporaries fit comfortably (4 096 and 16 384; the batch runs segment by segment).  The reference's OWN kernel
(PyTorchEMD's approxmatch / matchcost) is CUDA only and cannot run on this hardware, and its Chamfer is sklearn's kd-tree on the
host: neither is timed here, and no figure below is a comparison with them.

Per case: milliseconds between device events around the whole call after warm-up (median, min, max — the call includes the
host's checks and the upload of the offsets), the peak device memory above what the inputs hold (torch's allocator), and pair
evaluations per second: n * m per Chamfer direction (2 n m in all), 30 n m for the EMD (three all-pairs walks per level, ten
levels), computed from the shapes.  The fused and the torch results are compared at the sizes both run.

usage: bench_cloud_metrics.py [--reps N] [--warmup N] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_metrics_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_cloud_metrics.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd import cloud_metrics as M  # noqa: E402

dev = torch.device("cuda:0")
SIZES = (4096, 16384, 65536)
DENSE_MAX = 16384
RAGGED = (500, 1200, 2500, 3100, 4096, 5000, 7777, 9000, 12000, 20000)
LEVELS = [-(4.0 ** j) for j in range(7, -2, -1)] + [0.0]


def clouds(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.random((n, 3), dtype=np.float32) * np.array([4.0, 3.0, 2.5], np.float32)
    b = a + rng.normal(0.0, 0.01, (n, 3)).astype(np.float32)
    return torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)


def torch_dist2(x1, x2):
    dx, dy, dz = (x2[None, :, k] - x1[:, None, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def torch_emd(x1, x2):
    d = torch_dist2(x1, x2)
    n, m = d.shape
    multiL, multiR = (1, n // m) if n >= m else (m // n, 1)
    remainL, remainR = torch.full((n,), float(multiL), device=dev), torch.full((m,), float(multiR), device=dev)
    cost = torch.zeros((), dtype=torch.float64, device=dev)
    for level in LEVELS:
        e = torch.exp(level * d)
        ratioL = remainL / (1e-9 + (e * remainR[None, :]).sum(1))
        sumr = (e * ratioL[:, None]).sum(0) * remainR
        ratioR = torch.clamp(remainR / (sumr + 1e-9), max=1.0) * remainR
        remainR = torch.clamp(remainR - sumr, min=0.0)
        w = e * ratioL[:, None] * ratioR[None, :]
        cost += (d * w).sum(1).double().sum()
        remainL = torch.clamp(remainL - w.sum(1), min=0.0)
    return cost / n


def torch_chamfer(x, y):
    d = torch_dist2(x, y)
    return d.min(1).values.double().sqrt().mean() + d.min(0).values.double().sqrt().mean()


def measure(fn):
    """-> (summary of the milliseconds, peak bytes above the start, the last result)."""
    ts, peak, out = [], 0, None
    for rep in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        if rep >= args.warmup:
            ts.append(a.elapsed_time(b))
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
    ts.sort()
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
            "peak_bytes": int(peak)}, out


def rate(entry, pairs):
    entry["pair_evaluations"] = int(pairs)
    entry["pair_evaluations_per_s"] = float(f"{pairs / (entry['ms_median'] * 1e-3):.4g}")
    return entry


out = {"what": "point-cloud metrics: fused HIP (matrix-free EMD, brute-force Chamfer, ragged batches) against the same statements "
               "in torch ops with dense [n,m] arrays on the device, float32; the reference's own CUDA kernel cannot run here and "
               "is not part of any figure", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
       "launches_per_emd_call": 23, "launches_per_chamfer_call": 2, "cases": {}}
for n in SIZES:
    x, y = clouds(n, n)
    off = [0, n]
    case = {}
    s, emd = measure(lambda: M.emd_segments(x, off, y, off, return_residual=True))
    case["emd"] = rate(s, 30 * n * n)
    case["emd"]["value"], case["emd"]["residual"] = float(emd[0][0]), [float(v) for v in emd[1][0]]
    s, mean = measure(lambda: M.chamfer_segments(x, off, y, off)[0])
    case["chamfer"] = rate(s, 2 * n * n)
    case["chamfer"]["value"] = float(mean[0].sum())
    if n <= DENSE_MAX:
        s, ref = measure(lambda: torch_emd(x, y))
        case["emd_torch_dense"] = rate(s, 30 * n * n)
        case["emd_torch_dense"]["value"] = float(ref)
        s, ref = measure(lambda: torch_chamfer(x, y))
        case["chamfer_torch_dense"] = rate(s, 2 * n * n)
        case["chamfer_torch_dense"]["value"] = float(ref)
        case["emd_speedup"] = round(case["emd_torch_dense"]["ms_median"] / case["emd"]["ms_median"], 3)
        case["chamfer_speedup"] = round(case["chamfer_torch_dense"]["ms_median"] / case["chamfer"]["ms_median"], 3)
    else:
        case["emd_torch_dense"] = case["chamfer_torch_dense"] = "not run: the dense [n,m] temporaries do not fit comfortably"
    out["cases"][f"n_{n}"] = case

pairs_xy = [clouds(n, 100 + k) for k, n in enumerate(RAGGED)]
xyz1, xyz2 = torch.cat([p[0] for p in pairs_xy]), torch.cat([p[1] for p in pairs_xy])
off = np.concatenate([[0], np.cumsum(RAGGED)])
nm = sum(n * n for n in RAGGED)
case = {"segments": list(RAGGED)}
s, emd = measure(lambda: M.emd_segments(xyz1, off, xyz2, off))
case["emd"] = rate(s, 30 * nm)
s, mean = measure(lambda: M.chamfer_segments(xyz1, off, xyz2, off)[0])
case["chamfer"] = rate(s, 2 * nm)
s, ref = measure(lambda: torch.stack([torch_emd(a, b) for a, b in pairs_xy]))
case["emd_torch_dense"] = rate(s, 30 * nm)
case["emd_max_rel_difference_to_torch"] = float(((emd - ref).abs() / ref.abs()).max())
s, ref = measure(lambda: torch.stack([torch_chamfer(a, b) for a, b in pairs_xy]))
case["chamfer_torch_dense"] = rate(s, 2 * nm)
case["chamfer_max_rel_difference_to_torch"] = float(((mean.sum(1) - ref).abs() / ref.abs()).max())
case["emd_speedup"] = round(case["emd_torch_dense"]["ms_median"] / case["emd"]["ms_median"], 3)
case["chamfer_speedup"] = round(case["chamfer_torch_dense"]["ms_median"] / case["chamfer"]["ms_median"], 3)
out["cases"]["ragged_10"] = case

line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(out, indent=1) + "\n")
