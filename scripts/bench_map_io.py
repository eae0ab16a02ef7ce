"""Times the map's PLY record on the GPU; prints one JSON line and writes profiles/map_io_bench.json.

The workload: a map of --gaussians rows (default 500 000), F = 15, at M = 1 (width 32, the session's map) and M = 16 (width
77, the reference's full spherical harmonics).  Per M:
  pack / unpack         olsr_map_ply_pack / olsr_map_ply_unpack, each between its own pair of device events, medians of --reps
                        (30) after warm-up, alternating with
  torch_pack / _unpack  the same statement in torch ops on the device: torch.cat of the seven pieces with the transpose; seven
                        column slices with the transpose back, copied into the map's arrays
  device_copy           rows.clone(): a device copy of the record array, the same 2 P width 4 bytes of traffic
The kernels move bytes = 2 P width 4 (read once, written once); `hbm_share` is bytes / time over 6.3 TB/s, the achievable HBM
rate (8 TB/s peak); at M = 1 the 128 MB of traffic fit the 256 MiB Infinity Cache, so that row is a cache-resident rate.
  save_ply / load_ply   GaussianMap.save_ply / load_ply end to end on the host clock (each ends in a device synchronise), to and
                        from --dir (default: the system's temporary directory), medians of --file-reps (5)
  reference_save / _load  the reference's statements restated in numpy and torch: seven .cpu().numpy() copies, np.concatenate,
                        `elements[:] = list(map(tuple, attributes))`, the structured array to the file; np.fromfile of the
                        structured array, load_ply's per-name column copies, seven torch.tensor(..., device="cuda").  The
                        per-row tuple list runs ONCE on a 20 000-row slice and its time is SCALED by P / 20 000
                        (`tuple_list_scaled`: true); everything else runs at full size.  plyfile itself is not used.
Nothing is asserted: the numbers are what they are.
usage: bench_map_io.py [--reps N] [--warmup N] [--file-reps N] [--gaussians P] [--dir DIR] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--file-reps", type=int, default=5)
ap.add_argument("--gaussians", type=int, default=500_000)
ap.add_argument("--dir", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_io_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_map_io.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd import map_io  # noqa: E402
from online_lang_splatting_amd._host import stream_ptr  # noqa: E402
from online_lang_splatting_amd._lib import check, lib  # noqa: E402
from online_lang_splatting_amd.gaussian_map import GaussianMap  # noqa: E402

dev = torch.device("cuda:0")
HBM_ACHIEVABLE = 6.3e12
SLICE = 20_000
LRS = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)
P, F = int(args.gaussians), 15


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def summary(ts, nbytes=None):
    ts = sorted(ts)
    s = {"ms_median": round(statistics.median(ts), 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}
    if nbytes is not None:
        rate = nbytes / (statistics.median(ts) * 1e-3)
        s["GB_per_s"] = round(rate / 1e9, 1)
        s["hbm_share"] = round(rate / HBM_ACHIEVABLE, 3)
    return s


def host_clock(fn, reps):
    ts = []
    for _ in range(reps + 1):                 # (the first run warms the file system and the pinned allocations up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return summary(ts[1:])


def torch_pack(p, M):
    n = p["means3D"].shape[0]
    return torch.cat([p["means3D"], torch.zeros_like(p["means3D"]), p["shs"][:, :1].transpose(1, 2).flatten(start_dim=1),
                      p["shs"][:, 1:].transpose(1, 2).flatten(start_dim=1), p["language"], p["opacities"].reshape(n, 1),
                      p["scales"], p["rotations"]], dim=1)


def torch_unpack(rows, p, M):
    n = rows.shape[0]
    r = 3 * (M - 1)
    p["means3D"].copy_(rows[:, 0:3])
    p["shs"][:, :1].copy_(rows[:, 6:9].reshape(n, 3, 1).transpose(1, 2))
    if r:
        p["shs"][:, 1:].copy_(rows[:, 9:9 + r].reshape(n, 3, M - 1).transpose(1, 2))
    p["language"].copy_(rows[:, 9 + r:9 + r + F])
    p["opacities"].copy_(rows[:, 9 + r + F:10 + r + F])
    p["scales"].copy_(rows[:, 10 + r + F:13 + r + F])
    p["rotations"].copy_(rows[:, 13 + r + F:17 + r + F])


def reference_save(gm, path):
    """save_ply's statements (gaussian_model.py:509-563); -> the seconds the tuple list took on its slice, scaled to P."""
    p = gm.params
    xyz = p["means3D"].detach().cpu().numpy()
    normals = np.zeros_like(xyz)
    f_dc = p["shs"][:, :1].detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    f_rest = p["shs"][:, 1:].detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    opacities = p["opacities"].detach().cpu().numpy()
    scale = p["scales"].detach().cpu().numpy()
    rotation = p["rotations"].detach().cpu().numpy()
    dtype_full = [(a, "f4") for a in map_io.attribute_names(gm.M, gm.F)]
    elements = np.empty(xyz.shape[0], dtype=dtype_full)
    f_language = p["language"].detach().cpu().numpy()
    attributes = np.concatenate((xyz, normals, f_dc, f_rest, f_language, opacities, scale, rotation), axis=1)
    n = min(SLICE, attributes.shape[0])
    t0 = time.perf_counter()
    elements[:n] = list(map(tuple, attributes[:n]))
    t_slice = time.perf_counter() - t0
    elements[n:] = elements[:1]               # (the rest of the array is only there to be written)
    with open(path, "wb") as f:
        f.write(map_io.ply_header(xyz.shape[0], gm.M, gm.F))
        elements.tofile(f)
    return t_slice * (attributes.shape[0] / max(n, 1) - 1.0)


def reference_load(path, M):
    """load_ply's statements (:585-689) on the structured array plyfile would hand out."""
    with open(path, "rb") as f:
        n, props, offset = map_io.read_ply_header(f)
    el = np.fromfile(path, dtype=[(name, "<f4") for name, _ in props], offset=offset, count=n)
    xyz = np.stack((np.asarray(el["x"]), np.asarray(el["y"]), np.asarray(el["z"])), axis=1)
    opacities = np.asarray(el["opacity"])[..., np.newaxis]
    features_dc = np.zeros((n, 3, 1))
    for c in range(3):
        features_dc[:, c, 0] = np.asarray(el[f"f_dc_{c}"])
    extra = sorted([q for q, _ in props if q.startswith("f_rest_")], key=lambda x: int(x.split("_")[-1]))
    features_extra = np.zeros((n, len(extra)))
    for i, q in enumerate(extra):
        features_extra[:, i] = np.asarray(el[q])
    features_extra = features_extra.reshape((n, 3, M - 1))
    scales = np.zeros((n, 3))
    rots = np.zeros((n, 4))
    for i in range(3):
        scales[:, i] = np.asarray(el[f"scale_{i}"])
    for i in range(4):
        rots[:, i] = np.asarray(el[f"rot_{i}"])
    t = lambda a: torch.tensor(a, dtype=torch.float, device="cuda")  # noqa: E731
    return (t(xyz), t(features_dc).transpose(1, 2).contiguous(), t(features_extra).transpose(1, 2).contiguous(), t(opacities),
            t(scales), t(rots))


out = {"what": "the map's point_cloud.ply record: pack / unpack kernels against torch ops and a device copy; save_ply / load_ply "
               "end to end against the reference's statements restated in numpy (the per-row tuple list scaled from a slice)",
       "reps": args.reps, "warmup": args.warmup, "file_reps": args.file_reps, "device": torch.cuda.get_device_name(0),
       "gaussians": P, "F": F, "hbm_achievable_TB_per_s": HBM_ACHIEVABLE / 1e12, "tuple_list_scaled": True,
       "tuple_list_slice_rows": SLICE, "sizes": {}}
tmp = tempfile.mkdtemp(prefix="olsr_map_io_", dir=args.dir)
g = torch.Generator().manual_seed(3)
for M in (1, 16):
    width = map_io.ply_width(M, F)
    gm = GaussianMap(torch.randn(P, 3, generator=g), torch.randn(P, M, 3, generator=g), torch.randn(P, 1, generator=g),
                     torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g), torch.randn(P, F, generator=g), LRS,
                     capacity=P, device=dev)
    back = GaussianMap.blank(P, M, F, LRS, dev, capacity=P)
    rows = map_io.pack_rows(gm)
    col = (C.c_int32 * width)(*range(width))
    dst = back._struct(back._bufs[back._front])
    stream = stream_ptr(back.device)

    def unpack():
        check(lib().olsr_map_ply_unpack(P, M, F, width, col, rows.data_ptr(), C.byref(dst), stream))
    ev = {k: [] for k in ("pack", "unpack", "torch_pack", "torch_unpack", "device_copy")}
    for rep in range(args.warmup + args.reps):
        cur = {"pack": timed(lambda: map_io.pack_rows(gm)), "torch_pack": timed(lambda: torch_pack(gm.params, M)),
               "unpack": timed(unpack), "torch_unpack": timed(lambda: torch_unpack(rows, back.params, M)),
               "device_copy": timed(lambda: rows.clone())}
        if rep >= args.warmup:
            for k, pair in cur.items():
                ev[k].append(pair)
    torch.cuda.synchronize()
    nbytes = 2 * P * width * 4
    res = {k: summary([e0.elapsed_time(e1) for e0, e1 in pairs], nbytes) for k, pairs in ev.items()}
    res["width"], res["bytes_moved"] = width, nbytes
    same = all(torch.equal(back.params[k].view(torch.int32), gm.params[k].view(torch.int32)) for k in gm.params)
    res["unpack_of_pack_is_identity"] = bool(same) and bool(torch.equal(torch_pack(gm.params, M).view(torch.int32), rows.view(torch.int32)))
    path = os.path.join(tmp, f"point_cloud_M{M}.ply")
    res["save_ply"] = host_clock(lambda: gm.save_ply(path), args.file_reps)
    res["load_ply"] = host_clock(lambda: GaussianMap.load_ply(path, LRS, dev, capacity=P), args.file_reps)
    res["file_bytes"] = os.path.getsize(path)
    ref_path = os.path.join(tmp, f"reference_M{M}.ply")
    t0 = time.perf_counter()
    extra = reference_save(gm, ref_path)
    torch.cuda.synchronize()
    res["reference_save"] = {"ms_once_scaled": round((time.perf_counter() - t0 + extra) * 1e3, 1),
                             "ms_tuple_list_scaled": round(extra * 1e3 * P / max(P - SLICE, 1), 1)}
    res["reference_load"] = host_clock(lambda: reference_load(ref_path, M), min(args.file_reps, 3))
    os.remove(path)
    os.remove(ref_path)
    out["sizes"][f"M{M}"] = res
    del gm, back, rows
os.rmdir(tmp)
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(out, indent=1) + "\n")
