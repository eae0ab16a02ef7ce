"""Times TSDF fusion of rendered language maps on the GPU; prints one JSON line and writes profiles/tsdf_bench.json.

The workload: a volume of 400 x 150 x 250 (x, y, z) 2 cm voxels around scene.make_room_scene's 7 x 2.8 x 5 m room, 15
feature channels, fused from 12 keyframe views rendered at 1200 x 680 by the rasteriser (language [15,H,W], depth, opacity: device tensors, as
TSDFVolume.integrate_render takes them).  Measured, each between its own pair of device events after warm-up, the fused and
the torch-ops path alternating inside one repetition:
  one_view          TSDFVolume.integrate_views of one view (one launch)
  twelve_singles    twelve launches of one view each
  batch_of_twelve   one launch of twelve views: the volume is read and written once per touched voxel, not twelve times
  extraction        TSDFVolume.surface_points (count, prefix, the 4-byte host read, emit), on a host clock around a synchronise
  mesh              TSDFVolume.get_mesh on the same fused volume (count, prefix, the 16-byte host read, emit: the same vertices,
                    their normals and the faces), on the same clock, alternating with `extraction` inside one repetition
  torch_ops_one_view / torch_ops_twelve_views
                    the same update written in torch ops on the device, vectorised over the voxels like the reference's CPU
                    path (tsdf-fusion/fusion.py:250-293) with the 15 channels of fusion3.py
Bytes per the touched-voxel model: a voxel some view of a launch reaches costs one read and one write of its 2 + F floats;
the images are read once (H W (2 + F) floats per view).  The two extractions: the distance of every voxel is read once per pass
(the neighbours a voxel looks at are its block's or the next rows': cache hits), surface_points makes two such passes, get_mesh
one and then writes and reads back 4 bytes per voxel; a point costs its 3 + F floats and its index written and F floats read, a
vertex 3 floats more (the normal), a face 12 bytes.  `share_of_8_TBps` is those bytes over the median time over the
8 TB/s HBM peak of the data sheet (a float4 copy measures 6.3 TB/s on this part).  Nothing is asserted: the numbers are
what they are, and whether the batch beats twelve launches is one of them; the mesh pass contains the point pass, so
`mesh_over_extraction` is the finding there.
usage: bench_tsdf.py [--reps N] [--warmup N] [--gaussians P] [--out PATH]"""
import argparse
import json
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--gaussians", type=int, default=500_000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_tsdf.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd import render  # noqa: E402
from online_lang_splatting_amd.scene import make_room_scene, world2view2  # noqa: E402
from online_lang_splatting_amd.tsdf import TSDFVolume  # noqa: E402

dev = torch.device("cuda:0")
W, H, F, V = 1200, 680, 15, 12
DIM, VOXEL = (400, 150, 250), 0.02   # x, y, z: the room is 7 x 2.8 x 5 m
HBM_PEAK = 8.0e12


def rendered_views():
    rs = make_room_scene(args.gaussians, W, H, F, views=V, seed=3)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False)
    sc = rs.scene
    leaf = lambda t: t.to(dev)  # noqa: E731
    pc = SimpleNamespace(get_xyz=leaf(sc.means3D), get_opacity=leaf(sc.opacities), get_rotation=leaf(sc.rotations),
                         get_scaling=leaf(sc.scales), get_features=leaf(sc.shs), get_language_features=leaf(sc.language),
                         active_sh_degree=sc.sh_degree, max_sh_degree=int(math.isqrt(sc.shs.shape[1])) - 1, is_language=True)
    frames = []
    with torch.no_grad():
        for cam in rs.cameras:
            view = SimpleNamespace(FoVx=2 * math.atan(cam.tanfovx), FoVy=2 * math.atan(cam.tanfovy), image_height=H, image_width=W,
                                   world_view_transform=cam.world_view_transform.to(dev),
                                   full_proj_transform=cam.full_proj_transform.to(dev),
                                   projection_matrix=cam.projection_matrix.to(dev), camera_center=cam.camera_center.to(dev),
                                   cam_rot_delta=torch.zeros(3, device=dev), cam_trans_delta=torch.zeros(3, device=dev))
            pkg = render(view, pc, pipe, sc.bg.to(dev))
            K = np.array([[cam.fx, 0.0, cam.cx], [0.0, cam.fy, cam.cy], [0.0, 0.0, 1.0]])
            frames.append(TSDFVolume.render_view({k: pkg[k].detach().clone() for k in ("language", "depth", "opacity")}, K,
                                                 world2view2(cam.R, cam.T).numpy(), min_opacity=0.5))
    return frames


class TorchOps:
    """The same update in torch ops on the device, float32, vectorised over the voxels."""

    def __init__(self, vol):
        X, Y, Z = vol.vol_dim
        g = torch.meshgrid(torch.arange(X, device=dev), torch.arange(Y, device=dev), torch.arange(Z, device=dev), indexing="ij")
        origin = torch.from_numpy(vol.vol_origin).to(dev)
        self.pts = origin + torch.stack([c.reshape(-1) for c in g], dim=1).float() * VOXEL
        self.trunc = vol.trunc_margin
        n = X * Y * Z
        self.tsdf, self.weight = torch.ones(n, device=dev), torch.zeros(n, device=dev)
        self.feat = torch.zeros(F, n, device=dev)

    @torch.no_grad()
    def integrate(self, f):
        K, pose = f["cam_intr"], torch.from_numpy(np.asarray(f["cam_pose"], dtype=np.float32)).to(dev)
        depth, lang, opacity = f["depth_im"].reshape(-1), f["color_im"].reshape(F, -1), f["opacity"].reshape(-1)
        cam = (self.pts - pose[:3, 3]) @ pose[:3, :3]
        z = cam[:, 2]
        px = torch.round(float(K[0, 0]) * (cam[:, 0] / z) + float(K[0, 2]))
        py = torch.round(float(K[1, 1]) * (cam[:, 1] / z) + float(K[1, 2]))
        valid = (z > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        pix = torch.where(valid, py * W + px, torch.zeros_like(px)).long()
        d = depth[pix]
        diff = d - z
        valid &= (d != 0) & ~(opacity[pix] < f["min_opacity"]) & (diff >= -self.trunc)
        idx = valid.nonzero().squeeze(1)
        obs = float(f["obs_weight"])
        dist = torch.clamp_max(diff[idx] / self.trunc, 1.0)
        w_old = self.weight[idx]
        w_new = w_old + obs
        self.weight[idx] = w_new
        self.tsdf[idx] = (self.tsdf[idx] * w_old + obs * dist) / w_new
        self.feat[:, idx] = (self.feat[:, idx] * w_old + obs * lang[:, pix[idx]]) / w_new


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def summary(ts):
    ts = sorted(ts)
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


frames = rendered_views()
extent = np.array(DIM) * VOXEL
lo = -0.5 * extent                                   # the volume centred on the room (8 x 3 x 5 m around 7 x 2.8 x 5 m)
bnds = np.stack([lo, lo + (np.array(DIM) - 0.5) * VOXEL], axis=1)
n_vox = int(np.prod(DIM))


def fresh():
    return TSDFVolume(bnds, VOXEL, feature_dim=F, device=dev)


# what each launch touches (fresh volumes, so weight > 0 marks exactly the voxels a launch stored)
touched_single = []
for f in frames:
    v = fresh()
    v.integrate_views([f])
    touched_single.append(int((v.weight > 0).sum()))
    del v
vol = fresh()
assert vol.vol_dim == DIM
vol.integrate_views(frames)
touched_batch = int((vol.weight > 0).sum())
ref = TorchOps(vol)
for f in frames:
    ref.integrate(f)
torch.cuda.synchronize()
tsdf = vol.get_volume()[0].reshape(-1)
same = {"voxels_with_a_different_weight": int((vol.weight.reshape(-1) != ref.weight).sum()),
        "tsdf_max_abs_difference": float((tsdf - ref.tsdf)[vol.weight.reshape(-1) == ref.weight].abs().max())}

voxel_bytes, image_bytes = 2 * (2 + F) * 4, H * W * (2 + F) * 4
model = {"one_view": touched_single[0] * voxel_bytes + image_bytes,
         "twelve_singles": sum(touched_single) * voxel_bytes + V * image_bytes,
         "batch_of_twelve": touched_batch * voxel_bytes + V * image_bytes}

ev = {k: [] for k in ("one_view", "twelve_singles", "batch_of_twelve", "torch_ops_one_view", "torch_ops_twelve_views")}
extraction, mesh_ms = [], []
for rep in range(args.warmup + args.reps):
    cur = {"one_view": timed(lambda: vol.integrate_views(frames[:1])),
           "torch_ops_one_view": timed(lambda: ref.integrate(frames[0])),
           "twelve_singles": timed(lambda: [vol.integrate_views([f]) for f in frames]),
           "torch_ops_twelve_views": timed(lambda: [ref.integrate(f) for f in frames]),
           "batch_of_twelve": timed(lambda: vol.integrate_views(frames))}
    ms, cloud = host_timed(vol.surface_points)
    ms_mesh, mesh = host_timed(vol.get_mesh)
    if rep >= args.warmup:
        for k, pair in cur.items():
            ev[k].append(pair)
        extraction.append(ms)
        mesh_ms.append(ms_mesh)
torch.cuda.synchronize()

out = {"what": "TSDF fusion of rendered language maps: fused HIP (one launch per batch of views) against the same update in "
               "torch ops on the device, float32", "reps": args.reps, "warmup": args.warmup,
       "device": torch.cuda.get_device_name(0), "volume": list(DIM), "voxel_size": VOXEL, "voxels": n_vox, "image": [W, H],
       "F": F, "views": V, "gaussians": int(args.gaussians), "touched_voxels_per_single_view": touched_single,
       "touched_voxels_batch": touched_batch, "surface_points": int(cloud[0].shape[0]), "hbm_peak_bytes_per_s": HBM_PEAK,
       "fused_against_torch_ops": same}
for k, pairs in ev.items():
    out[k] = summary([a.elapsed_time(b) for a, b in pairs])
    if k in model:
        out[k]["model_bytes"] = model[k]
        out[k]["model_TBps"] = round(model[k] / (out[k]["ms_median"] * 1e-3) / 1e12, 3)
        out[k]["share_of_8_TBps"] = round(model[k] / (out[k]["ms_median"] * 1e-3) / HBM_PEAK, 4)
n_points, n_faces = int(cloud[0].shape[0]), int(mesh[1].shape[0])
assert int(mesh[0].shape[0]) == n_points and torch.equal(mesh[0], cloud[0])
point_bytes = (3 + F) * 4 + 4 + F * 4
model.update(extraction=2 * 4 * n_vox + n_points * point_bytes,
             mesh=3 * 4 * n_vox + n_points * (point_bytes + 3 * 4) + n_faces * 3 * 4)
for k, ts in (("extraction", extraction), ("mesh", mesh_ms)):   # (host clock: the launches, the host read and the allocations included)
    out[k] = summary(ts)
    out[k]["model_bytes"] = model[k]
    out[k]["model_TBps"] = round(model[k] / (out[k]["ms_median"] * 1e-3) / 1e12, 3)
out["mesh"].update(vertices=n_points, faces=n_faces)
out["mesh_over_extraction"] = round(out["mesh"]["ms_median"] / out["extraction"]["ms_median"], 4)
out["batch_over_twelve_singles"] = round(out["batch_of_twelve"]["ms_median"] / out["twelve_singles"]["ms_median"], 4)
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fo:
    fo.write(json.dumps(out, indent=1) + "\n")
