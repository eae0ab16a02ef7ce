"""Generates tests/golden/pose_wide.npz: ONE pose update of the reference per case of tests/pose_ref.all_cases(), run here on
its importable Python (utils/pose_utils.update_pose, utils/camera_utils.Camera.update_RT and the three camera properties).  The
increments are set to the case's tau directly (the Adam half is pinned elsewhere), so no error accumulates: one step each.
Runs ONLY in the authoring container (needs /root/reference); the committed .npz is data: inputs (start R and T, the index of
the projection matrix, tau) and, per case, what the reference computes in float32 (`ref32_*`) and what the same functions
compute on float64 tensors from the same float32 inputs (`truth_*`).  The case whose state has a wrong last row is left out:
the reference rebuilds T_w2c from R and T and never sees that row."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
import pose_ref  # noqa: E402
from utils.camera_utils import Camera  # noqa: E402
from utils.pose_utils import update_pose  # noqa: E402

KEYS = ("R", "T", "view", "full", "campos", "converged")


def one_step(case, dtype):
    torch.set_default_dtype(dtype)   # the reference's torch.eye / torch.zeros follow it
    T0 = torch.from_numpy(pose_ref.start_poses()[case.pose]).to(dtype)
    proj = torch.from_numpy(pose_ref.projections()[case.proj]).to(dtype)
    cam = Camera(0, None, None, torch.eye(4), proj, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1, 1, device="cpu")
    cam.update_RT(T0[:3, :3].contiguous(), T0[:3, 3].contiguous())
    tau = torch.from_numpy(case.tau).to(dtype)
    with torch.no_grad():
        cam.cam_trans_delta.data.copy_(tau[:3])
        cam.cam_rot_delta.data.copy_(tau[3:])
        conv = update_pose(cam)
        out = dict(R=cam.R, T=cam.T, view=cam.world_view_transform, full=cam.full_proj_transform, campos=cam.camera_center)
        out = {k: v.clone().numpy() for k, v in out.items()}
    out["converged"] = np.array(bool(conv))
    assert all(v.dtype == (np.float32 if dtype == torch.float32 else np.float64) for k, v in out.items() if k != "converged")
    return out


cases = [c for c in pose_ref.all_cases() if c.cls != "last_row"]
rec = {f"{p}_{k}": [] for p in ("ref32", "truth") for k in KEYS}
for c in cases:
    for prefix, dtype in (("ref32", torch.float32), ("truth", torch.float64)):
        for k, v in one_step(c, dtype).items():
            rec[f"{prefix}_{k}"].append(v)
torch.set_default_dtype(torch.float32)
out = {k: np.stack(v) for k, v in rec.items()}
out["names"] = np.array([c.name for c in cases])
out["classes"] = np.array([c.cls for c in cases])
out["tau"] = np.stack([c.tau for c in cases])
out["proj_index"] = np.array([c.proj for c in cases], dtype=np.int32)
out["R0"] = np.stack([pose_ref.start_poses()[c.pose][:3, :3] for c in cases])
out["T0"] = np.stack([pose_ref.start_poses()[c.pose][:3, 3] for c in cases])
np.savez_compressed(os.path.join(HERE, "pose_wide.npz"), **out)
print("wrote pose_wide.npz:", len(cases), "cases,", sum(v.nbytes for v in out.values()), "bytes of arrays")
