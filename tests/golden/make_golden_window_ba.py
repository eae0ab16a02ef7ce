"""Generates tests/golden/window_ba.npz: the reference's bundle adjustment of the mapping window, run here on its importable
Python (utils/camera_utils.Camera, utils/pose_utils.update_pose, under the window optimiser the back end sets up at a new
keyframe, utils/slam_backend.py:933-980), and the isotropic regulariser of utils/slam_backend.py:664-667 with autograd.
Runs ONLY in the authoring container (needs /root/reference); the committed .npz is data.

Window: five CPU Cameras, window order uids (0, 3, 5, 8, 11), pose_window = 3 — view 0 is frame 0 (no parameter at all),
views 1-2 optimise pose (half the tracking rates) and exposure, views 3-4 their exposure alone.  Eight iterations of recorded
gradients; after each step of that optimiser the reference calls update_pose on the first pose_window views except uid 0
(:756-765).  Recorded after every iteration, per view: R, T, world_view_transform, full_proj_transform, camera_center,
exposure, and the tau the step applied.

Regulariser: `10 * |scaling - scaling.mean(dim=1)|.mean()` with scaling = exp(_scaling), loss and gradient with respect to
_scaling in float32 and float64, and with respect to scaling itself (the activated form), for the first P rows of one
[4099,3] array (reg_x; reg_s = its float32 exp), P in (1, 63, 64, 65, 257, 4099).  Rows are chosen away from ties (a tie's sign is decided by the last bit of
an exp): a third of them three equal scales, a third two equal and one apart, a third with every |d_k| >= 1e-3 m."""
import math
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
sys.path.insert(0, REF)
from gaussian_splatting.utils.graphics_utils import getProjectionMatrix2, focal2fov  # noqa: E402
from utils.camera_utils import Camera  # noqa: E402
from utils.pose_utils import update_pose  # noqa: E402

g = torch.Generator().manual_seed(20261019)
out = {}
UIDS, POSE_WINDOW, NIT = (0, 3, 5, 8, 11), 3, 8
LR_ROT, LR_TRANS = 0.003, 0.001          # config Training.lr.cam_rot_delta / cam_trans_delta
W, H = 640, 480
fx = fy = W / 2.0
cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
proj = getProjectionMatrix2(znear=0.01, zfar=100.0, fx=fx, fy=fy, cx=cx, cy=cy, W=W, H=H).transpose(0, 1)
cams = []
for v, uid in enumerate(UIDS):
    cam = Camera(uid, None, None, torch.eye(4), proj, fx, fy, cx, cy, focal2fov(fx, W), focal2fov(fy, H), H, W, device="cpu")
    a, b = math.radians(3.0 * v - 4.0), math.radians(1.5 * v)
    Ry = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, math.cos(b), -math.sin(b)], [0.0, math.sin(b), math.cos(b)]])
    cam.update_RT((Rx @ Ry).contiguous(), torch.tensor([0.1 * v, -0.05 * v, 0.02 * v + 0.01]))
    with torch.no_grad():
        cam.exposure_a.fill_(0.01 * v)
        cam.exposure_b.fill_(-0.005 * v)
    cams.append(cam)
out["R0"] = np.stack([c.R.clone().numpy() for c in cams])
out["T0"] = np.stack([c.T.clone().numpy() for c in cams])
out["exposure0"] = np.array([[float(c.exposure_a.detach()), float(c.exposure_b.detach())] for c in cams], dtype=np.float32)

# The window's optimiser, as the back end sets it up at a new keyframe: one Adam; frame 0 contributes nothing, a view in the
# first POSE_WINDOW window positions its two pose increments at half the tracking rates, every view its two exposure terms.
groups = []
for v, cam in enumerate(cams):
    if cam.uid == 0:
        continue
    if v < POSE_WINDOW:
        groups += [{"params": [cam.cam_rot_delta], "lr": 0.5 * LR_ROT}, {"params": [cam.cam_trans_delta], "lr": 0.5 * LR_TRANS}]
    groups += [{"params": [cam.exposure_a], "lr": 0.01}, {"params": [cam.exposure_b], "lr": 0.01}]
window_adam = torch.optim.Adam(groups)
posed = [cam for cam in cams[:POSE_WINDOW] if cam.uid != 0]   # the views whose pose the back end updates after each step

V = len(UIDS)
scale = torch.tensor([10.0 ** (-0.3 * i) for i in range(NIT)]).view(NIT, 1, 1)
gtau = torch.randn(NIT, V, 6, generator=g) * scale   # [rho | theta] per view, as the rasterizer's dL_dtau sums
gexp = torch.randn(NIT, V, 2, generator=g) * scale
rec = {k: [] for k in ("R", "T", "view", "full", "campos", "exposure", "tau")}
for i in range(NIT):
    for v, cam in enumerate(cams):   # the single backward of the iteration leaves a gradient on every camera's parameters
        cam.cam_trans_delta.grad = gtau[i, v, :3].clone()
        cam.cam_rot_delta.grad = gtau[i, v, 3:].clone()
        cam.exposure_a.grad = gexp[i, v, 0:1].clone()
        cam.exposure_b.grad = gexp[i, v, 1:2].clone()
    with torch.no_grad():
        window_adam.step()
        window_adam.zero_grad(set_to_none=True)
        rec["tau"].append(np.stack([torch.cat([c.cam_trans_delta, c.cam_rot_delta]).detach().clone().numpy() for c in cams]))
        for cam in posed:
            update_pose(cam)
    rec["R"].append(np.stack([c.R.clone().numpy() for c in cams]))
    rec["T"].append(np.stack([c.T.clone().numpy() for c in cams]))
    rec["view"].append(np.stack([c.world_view_transform.clone().numpy() for c in cams]))
    rec["full"].append(np.stack([c.full_proj_transform.clone().numpy() for c in cams]))
    rec["campos"].append(np.stack([c.camera_center.clone().numpy() for c in cams]))
    rec["exposure"].append(np.array([[float(c.exposure_a.detach()), float(c.exposure_b.detach())] for c in cams], dtype=np.float32))
out["uids"] = np.array(UIDS)
out["pose_window"] = np.array(POSE_WINDOW)
out["lr"] = np.array([LR_ROT * 0.5, LR_TRANS * 0.5, 0.01])
out["proj"] = np.ascontiguousarray(proj.numpy())
out["grad_tau"] = gtau.numpy()
out["grad_exposure"] = gexp.numpy()
for k, v in rec.items():
    out[k] = np.stack(v)

# ---- the isotropic regulariser ----
PMAX, SIZES, WEIGHT = 4099, (1, 63, 64, 65, 257, 4099), 10.0
x = (torch.randn(PMAX, 3, generator=g) * 0.7 - 4.0)
kind = torch.arange(PMAX) % 3
x[kind == 0] = x[kind == 0][:, :1].expand(-1, 3)                       # three equal scales
two = (kind == 1).nonzero().flatten()
x[two, 1] = x[two, 0]
x[two, 2] = x[two, 0] + torch.where(torch.rand(len(two), generator=g) < 0.5, -1.0, 1.0) * (0.05 + torch.rand(len(two), generator=g))
for r in (kind == 2).nonzero().flatten().tolist():                     # every |d_k| >= 1e-3 m
    while True:
        s = torch.exp(x[r].double())
        if ((s - s.mean()).abs() >= 2e-3 * s.mean()).all():
            break
        x[r] = torch.randn(3, generator=g) * 0.7 - 4.0
x = x.float().contiguous()
out["reg_x"] = x.numpy()
out["reg_s"] = torch.exp(x).numpy()      # the float32 scales the activated form is stated on
out["reg_sizes"] = np.array(SIZES)
out["reg_weight"] = np.array(WEIGHT)


def statement(raw, dtype, activated):
    """WEIGHT times the mean over all 3 P elements of |s - row mean of s|, and its gradient with respect to `raw`."""
    p = raw.to(dtype).clone().requires_grad_(True)
    s = p if activated else torch.exp(p)
    row_mean = s.mean(dim=1, keepdim=True)
    loss = WEIGHT * (s - row_mean).abs().mean()
    loss.backward()
    return loss.detach().numpy(), p.grad.numpy()


# A row of three equal scales has the exact gradient zero although its float32 mean differs from the scale in about 15 % of
# such rows (d_k is then the same non-zero number three times: three equal signs cancel).  Autograd leaves a rounding
# residue there at some P — mean's backward forms (c sg + c sg + c sg) / 3, which is not always c sg — so it is bounded
# here by 4 ulp of c = weight / (3 P) in the statement's own precision, not asserted to be zero.
for P in SIZES:
    for name, dtype in (("32", torch.float32), ("64", torch.float64)):
        out[f"reg_loss{name}_P{P}"], out[f"reg_grad{name}_P{P}"] = statement(x[:P], dtype, False)
    # the activated form: the same statement with respect to scaling = exp(_scaling) as float32 values
    s32 = torch.exp(x[:P])
    for name, dtype in (("32", torch.float32), ("64", torch.float64)):
        out[f"reg_act_loss{name}_P{P}"], out[f"reg_act_grad{name}_P{P}"] = statement(s32, dtype, True)
    eq = (kind[:P] == 0).numpy()
    c = WEIGHT / (3.0 * P)
    for name, ulp in (("32", 2.0 ** -24), ("64", 2.0 ** -53)):
        assert np.abs(out[f"reg_act_grad{name}_P{P}"][eq]).max(initial=0.0) <= 4 * ulp * c
        assert np.abs(out[f"reg_grad{name}_P{P}"][eq]).max(initial=0.0) <= 4 * ulp * c * float(s32.max())
    m_torch = s32.mean(dim=1)
    m_ours = ((s32[:, 0] + s32[:, 1]) + s32[:, 2]) / 3.0
    assert torch.equal(m_torch, m_ours), "torch's mean(dim=1) is not ((s0 + s1) + s2) / 3 on this data"
s = torch.exp(x)
eq = kind == 0
print("rows of equal scales whose float32 mean differs from the scale: %.1f %%" % (100.0 * float((s[eq].mean(dim=1) != s[eq][:, 0]).float().mean())))
dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "window_ba.npz")
np.savez_compressed(dst, **out)
print("wrote", os.path.basename(dst), "with", len(out), "arrays")
