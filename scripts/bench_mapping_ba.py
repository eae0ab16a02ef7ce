"""Cost of mapping's bundle adjustment on the room map (500 k Gaussians, 1200 x 680, 10 window + 2 rehearsal views, one view
in flight with the carried depth order, as scripts/probe/mapping_time.py room 12 1 1):

    python scripts/bench_mapping_ba.py [--reps 30] [--json profiles/mapping_ba_bench.json]

The three variants of the mapping iteration — feature off, window step only, window step + isotropic regulariser — alternate
in ONE process (each on its own copy of the map, the same lanes), every iteration between two device events, medians of
--reps.  On their own, between events as well: the window step (olsr_window_pose_step, 12 views), olsr_isotropic_reg (gradient
and loss), and the same statements in torch ops on the device — torch.optim.Adam over the window's pose increments and
exposures with update_pose's arithmetic per view, and the regulariser under autograd.  No time is fixed in advance: the
figures are reported as measured."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from online_lang_splatting_amd import KeyframeWindow, _abi, losses  # noqa: E402
from online_lang_splatting_amd.frame_shard import FrameLanes  # noqa: E402
from online_lang_splatting_amd.scene import make_room_scene  # noqa: E402
from online_lang_splatting_amd.slam_iterations import MappingStep  # noqa: E402

LRS = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def summary(ms):
    return dict(ms_median=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), n=len(ms))


def torch_window(T_w2c, ids, proj, pose_window):
    """keyframe_optimizers.step() + update_pose in torch ops on the device (utils/slam_backend.py:933-980, :756-765;
    utils/pose_utils.py:26-97)."""
    dev = proj.device
    cams = [dict(T=T.clone(), rot=torch.zeros(3, device=dev, requires_grad=True), trans=torch.zeros(3, device=dev, requires_grad=True),
                 a=torch.zeros(1, device=dev, requires_grad=True), b=torch.zeros(1, device=dev, requires_grad=True)) for T in T_w2c]
    groups = []
    for v, (c, i) in enumerate(zip(cams, ids)):
        if i == 0:
            continue
        if v < pose_window:
            groups += [{"params": [c["rot"]], "lr": 0.0015}, {"params": [c["trans"]], "lr": 0.0005}]
        groups += [{"params": [c["a"]], "lr": 0.01}, {"params": [c["b"]], "lr": 0.01}]
    opt = torch.optim.Adam(groups)
    eye = torch.eye(3, device=dev)

    def skew(w):
        z = torch.zeros((), device=dev)
        return torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])

    # (the gradients are in place before the clock starts, as the fused side's slots are: only parameters of the optimiser)
    for grp in groups:
        for p_ in grp["params"]:
            p_.grad = torch.full_like(p_, 1e-3)

    def step():
        with torch.no_grad():
            opt.step()
            for v, (c, i) in enumerate(zip(cams, ids)):
                if v >= pose_window or i == 0:
                    continue
                Wm = skew(c["rot"])
                W2 = Wm @ Wm
                angle = torch.norm(c["rot"])   # (the reference branches on it on the host: a read-back per view, not taken here)
                R = eye + (torch.sin(angle) / angle) * Wm + ((1 - torch.cos(angle)) / angle ** 2) * W2
                Vm = eye + Wm * ((1 - torch.cos(angle)) / angle ** 2) + W2 * ((angle - torch.sin(angle)) / angle ** 3)
                E = torch.eye(4, device=dev)
                E[:3, :3], E[:3, 3] = R, Vm @ c["trans"]
                c["T"] = E @ c["T"]
                c["rot"].zero_()
                c["trans"].zero_()
                c["view"] = c["T"].t()
                c["full"] = c["view"] @ proj
                c["campos"] = c["view"].inverse()[3, :3]
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "mapping_ba_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    W, H, F, NW = 1200, 680, 15, 10
    rs = make_room_scene(a.P, W, H, F, views=NW, random_views=2, seed=3)
    sc, cams, targets = rs.scene, rs.cameras, rs.targets
    g_dev, _ = bench.device_inputs(sc, cams[0], dev)
    camd = [bench.device_inputs(sc, c, dev)[1] for c in cams]
    R0 = max(bench._sized_capacity(F, g_dev, c, H, W, 0, dev, (15, _abi.BWD_REFERENCE, _abi.BINNING_ELLIPSE)) for c in camd)
    lanes = FrameLanes(1, sc.P, W, H, F, sc.shs.shape[1], int(1.5 * R0) + (1 << 16), dev)

    def fresh():
        return dict(means3D=g_dev["means3D"].clone(), shs=g_dev["shs"].clone(),
                    opacities=torch.logit(g_dev["opacities"].clamp(1e-4, 1 - 1e-4)).contiguous(),
                    scales=torch.log(g_dev["scales"]).contiguous(), rotations=g_dev["rotations"].clone(),
                    language=g_dev["language"].clone())
    ids = list(range(NW))   # view 0 is frame 0: frozen
    T_w2c = torch.stack([c["viewmatrix"].t().contiguous() for c in camd[:NW]])
    proj = camd[0]["projmatrix_raw"]

    def window():
        return KeyframeWindow(T_w2c, ids, proj, camd[0]["tanfovx"], camd[0]["tanfovy"])
    exposure = torch.zeros(2, device=dev)
    steps = {
        "off": MappingStep(lanes, fresh(), g_dev["bg"], 0, camd, targets, LRS, exposure=exposure, fused_loss=True, carry_order=True),
        "window": MappingStep(lanes, fresh(), g_dev["bg"], 0, camd[NW:], targets, LRS, exposure=exposure, fused_loss=True,
                              carry_order=True, window=window()),
        "window_reg": MappingStep(lanes, fresh(), g_dev["bg"], 0, camd[NW:], targets, LRS, exposure=exposure, fused_loss=True,
                                  carry_order=True, window=window(), isotropic_weight=10.0),
    }
    for _ in range(4):
        for st in steps.values():
            st.iteration()
    ms = {k: [] for k in steps}
    for _ in range(a.reps):
        for k, st in steps.items():   # the variants alternate
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st.iteration()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = dict(gpu=torch.cuda.get_device_name(0), P=sc.P, width=W, height=H, window_views=NW, rehearsal_views=len(camd) - NW,
               lanes=1, carry_order=True, iteration={k: summary(v) for k, v in ms.items()})
    off = res["iteration"]["off"]["ms_median"]
    res["added_ms"] = {k: round(res["iteration"][k]["ms_median"] - off, 4) for k in ("window", "window_reg")}
    print(json.dumps(dict(iteration=res["iteration"], added_ms=res["added_ms"])), flush=True)

    win12 = KeyframeWindow(torch.stack([c["viewmatrix"].t().contiguous() for c in camd]), list(range(len(camd))), proj,
                           camd[0]["tanfovx"], camd[0]["tanfovy"], pose_window=5)
    win12.grad_tau.fill_(1e-3)
    win12.grad_exposure.fill_(1e-3)
    res["window_step"] = summary(timed(win12.step, a.reps))
    res["window_step_torch"] = summary(timed(torch_window([c["viewmatrix"].t().contiguous() for c in camd], list(range(len(camd))),
                                                          proj, 5), a.reps))
    scales = steps["off"].params["scales"]
    res["isotropic_reg"] = summary(timed(lambda: losses.isotropic_loss(scales, _abi.ACT_SCALE_EXP, 10.0, want_grad=True), a.reps))
    raw = scales.clone().requires_grad_(True)

    def torch_reg():
        raw.grad = None
        scaling = torch.exp(raw)
        (10 * torch.abs(scaling - scaling.mean(dim=1).view(-1, 1)).mean()).backward()
    res["isotropic_reg_torch"] = summary(timed(torch_reg, a.reps))
    res["ratio_to_torch"] = dict(window_step=round(res["window_step_torch"]["ms_median"] / res["window_step"]["ms_median"], 2),
                                 isotropic_reg=round(res["isotropic_reg_torch"]["ms_median"] / res["isotropic_reg"]["ms_median"], 2))
    print(json.dumps({k: res[k] for k in ("window_step", "window_step_torch", "isotropic_reg", "isotropic_reg_torch", "ratio_to_torch")}),
          flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
