"""Times the colour-refinement loss and loop on the GPU; prints one JSON line.

(a) olsr_refinement_loss alone on a config-3 sized frame (1200x680) against the same loss written with torch ops on the same
    GPU (a restatement of the formula: five grouped 11x11 conv2d, forward + autograd backward).
(b) ms per RefinementStep.iteration on the room map and on the volume (500 k Gaussians, 1200x680, F = 15), against the same
    loop with the torch-op loss in the middle.
Medians over `--reps` repetitions (default 60), each between its own pair of device events, after `--warmup` warm-up ones.
usage: bench_refine.py [--reps N] [--warmup N] [--scenes room,volume | none] [--P N]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import ssim_ref  # noqa: E402  (the torch restatement of the loss the tests hold the kernel to)
from online_lang_splatting_amd import _abi, losses  # noqa: E402
from online_lang_splatting_amd.frame_shard import FrameLanes  # noqa: E402
from online_lang_splatting_amd.scene import arc_cameras, make_room_scene, make_scene  # noqa: E402
from online_lang_splatting_amd.slam_iterations import RefinementStep  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--scenes", default="room,volume")
ap.add_argument("--P", type=int, default=500_000)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_refine.py needs the GPU: nothing here can be measured without one")
dev = torch.device("cuda:0")
H, W, Fch, LAMBDA = 680, 1200, 15, 0.2

def torch_loss(image, gt, lam=LAMBDA):
    """(1 - lam) L1 + lam (1 - SSIM) with torch ops (tests/ssim_ref.py, float32 on the GPU); -> (loss, d loss / d image)."""
    o = ssim_ref.loss_and_grad(image, gt, lam)
    return o["loss"][0], o["dL_dimage"]


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return statistics.median(ts), ts[0], ts[-1]


class TorchLossStep(RefinementStep):
    def loss(self, image, gt_image):
        l, d = torch_loss(image, gt_image, self.lambda_dssim)
        return dict(loss=l.reshape(1), dL_dimage=d.contiguous())


out = {"what": "colour-refinement loss and loop", "H": H, "W": W, "lambda_dssim": LAMBDA, "reps": args.reps, "warmup": args.warmup}
g = torch.Generator().manual_seed(0)
gt = torch.rand(3, H, W, generator=g).to(dev)
image = (gt + 0.05 * torch.randn(3, H, W, generator=g).to(dev)).clamp(0, 1).contiguous()
buf = {}
m, lo, hi = median_ms(lambda: losses.refinement_loss(image, gt, lambda_dssim=LAMBDA, buffers=buf), args.reps, args.warmup)
out["loss_entry"] = {"ms_median": round(m, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
m, lo, hi = median_ms(lambda: losses.refinement_loss(image, gt, lambda_dssim=LAMBDA, want_grad=False, buffers=buf), args.reps, args.warmup)
out["loss_entry_values_only"] = {"ms_median": round(m, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
m, lo, hi = median_ms(lambda: torch_loss(image, gt), args.reps, args.warmup)
out["torch_ops_same_gpu"] = {"ms_median": round(m, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
out["loss_speedup"] = round(out["torch_ops_same_gpu"]["ms_median"] / out["loss_entry"]["ms_median"], 2)
# bytes the algorithm needs: image and target read once, the cotangent written once (+ the three intermediate planes of the
# two-launch form written and read once)
out["loss_algorithmic_bytes"] = 3 * 3 * H * W * 4
out["loss_intermediate_bytes"] = 2 * 9 * H * W * 4

lrs = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)
for which in [s for s in args.scenes.split(",") if s and s != "none"]:
    if which == "room":
        rs = make_room_scene(args.P, W, H, Fch, views=10, seed=3)
        sc, cams, gts = rs.scene, rs.cameras, [t[0] for t in rs.targets]
    else:
        sc = make_scene(args.P, W, H, Fch, seed=3)
        cams = arc_cameras(W, H, n=10)
        gen = torch.Generator().manual_seed(1)
        gts = [torch.rand(3, H, W, generator=gen) for _ in cams]
    M = sc.shs.shape[1]
    g_dev, _ = bench.device_inputs(sc, cams[0], dev)
    camd = [bench.device_inputs(sc, c, dev)[1] for c in cams]
    R0 = max(bench._sized_capacity(Fch, g_dev, c, H, W, 0, dev, (15, _abi.BWD_REFERENCE, _abi.BINNING_ELLIPSE)) for c in camd)
    res = {"P": sc.P, "views": len(camd)}
    for name, cls in (("fused", RefinementStep), ("torch_ops_loss", TorchLossStep)):
        lanes = FrameLanes(1, sc.P, W, H, Fch, M, int(1.5 * R0) + (1 << 16), dev)
        params = dict(means3D=g_dev["means3D"].clone(), shs=g_dev["shs"].clone(),
                      opacities=torch.logit(g_dev["opacities"].clamp(1e-4, 1 - 1e-4)).contiguous(),
                      scales=torch.log(g_dev["scales"]).contiguous(), rotations=g_dev["rotations"].clone(),
                      language=g_dev["language"].clone())
        step = cls(lanes, params, g_dev["bg"], 0, camd, gts, lrs, lambda_dssim=LAMBDA, position_schedule=(1.6e-4, 1.6e-6, 30000))
        k = [0]

        def one():
            step.iteration(k[0] % len(camd))
            k[0] += 1
        m, lo, hi = median_ms(one, args.reps, max(args.warmup, len(camd)))
        res[name] = {"ms_median": round(m, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
        del step, lanes, params
    res["iteration_speedup"] = round(res["torch_ops_loss"]["ms_median"] / res["fused"]["ms_median"], 3)
    out["refinement_iteration_" + which] = res
print(json.dumps(out))
