"""Times the CLIP ConvNeXt image tower on the GPU; prints one JSON line and writes profiles/clip_trunk_bench.json.

At the back end's sizes (convnext_large: depths 3, 3, 27, 3, dims 192 ... 1536, E = 768, a 680 x 1200 frame resized to 768 x 768,
float32):
(a) ClipTrunk.forward (111 launches) against the same statements in torch ops on the same GPU (float32, eval(), no_grad, warmed
    up: tests/clip_trunk_ref.forward, the restatement the tests hold the kernels to);
(b) every launch of the fused path on its own (the `launches` mask of olsr_clip_trunk_forward), summed per launch kind and per
    stage, with the FLOPs of each; and the torch-op side per stage (stem; downsample + blocks of each stage; head);
(c) the arithmetic rate of the whole forward on the layers' own FLOPs (about 800 GFLOP), and that as a share of the
    157.3 TFLOP/s fp32 matrix peak;
(d) peak device memory of both paths;
(e) the keyframe chain trunk -> HR net -> encoder -> online step (ClipTrunk.feature_fn into OnlineLanguageTargets) against
    the same chain with the trunk in torch ops.
Medians over `--reps` repetitions (default 30, at least 20), each between its own pair of device events, after `--warmup`
warm-up ones.  No speed ratio is required: the figures are a measurement, whichever way they fall.
usage: bench_clip_trunk.py [--reps N] [--warmup N] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_trunk_ref as R  # noqa: E402  (the torch restatement the tests hold the kernels to)
import hr_net_ref as RH  # noqa: E402
import lang_codec_ref as RC  # noqa: E402
import lang_encoder_ref as RE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_trunk_bench.json"))
args = ap.parse_args()
if args.reps < 20:
    raise SystemExit("bench_clip_trunk.py: at least 20 repetitions")
if not torch.cuda.is_available():
    raise SystemExit("bench_clip_trunk.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd import ClipTrunk, _abi  # noqa: E402
from online_lang_splatting_amd.hr_net import HighResLanguageNet  # noqa: E402
from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec  # noqa: E402
from online_lang_splatting_amd.lang_encoder import LanguageEncoder  # noqa: E402
from online_lang_splatting_amd.slam_iterations import OnlineLanguageTargets  # noqa: E402

dev = torch.device("cuda:0")
PEAK_FP32_MATRIX = 157.3e12
DEPTHS, DIMS, E, RES = _abi.CLIP_TRUNK_DEPTHS, _abi.CLIP_TRUNK_DIMS, _abi.CLIP_TRUNK_EMBED, 768
CFG = dict(depths=DEPTHS, dims=DIMS, embed_dim=E)
HW = (680, 1200)


def launch_table():
    """(kind, stage, multiply-adds) per launch, in the order of include/olsr_clip_trunk.h."""
    px = (RES // 4) ** 2
    rows = [("stem_conv", "stem", px * DIMS[0] * 48), ("stem_ln", "stem", 0)]
    for i in range(4):
        c = DIMS[i]
        if i > 0:
            px //= 4
            rows.append(("downsample", f"stage{i}", px * c * 4 * DIMS[i - 1]))
        for _ in range(DEPTHS[i]):
            rows.append(("dw_ln", f"stage{i}", px * c * 49))
            if c <= _abi.CLIP_TRUNK_FUSED_MAX_C:
                rows.append(("mlp_fused", f"stage{i}", px * 8 * c * c))
            else:
                rows += [("fc1_gelu", f"stage{i}", px * 4 * c * c), ("fc2_residual", f"stage{i}", px * 4 * c * c)]
    rows.append(("head", "head", px * DIMS[3] * E))
    return rows


def stats_ms(fn, reps, warm):
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
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4)}


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del out
    return int(grown)


state = R.trunk_state(0, device=dev, **CFG)
image = R.make_image(*HW, 0, device=dev)
trunk = ClipTrunk(dev, state, resolution=RES, **CFG)


def torch_forward():
    return R.forward(state, image, torch.float32, resolution=RES, **CFG)


table = launch_table()
assert len(table) == trunk.n_launches, (len(table), trunk.n_launches)
total_macs = sum(m for _, _, m in table)
out = {"what": "CLIP ConvNeXt-L image tower: 111 fused launches against torch ops (float32)", "reps": args.reps,
       "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "image": list(HW), "resolution": RES,
       "gflop": round(2 * total_macs / 1e9, 1), "fp32_matrix_peak_tflops": PEAK_FP32_MATRIX / 1e12, "launches": trunk.n_launches}
got, want = trunk.forward(image), torch_forward()
out["max_abs_difference_to_torch_ops"] = {k: float((got[k] - want[k]).abs().max()) for k in got}
out["max_abs_value"] = {k: float(want[k].abs().max()) for k in want}
out["fused_forward"] = stats_ms(lambda: trunk.forward(image), args.reps, args.warmup)
out["torch_ops_forward"] = stats_ms(torch_forward, args.reps, args.warmup)
for path in ("fused", "torch_ops"):
    tf = 2.0 * total_macs / (out[f"{path}_forward"]["ms_median"] * 1e-3)
    out[f"{path}_tflops"] = round(tf / 1e12, 2)
    out[f"{path}_share_of_fp32_matrix_peak"] = round(tf / PEAK_FP32_MATRIX, 4)
out["speedup"] = round(out["torch_ops_forward"]["ms_median"] / out["fused_forward"]["ms_median"], 3)

# every launch on its own, summed per kind and per stage
kinds, stages = {}, {}
for k, (kind, stage, macs) in enumerate(table):
    t = stats_ms(lambda: trunk.forward(image, launches=1 << k), args.reps, 1)["ms_median"]
    for d, key in ((kinds, kind), (stages, stage)):
        r = d.setdefault(key, {"launches": 0, "gflop": 0.0, "ms": 0.0})
        r["launches"] += 1
        r["gflop"] += 2 * macs / 1e9
        r["ms"] += t
for d in (kinds, stages):
    for r in d.values():
        r["gflop"], r["ms"] = round(r["gflop"], 2), round(r["ms"], 4)
        r["tflops"] = round(r["gflop"] / r["ms"], 2) if r["ms"] > 0 else None
out["fused_per_kind"], out["fused_per_stage"] = kinds, stages
out["launches_sum_ms"] = round(sum(r["ms"] for r in kinds.values()), 4)

# the torch-op side per stage: the same statements, each stage on the input the stage before it left
with torch.no_grad():
    t_ = "visual.trunk."
    x = torch.nn.functional.interpolate(R.normalised(image, torch.float32)[None], size=(RES, RES), mode="bilinear", align_corners=False)

    def stem():
        y = torch.nn.functional.interpolate(R.normalised(image, torch.float32)[None], size=(RES, RES), mode="bilinear",
                                            align_corners=False)
        return R._ln2d(torch.nn.functional.conv2d(y, state[t_ + "stem.0.weight"], state[t_ + "stem.0.bias"], stride=4),
                       state[t_ + "stem.1.weight"], state[t_ + "stem.1.bias"], R.EPS)

    def stage(i, y):
        p = f"{t_}stages.{i}."
        if i > 0:
            y = R._ln2d(y, state[p + "downsample.0.weight"], state[p + "downsample.0.bias"], R.EPS)
            y = torch.nn.functional.conv2d(y, state[p + "downsample.1.weight"], state[p + "downsample.1.bias"], stride=2)
        for j in range(DEPTHS[i]):
            y = R._block(state, f"{p}blocks.{j}.", y, R.EPS)
        return y

    per = {"stem": stats_ms(stem, args.reps, 2)["ms_median"]}
    x = stem()
    for i in range(4):
        per[f"stage{i}"] = stats_ms(lambda: stage(i, x), args.reps, 2)["ms_median"]
        x = stage(i, x)

    def head():
        h = torch.nn.functional.layer_norm(x.permute(0, 2, 3, 1), (DIMS[3],), state[t_ + "head.norm.weight"],
                                           state[t_ + "head.norm.bias"], R.EPS)
        return torch.nn.functional.linear(h, state["visual.head.proj.weight"])

    per["head"] = stats_ms(head, args.reps, 2)["ms_median"]
out["torch_ops_per_stage_ms"] = per
del x

t2 = ClipTrunk(dev, resolution=RES, **CFG)   # a new object: its workspace and outputs are allocated inside the measured call
out["fused_peak_bytes"] = peak_bytes(lambda: t2.forward(image))
out["fused_workspace_bytes"] = int(t2.workspace().numel())
del t2
out["torch_ops_peak_bytes"] = peak_bytes(torch_forward)
out["parameter_bytes"] = int(trunk.flat.numel() * 4)

# the keyframe chain: trunk -> HR net -> encoder -> online step
hr = HighResLanguageNet(dev, RH.net_state(0))
enc = LanguageEncoder(dev, RE.encoder_state(0))
codec = OnlineLanguageCodec(dev, seed=0)
codec.load_state_dict(RC.unflatten(RC.initial_params(0)))
lt = OnlineLanguageTargets(codec, lr=1e-4, hw=(RES // 4, RES // 4))
fn = trunk.feature_fn(hr, enc)


def fused_chain():
    call = fn(0, image)
    return getattr(lt, call[0])(0, *call[1:])


def torch_chain():
    o = torch_forward()
    return lt.add_keyframe_backbone(0, o["clip_vis_dense"][None].contiguous(), o["res3"][None].contiguous(), o["res2"][None].contiguous(), hr, enc)


chain = {"trunk_fused": stats_ms(fused_chain, args.reps, args.warmup), "trunk_in_torch_ops": stats_ms(torch_chain, args.reps, args.warmup),
         "hr_net_and_after_alone": stats_ms(lambda: lt.add_keyframe_backbone(0, got["clip_vis_dense"][None], got["res3"][None],
                                                                           got["res2"][None], hr, enc), args.reps, args.warmup)}
chain["speedup"] = round(chain["trunk_in_torch_ops"]["ms_median"] / chain["trunk_fused"]["ms_median"], 3)
out["keyframe_chain"] = chain

print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
