"""Times the high-resolution language feature net on the GPU; prints one JSON line and writes profiles/hr_net_bench.json.

At the back end's sizes (clip_vis_dense [1,768,24,24], res3 [1,384,48,48], res2 [1,192,96,96] -> [1,768,192,192], float32):
(a) HighResLanguageNet.forward (thirteen launches) against the same module in torch ops on the same GPU (MIOpen, float32,
    eval(), no_grad: tests/hr_net_ref.forward, the restatement the tests hold the kernels to);
(b) every launch of the fused path on its own (the `launches` mask of olsr_hr_net_forward), with its FLOPs, its workgroup
    count and its arithmetic rate;
(c) the arithmetic rate of the whole forward, 2 x the multiply-adds of the thirteen layers over the time, and that as a share of
    the 157.3 TFLOP/s fp32 matrix peak;
(d) peak device memory of both paths;
(e) the keyframe chain: OnlineLanguageTargets.add_keyframe_backbone (HR net -> encoder -> online step) against torch-op HR net
    and encoder followed by add_keyframe.
Medians over `--reps` repetitions (default 30, at least 20), each between its own pair of device events, after `--warmup`
warm-up ones.  No speed ratio is required: the figures are a measurement, whichever way they fall.
usage: bench_hr_net.py [--reps N] [--warmup N] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hr_net_ref as R  # noqa: E402  (the torch restatement the tests hold the kernels to)
import lang_codec_ref as RC  # noqa: E402
import lang_encoder_ref as RE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hr_net_bench.json"))
args = ap.parse_args()
if args.reps < 20:
    raise SystemExit("bench_hr_net.py: at least 20 repetitions")
if not torch.cuda.is_available():
    raise SystemExit("bench_hr_net.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd.hr_net import HighResLanguageNet  # noqa: E402
from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec  # noqa: E402
from online_lang_splatting_amd.lang_encoder import LanguageEncoder  # noqa: E402
from online_lang_splatting_amd.slam_iterations import OnlineLanguageTargets  # noqa: E402

dev = torch.device("cuda:0")
PEAK_FP32_MATRIX = 157.3e12
H = W = 24
SIZES = ((H, W), (2 * H, 2 * W), (4 * H, 4 * W))


def layer_table():
    """(name, output pixels, multiply-adds, workgroups) per launch: 64 pixels x 64 output channels per workgroup, 8 x 8 tiles
    for the 3x3 and the transposed layers (whose four phases are workgroups of their own)."""
    rows, hw = [], H * W
    for k, (path, kind, o, i, _) in enumerate(R.LAYERS):
        scale = 1 if k == 0 else 4 if k <= 5 else 16 if k <= 10 else 64       # the layer's OUTPUT grid over fv's
        px = hw * scale
        side = H * int(scale ** 0.5)
        if kind == "conv1":
            macs, groups = px * o * i, -(-px // 64) * (o // 64)
        elif kind == "conv3":
            macs, groups = px * o * i * 9, (-(-side // 8)) ** 2 * (o // 64)
        else:   # four taps per output pixel; tiles over the input grid, four phases
            macs, groups = px * o * i * 4, (-(-(side // 2) // 8)) ** 2 * (o // 64) * 4
        rows.append((path, px, macs, groups))
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


state = R.net_state(0)
dev_state = {k: v.to(dev) for k, v in state.items()}
fv, f3, f2 = (t.to(dev) for t in R.make_inputs(SIZES, 0))
net = HighResLanguageNet(dev, state)


def torch_forward():
    return R.forward(dev_state, fv, f3, f2, torch.float32)[None]


table = layer_table()
total_macs = sum(m for _, _, m, _ in table)
out = {"what": "high-resolution language feature net: thirteen fused launches against torch ops (MIOpen, float32)",
       "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "sizes": [list(s) for s in SIZES],
       "gflop": round(2 * total_macs / 1e9, 2), "fp32_matrix_peak_tflops": PEAK_FP32_MATRIX / 1e12}
got, want = net.forward(fv, f3, f2), torch_forward()
out["max_abs_difference_to_torch_ops"] = float((got - want).abs().max())
out["fused_forward"] = stats_ms(lambda: net.forward(fv, f3, f2), args.reps, args.warmup)
out["torch_ops_forward"] = stats_ms(torch_forward, args.reps, args.warmup)
for path in ("fused", "torch_ops"):
    tf = 2.0 * total_macs / (out[f"{path}_forward"]["ms_median"] * 1e-3)
    out[f"{path}_tflops"] = round(tf / 1e12, 2)
    out[f"{path}_share_of_fp32_matrix_peak"] = round(tf / PEAK_FP32_MATRIX, 4)
out["speedup"] = round(out["torch_ops_forward"]["ms_median"] / out["fused_forward"]["ms_median"], 3)

out["launches"] = []
for k, (path, px, macs, groups) in enumerate(table):
    t = stats_ms(lambda: net.forward(fv, f3, f2, launches=1 << k), args.reps, 2)
    out["launches"].append({"launch": k, "layer": path, "output_pixels": px, "gflop": round(2 * macs / 1e9, 2), "workgroups": groups,
                            "ms_median": t["ms_median"], "ms_min": t["ms_min"],
                            "tflops": round(2 * macs / (t["ms_median"] * 1e-3) / 1e12, 2)})
out["launches_sum_ms"] = round(sum(r["ms_median"] for r in out["launches"]), 4)

n2 = HighResLanguageNet(dev, state)   # a new object: its workspace and output are allocated inside the measured call
out["fused_peak_bytes"] = peak_bytes(lambda: n2.forward(fv, f3, f2))
out["fused_workspace_bytes"] = int(n2.workspace(H, W, *SIZES[1], *SIZES[2]).numel())
del n2
out["torch_ops_peak_bytes"] = peak_bytes(torch_forward)
out["output_bytes"] = 768 * 64 * H * W * 4

# the keyframe chain: HR net -> encoder -> online step
enc_state, online = RE.encoder_state(0), RC.initial_params(0)
enc = LanguageEncoder(dev, enc_state)
enc_module = RE.encoder_from(enc_state, torch.float32).to(dev)
codec = OnlineLanguageCodec(dev, seed=0)
codec.load_state_dict(RC.unflatten(online))
lt = OnlineLanguageTargets(codec, lr=1e-4, hw=(8 * H, 8 * W))


def torch_chain():
    with torch.no_grad():
        rows = enc_module.encode(torch_forward().permute(0, 2, 3, 1).reshape(-1, 768))
    return lt.add_keyframe(0, rows)


chain = {"add_keyframe_backbone": stats_ms(lambda: lt.add_keyframe_backbone(0, fv, f3, f2, net, enc), args.reps, args.warmup),
         "torch_ops_hr_and_encode_then_add_keyframe": stats_ms(torch_chain, args.reps, args.warmup)}
chain["speedup"] = round(chain["torch_ops_hr_and_encode_then_add_keyframe"]["ms_median"] / chain["add_keyframe_backbone"]["ms_median"], 3)
out["keyframe_chain"] = chain

print(json.dumps(out))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
