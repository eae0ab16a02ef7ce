"""Times the general language encoder 768 -> 32 on the GPU; prints one JSON line and writes profiles/lang_encoder_bench.json.

Per size (a keyframe's 192 x 192 map, N = 36 864, and 640 x 480), on a contiguous [1,768,h,w] float32 map:
(a) LanguageEncoder.encode (one launch) against the same statements in torch ops on the same GPU: permute(0,2,3,1),
    reshape(-1,768) and the restated AutoencoderMLP.encode (tests/lang_encoder_ref.py) in eval() under no_grad;
(b) LanguageEncoder.encode_codes (the 15-channel codes from the same launch) against those torch ops followed by the online
    encoder in torch ops;
(c) the arithmetic rate 2 * 567 296 * N over the time, and that as a share of the 157.3 TFLOP/s fp32 matrix peak;
(d) peak device memory of both paths;
(e) at 192 x 192 the keyframe chain: OnlineLanguageTargets.add_keyframe_hr against torch-op encode followed by add_keyframe.
Medians over `--reps` repetitions (default 40), each between its own pair of device events, after `--warmup` warm-up ones.
No speed ratio is required: there is no earlier figure for this entry, the comparison is the torch-op path of the same run.
Required, because it can be derived: the fused path's peak memory growth at N = 36 864 is its outputs, N (32 + 15) 4 bytes,
plus at most 1 MB.
usage: bench_lang_encoder.py [--reps N] [--warmup N] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lang_codec_ref as RC  # noqa: E402
import lang_encoder_ref as R  # noqa: E402  (the torch restatement the tests hold the kernel to)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lang_encoder_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_lang_encoder.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec  # noqa: E402
from online_lang_splatting_amd.lang_encoder import LanguageEncoder  # noqa: E402
from online_lang_splatting_amd.slam_iterations import OnlineLanguageTargets  # noqa: E402

dev = torch.device("cuda:0")
MACS_PER_PIXEL = sum(a * b for a, b in zip(R.WIDTHS, R.WIDTHS[1:]))
assert MACS_PER_PIXEL == 567296
PEAK_FP32_MATRIX = 157.3e12
LR = 1e-4


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


state, online = R.encoder_state(0), RC.initial_params(0)
module = R.encoder_from(state, torch.float32).to(dev)
online_module = RC.codec_from(online, torch.float32).to(dev)


def torch_encode(hr):
    with torch.no_grad():
        return module.encode(hr.permute(0, 2, 3, 1).reshape(-1, 768))


def torch_encode_codes(hr):
    with torch.no_grad():
        f32 = module.encode(hr.permute(0, 2, 3, 1).reshape(-1, 768))
        return f32, online_module.encode(f32).T.contiguous()


def fresh():
    enc, codec = LanguageEncoder(dev, state), OnlineLanguageCodec(dev, seed=0)
    codec.load_state_dict(RC.unflatten(online))
    return enc, codec


out = {"what": "general language encoder 768 -> 32: fused launch against torch ops", "reps": args.reps, "warmup": args.warmup,
       "device": torch.cuda.get_device_name(0), "macs_per_pixel": MACS_PER_PIXEL, "fp32_matrix_peak_tflops": PEAK_FP32_MATRIX / 1e12,
       "sizes": {}}
enc, codec = fresh()
for name, (h, w) in (("192x192", (192, 192)), ("640x480", (480, 640))):
    N = h * w
    hr = R.make_features(N, 0).t().contiguous().view(1, 768, h, w).to(dev)
    res = {"N": N, "input_bytes": N * 768 * 4}
    res["fused_encode"] = stats_ms(lambda: enc.encode(hr), args.reps, args.warmup)
    res["fused_encode_codes"] = stats_ms(lambda: enc.encode_codes(hr, codec), args.reps, args.warmup)
    res["torch_ops_encode"] = stats_ms(lambda: torch_encode(hr), args.reps, args.warmup)
    res["torch_ops_encode_codes"] = stats_ms(lambda: torch_encode_codes(hr), args.reps, args.warmup)
    for path in ("fused", "torch_ops"):
        tf = 2.0 * MACS_PER_PIXEL * N / (res[f"{path}_encode"]["ms_median"] * 1e-3)
        res[f"{path}_encode_tflops"] = round(tf / 1e12, 2)
        res[f"{path}_encode_share_of_fp32_matrix_peak"] = round(tf / PEAK_FP32_MATRIX, 4)
    res["encode_speedup"] = round(res["torch_ops_encode"]["ms_median"] / res["fused_encode"]["ms_median"], 2)
    res["encode_codes_speedup"] = round(res["torch_ops_encode_codes"]["ms_median"] / res["fused_encode_codes"]["ms_median"], 2)

    e2, c2 = fresh()   # new objects: their output buffers are allocated inside the measured call
    res["fused_peak_bytes"] = peak_bytes(lambda: e2.encode_codes(hr, c2))
    del e2, c2
    res["torch_ops_peak_bytes"] = peak_bytes(lambda: torch_encode_codes(hr))
    res["output_bytes"] = N * (32 + 15) * 4
    out["sizes"][name] = res
    del hr

# the keyframe chain at 192 x 192
h = w = 192
hr = R.make_features(h * w, 1).t().contiguous().view(1, 768, h, w).to(dev)
lt = OnlineLanguageTargets(codec, lr=LR, hw=(h, w))
chain = {"N": h * w}
chain["add_keyframe_hr"] = stats_ms(lambda: lt.add_keyframe_hr(0, hr, enc), args.reps, args.warmup)
chain["torch_ops_encode_then_add_keyframe"] = stats_ms(lambda: lt.add_keyframe(0, torch_encode(hr)), args.reps, args.warmup)
chain["speedup"] = round(chain["torch_ops_encode_then_add_keyframe"]["ms_median"] / chain["add_keyframe_hr"]["ms_median"], 2)
out["keyframe_chain_192x192"] = chain

line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
kf = out["sizes"]["192x192"]
if kf["fused_peak_bytes"] > kf["output_bytes"] + (1 << 20):
    raise SystemExit(f"the fused path's peak memory growth {kf['fused_peak_bytes']} exceeds its outputs {kf['output_bytes']} + 1 MB")
