"""Times a text query on a language code map on the GPU; prints one JSON line and writes profiles/lang_query_bench.json.

Per size (640 x 480, the reference's evaluation size, and 1200 x 680; three positives and the four negatives, K = 7) two paths
on the same GPU, float32:
  fused       LanguageQuery.similarities (stage A: codes -> K similarity planes, one launch) and LanguageQuery.localise
              (stage B: relevancy, 30 x 30 mean, blended map, score / coordinate / min / max, mask; four launches, no host read)
  torch ops   the same statements as the reference writes them (tests/lang_query_ref.py on the GPU): model_online.decode,
              model.decode — which writes the [N,768] feature image —, embed @ p.T, get_relevancy per positive, the mean as a
              30 x 30 conv2d on a reflect-101 padded map (the reference calls cv2.filter2D on the host), max / nonzero /
              min / max / threshold with their host reads.
and a third row for the reference's own sequence at full size: codes 1200 x 680 -> decoded at 640 x 480 -> back to 1200 x 680
(fused: the K similarity planes are up-sampled inside stage B; torch ops: the 768-channel features, F.interpolate, as :274).
The torch path runs whole (no row chunks): the device holds its feature image.

Per path: median / min / max over `--reps` repetitions, each between its own pair of device events after `--warmup` warm-up
calls; torch.cuda.max_memory_allocated over one call (on top of what was allocated before it); stage A's achieved FLOP/s as
2 * 744 552 * N over its time, and that as a share of the 157.3 TFLOP/s fp32 matrix peak (744 552 multiply-adds per pixel in
the two decoders; the K products add 0.7 % and are not counted; compute-bound: the weights are 3 MB).  For the torch path the
share is of the same peak, over the time of its whole stage A.  No speed ratio is required: the times are what they are.
usage: bench_lang_query.py [--reps N] [--warmup N] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lang_codec_ref as RC  # noqa: E402
import lang_query_ref as R  # noqa: E402  (the torch restatement the tests hold the kernels to)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lang_query_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_lang_query.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec  # noqa: E402
from online_lang_splatting_amd.lang_query import LanguageDecoder, LanguageQuery  # noqa: E402

dev = torch.device("cuda:0")
MACS_PER_PIXEL = 15 * 24 + 24 * 32 + sum(a * b for a, b in zip(R.WIDTHS, R.WIDTHS[1:]))
assert MACS_PER_PIXEL == 744552
PEAK_FP32_MATRIX = 157.3e12


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


class TorchOps:
    """The reference's statements in torch ops, float32, on the GPU."""

    def __init__(self, case):
        self.codec = RC.codec_from(case["online"], torch.float32).to(dev)
        self.dec = R.decoder_from(case["dec_state"], torch.float32).to(dev)
        self.p = torch.cat([case["pos"], case["neg"]]).to(dev)
        self.n_pos, self.n_neg = case["pos"].shape[0], case["neg"].shape[0]

    @torch.no_grad()
    def stage_a(self, codes, decode_hw=None, out_hw=None):
        c = codes
        if decode_hw is not None:
            c = R.resize(c, decode_hw)
        h, w = c.shape[1:]
        feat = R.features(c.permute(1, 2, 0).reshape(-1, 15), self.codec, self.dec)
        if out_hw is not None:
            feat = F.interpolate(feat.view(1, h, w, -1).permute(0, 3, 1, 2), size=out_hw, mode="bilinear",
                                 align_corners=False).permute(0, 2, 3, 1).reshape(-1, 768)
            h, w = out_hw
        return torch.mm(feat, self.p.T).T.reshape(-1, h, w)

    @torch.no_grad()
    def stage_b(self, sims):
        out = R.localise(R.relevancy(sims, self.n_pos, self.n_neg), R.THRESH)
        out["score"] = [float(s) for s in out["score"]]   # the reference reads the score and the coordinates on the host
        return out


def measure(label, H, W, decode_hw=None):
    case = R.make_case(H, W, 0, 3, 0)
    codes = case["codes"].to(dev)
    codec = OnlineLanguageCodec(dev, seed=0)
    codec.load_state_dict(RC.unflatten(case["online"]))
    q = LanguageQuery(LanguageDecoder(dev, case["dec_state"]), codec)
    q.thresh = R.THRESH
    q.set_phrases(case["pos"].to(dev), case["neg"].to(dev))
    t = TorchOps(case)
    out_hw = (H, W) if decode_hw is not None else None
    n_dec = (decode_hw[0] * decode_hw[1]) if decode_hw is not None else H * W
    res = {"width": W, "height": H, "decode_hw": decode_hw, "K": 7, "positives": 3, "N_decoded": n_dec,
           "stage_a_flop": 2 * MACS_PER_PIXEL * n_dec, "feature_image_bytes": n_dec * 768 * 4}
    # memory first, on fresh objects: one whole query each
    res["fused_peak_bytes"] = peak_bytes(lambda: q.relevancy(codes, out_hw=out_hw, decode_hw=decode_hw))
    res["torch_ops_peak_bytes"] = peak_bytes(lambda: t.stage_b(t.stage_a(codes, decode_hw, out_hw)))
    res["torch_ops_in_row_chunks"] = False
    sims_f = q.similarities(codes, decode_hw=decode_hw).clone()
    sims_t = t.stage_a(codes, decode_hw, out_hw)
    res["fused_stage_a"] = stats_ms(lambda: q.similarities(codes, decode_hw=decode_hw), args.reps, args.warmup)
    res["fused_stage_b"] = stats_ms(lambda: q.localise(sims_f, out_hw=out_hw), args.reps, args.warmup)
    res["torch_ops_stage_a"] = stats_ms(lambda: t.stage_a(codes, decode_hw, out_hw), args.reps, args.warmup)
    res["torch_ops_stage_b"] = stats_ms(lambda: t.stage_b(sims_t), args.reps, args.warmup)
    for path in ("fused", "torch_ops"):
        tf = res["stage_a_flop"] / (res[f"{path}_stage_a"]["ms_median"] * 1e-3)
        res[f"{path}_stage_a_tflops"] = round(tf / 1e12, 2)
        res[f"{path}_stage_a_share_of_fp32_matrix_peak"] = round(tf / PEAK_FP32_MATRIX, 4)
        res[f"{path}_total_ms_median"] = round(res[f"{path}_stage_a"]["ms_median"] + res[f"{path}_stage_b"]["ms_median"], 4)
    # same answer: the two paths' relevancy at the sizes timed
    a = q.relevancy(codes, out_hw=out_hw, decode_hw=decode_hw)["relevancy"]
    b = R.relevancy(sims_t, 3, 4)
    res["relevancy_max_abs_difference_between_paths"] = float((a - b).abs().max())
    del sims_t, b
    torch.cuda.empty_cache()
    print(label, json.dumps(res), file=sys.stderr, flush=True)
    return res


out = {"what": "text query on a language code map: stage A (codes -> K similarities) and stage B (relevancy, smoothing, "
               "localisation, mask), fused HIP against the reference's statements in torch ops, float32",
       "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "macs_per_pixel": MACS_PER_PIXEL,
       "fp32_matrix_peak_tflops": PEAK_FP32_MATRIX / 1e12}
out["640x480"] = measure("640x480", 480, 640)
out["1200x680"] = measure("1200x680", 680, 1200)
out["1200x680_decoded_at_640x480"] = measure("1200x680 via 640x480", 680, 1200, decode_hw=(480, 640))
line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
