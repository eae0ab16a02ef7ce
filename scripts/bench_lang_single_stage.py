"""Times the single-stage language chain (768 -> 15 -> 768) on the GPU; prints one JSON line and writes
profiles/lang_single_stage_bench.json.

Encoder, a keyframe's 192 x 192 map (N = 36 864) as a contiguous [1,768,h,w] float32 tensor:
    SingleStageEncoder.encode (one launch) against (a) the same statements in torch ops on the same GPU, permute(0,2,3,1),
    reshape(-1,768), the restated AutoencoderMLP.encode (tests/lang_single_stage_ref.py) in eval() under no_grad and .T, and
    (b) the two-stage fused entries at the same size, LanguageEncoder.encode_codes (768 -> 32 -> 15 in one launch).
Query, 640 x 480 and 1200 x 680 with K = 7 phrase rows (3 positives, 4 negatives):
    SingleStageQuery.similarities (stage A, one launch) and .relevancy (both stages) against (a) model.decode and the product
    with the phrases in torch ops, and (b) the two-stage LanguageQuery at the same size.
Per path: the median of `--reps` repetitions (default 30), each between its own pair of device events, after `--warmup`
warm-up ones; the peak growth of device memory; and the arithmetic rate from the parameter counts, 2 x 393 192 MACs per pixel
for the encoder and 2 x (540 648 + 768 K) for stage A, with its share of the 157.3 TFLOP/s fp32 matrix peak.
No speed ratio is required: what is measured is recorded, as a finding where the fused path loses.
usage: bench_lang_single_stage.py [--reps N] [--warmup N] [--out PATH]"""
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
import lang_encoder_ref as RE  # noqa: E402
import lang_query_ref as RQ  # noqa: E402
import lang_single_stage_ref as R  # noqa: E402  (the torch restatement the tests hold the kernels to)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lang_single_stage_bench.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_lang_single_stage.py needs the GPU: nothing here can be measured without one")
from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec  # noqa: E402
from online_lang_splatting_amd.lang_encoder import LanguageEncoder  # noqa: E402
from online_lang_splatting_amd.lang_query import LanguageDecoder, LanguageQuery  # noqa: E402
from online_lang_splatting_amd.lang_single_stage import SingleStageDecoder, SingleStageEncoder, SingleStageQuery  # noqa: E402

dev = torch.device("cuda:0")
ENC_MACS = sum(a * b for a, b in zip(R.ENCODER_WIDTHS, R.ENCODER_WIDTHS[1:]))
DEC_MACS = sum(a * b for a, b in zip(R.DECODER_WIDTHS, R.DECODER_WIDTHS[1:]))
assert ENC_MACS == 393192 and DEC_MACS == 540648   # the Linear weights of the 396 927 and 542 544 parameters
PEAK_FP32_MATRIX = 157.3e12
K, N_POS = 7, 3


def stats_ms(fn, reps=args.reps, warm=args.warmup):
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


def rate(res, key, macs, N):
    tf = 2.0 * macs * N / (res[key]["ms_median"] * 1e-3)
    res[key]["tflops"] = round(tf / 1e12, 2)
    res[key]["share_of_fp32_matrix_peak"] = round(tf / PEAK_FP32_MATRIX, 4)


enc_state, dec_state = R.module_state(0)
module = R.module_from(dict(enc_state, **dec_state), torch.float32).to(dev)
two_enc_state, two_dec_state, online = RE.encoder_state(0), RQ.decoder_state(0), RC.initial_params(0)
out = {"what": "single-stage language chain 768 -> 15 -> 768: fused launches against torch ops and the two-stage fused entries",
       "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "encoder_macs_per_pixel": ENC_MACS,
       "decoder_macs_per_pixel": DEC_MACS, "fp32_matrix_peak_tflops": PEAK_FP32_MATRIX / 1e12}


def codec():
    c = OnlineLanguageCodec(dev, seed=0)
    c.load_state_dict(RC.unflatten(online))
    return c


# ---- the encoder at a keyframe's size
h = w = 192
N = h * w
hr = R.make_features(N, 0).t().contiguous().view(1, 768, h, w).to(dev)


def torch_encode(x):
    with torch.no_grad():
        return module.encode(x.permute(0, 2, 3, 1).reshape(-1, 768)).T.contiguous()


enc, two_enc, two_codec = SingleStageEncoder(dev, enc_state), LanguageEncoder(dev, two_enc_state), codec()
res = {"N": N, "input_bytes": N * 768 * 4, "output_bytes": N * 15 * 4}
res["fused"] = stats_ms(lambda: enc.encode(hr))
res["torch_ops"] = stats_ms(lambda: torch_encode(hr))
res["two_stage_fused"] = stats_ms(lambda: two_enc.encode_codes(hr, two_codec))
rate(res, "fused", ENC_MACS, N)
rate(res, "torch_ops", ENC_MACS, N)
res["speedup_over_torch_ops"] = round(res["torch_ops"]["ms_median"] / res["fused"]["ms_median"], 2)
res["time_relative_to_two_stage_fused"] = round(res["fused"]["ms_median"] / res["two_stage_fused"]["ms_median"], 2)
fresh = SingleStageEncoder(dev, enc_state)   # a new object: its output buffer is allocated inside the measured call
res["fused_peak_bytes"] = peak_bytes(lambda: fresh.encode(hr))
res["torch_ops_peak_bytes"] = peak_bytes(lambda: torch_encode(hr))
out["encoder_192x192"] = res
del hr, fresh

# ---- the query
pos, neg = RQ.unit_rows(N_POS, 1).to(dev), RQ.unit_rows(K - N_POS, 2).to(dev)
phrases = torch.cat([pos, neg])


def torch_sims(c):
    with torch.no_grad():
        return torch.mm(module.decode(c.permute(1, 2, 0).reshape(-1, 15)), phrases.T).T.reshape(K, *c.shape[1:])


out["query"] = {}
for name, (h, w) in (("640x480", (480, 640)), ("1200x680", (680, 1200))):
    N = h * w
    codes = torch.randn(15, h, w, device=dev)
    codes = (codes / codes.norm(dim=0, keepdim=True)).contiguous()
    q = SingleStageQuery(SingleStageDecoder(dev, dec_state))
    two = LanguageQuery(LanguageDecoder(dev, two_dec_state), codec())
    for x in (q, two):
        x.set_phrases(pos, neg)
    res = {"N": N, "K": K}
    res["fused_similarities"] = stats_ms(lambda: q.similarities(codes))
    res["fused_relevancy"] = stats_ms(lambda: q.relevancy(codes))
    res["torch_ops_similarities"] = stats_ms(lambda: torch_sims(codes))
    res["two_stage_fused_similarities"] = stats_ms(lambda: two.similarities(codes))
    res["two_stage_fused_relevancy"] = stats_ms(lambda: two.relevancy(codes))
    rate(res, "fused_similarities", DEC_MACS + 768 * K, N)
    rate(res, "torch_ops_similarities", DEC_MACS + 768 * K, N)
    res["similarities_speedup_over_torch_ops"] = round(res["torch_ops_similarities"]["ms_median"] / res["fused_similarities"]["ms_median"], 2)
    res["similarities_time_relative_to_two_stage_fused"] = round(
        res["fused_similarities"]["ms_median"] / res["two_stage_fused_similarities"]["ms_median"], 2)
    fresh = SingleStageQuery(q.decoder)
    fresh.set_phrases(pos, neg)
    res["fused_relevancy_peak_bytes"] = peak_bytes(lambda: fresh.relevancy(codes))
    res["torch_ops_similarities_peak_bytes"] = peak_bytes(lambda: torch_sims(codes))
    res["feature_image_bytes"] = N * 768 * 4
    out["query"][name] = res
    del codes, q, two, fresh

line = json.dumps(out)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
