"""SHA-256 of every output of the language nets on seeded inputs, as JSON: run it on two builds and compare the files.

The codec (train step, encode, decode), the general and the single-stage encoder (rows and channel planes, both code layouts,
N = 257: four full tiles and a one-pixel tail; once with planes one float off a 16-byte boundary and a plane stride above N),
the two text queries (37 x 53: 30 full tiles and a 41-pixel tail; similarities native and with the codes resampled to a
29 x 41 decode size at K = 9, 17 and 64 phrase rows, so that 1, 2 and 4 phrase tiles are hashed; relevancy at K = 9) and the HR
net (5x7, 9x10).  Inputs come from the tests' reference modules; no test reads this.
usage: lang_bits.py --out PATH"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hr_net_ref as RH  # noqa: E402
import lang_codec_ref as RC  # noqa: E402
import lang_encoder_ref as RE  # noqa: E402
import lang_query_ref as RQ  # noqa: E402
import lang_single_stage_ref as RS  # noqa: E402
from online_lang_splatting_amd.hr_net import HighResLanguageNet  # noqa: E402
from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec  # noqa: E402
from online_lang_splatting_amd.lang_encoder import LanguageEncoder  # noqa: E402
from online_lang_splatting_amd.lang_query import LanguageDecoder, LanguageQuery  # noqa: E402
from online_lang_splatting_amd.lang_single_stage import SingleStageDecoder, SingleStageEncoder, SingleStageQuery  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
args = ap.parse_args()
DEV = torch.device("cuda:0")
digests = {}


def put(name, t):
    t = t.detach().cpu().contiguous()
    digests[name] = hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def codec_of(flat):
    c = OnlineLanguageCodec(DEV, seed=0)
    c.load_state_dict(RC.unflatten(flat))
    return c


# the codec
flat, q, _ = RC.make_case(257, 3)
x = RC.unit(q).to(DEV)
codec = codec_of(flat)
grad = torch.zeros(RC.N_PARAMS, dtype=torch.float32, device=DEV)
loss, codes = codec.train_step(x, 1e-3, codes="pre", layout="channels", grad_out=grad, step=1)
for name, t in (("loss", loss), ("codes", codes), ("grad", grad), ("params", codec.flat), ("exp_avg", codec.exp_avg),
                ("exp_avg_sq", codec.exp_avg_sq)):
    put(f"codec.train_step.{name}", t)
for layout in ("rows", "channels"):
    c = codec.encode(x, layout)
    put(f"codec.encode.{layout}", c)
    put(f"codec.decode.{layout}", codec.decode(c, layout))

def off_planes(rows):
    """rows [N,768] as channel planes [768,1,N] that start one float off a 16-byte boundary, N + 3 floats apart"""
    n = rows.shape[0]
    buf = torch.zeros(1 + 768 * (n + 3), dtype=torch.float32, device=DEV)
    planes = torch.as_strided(buf[1:], (768, 1, n), (n + 3, n, 1))
    planes.copy_(rows.t().view(768, 1, n))
    assert planes.data_ptr() % 16 == 4
    return planes


# the general encoder
enc = LanguageEncoder(DEV, RE.encoder_state(1))
codec = codec_of(RC.initial_params(0))
rows = RE.make_features(257, 2).to(DEV)
planes = rows.t().contiguous().view(768, 1, 257)
for name, f in (("rows", rows), ("channels", planes)):
    put(f"encoder.{name}.features32", enc.encode(f))
    for layout in ("rows", "channels"):
        f32, c = enc.encode_codes(f, codec, layout)
        put(f"encoder.{name}.fused.{layout}.features32", f32)
        put(f"encoder.{name}.fused.{layout}.codes", c)
f32, c = enc.encode_codes(off_planes(rows), codec, "channels")
put("encoder.channels_unaligned.fused.channels.features32", f32)
put("encoder.channels_unaligned.fused.channels.codes", c)

# the single-stage encoder
ss_enc = SingleStageEncoder(DEV, RS.encoder_state(1))
rows = RS.make_features(257, 2).to(DEV)
for name, f in (("rows", rows), ("channels", rows.t().contiguous().view(768, 1, 257)), ("channels_unaligned", off_planes(rows))):
    for layout in ("rows", "channels"):
        put(f"ss_encoder.{name}.{layout}", ss_enc.encode(f, layout))

# the text query
case = RQ.make_case(37, 53, 4, 3, 2, 4)
query = LanguageQuery(LanguageDecoder(DEV, case["dec_state"]), codec_of(case["online"]))
query.thresh = RQ.THRESH
query.set_phrases(case["pos"].to(DEV), case["neg"].to(DEV))
query.set_labels(case["labels"].to(DEV))
for name, hw in (("native", None), ("decode29x41", (29, 41))):
    put(f"query.{name}.similarities", query.similarities(case["codes"].to(DEV), decode_hw=hw))
    for k, v in query.relevancy(case["codes"].to(DEV), decode_hw=hw).items():
        put(f"query.{name}.relevancy.{k}", v)


def more_phrases(query, case, tag):
    """similarities with 17 and 64 phrase rows (K = 9 is the case's own 3 + 2 + 4)"""
    for K in (17, 64):
        query.set_phrases(case["pos"].to(DEV), RQ.unit_rows(K - 5, K).to(DEV))
        for name, hw in (("native", None), ("decode29x41", (29, 41))):
            put(f"{tag}.K{K}.{name}.similarities", query.similarities(case["codes"].to(DEV), decode_hw=hw))


more_phrases(query, case, "query")

# the single-stage text query
case = RS.make_query_case(37, 53, 4, 3, 2, 4)
query = SingleStageQuery(SingleStageDecoder(DEV, case["dec_state"]))
query.set_phrases(case["pos"].to(DEV), case["neg"].to(DEV))
query.set_labels(case["labels"].to(DEV))
for name, hw in (("native", None), ("decode29x41", (29, 41))):
    put(f"ss_query.K9.{name}.similarities", query.similarities(case["codes"].to(DEV), decode_hw=hw))
for k, v in query.relevancy(case["codes"].to(DEV)).items():
    put(f"ss_query.K9.native.relevancy.{k}", v)
more_phrases(query, case, "ss_query")

# the HR net
net = HighResLanguageNet(DEV, RH.net_state(300))
for name, sizes, seed in (("5x7", ((5, 7), (10, 14), (20, 28)), 11), ("9x10", ((9, 10), (7, 9), (40, 37)), 12)):
    put(f"hr_net.{name}", net(*(t.to(DEV) for t in RH.make_inputs(sizes, seed))))

torch.cuda.synchronize()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(digests, f, indent=1, sort_keys=True)
print(f"lang_bits: {len(digests)} digests -> {args.out}")
