"""SHA-256 of every output of the language nets on seeded inputs, as JSON: run it on two builds and compare the files.

The codec (train step, encode, decode), the general encoder (rows and channel planes, with and without fused codes,
N = 257), the text query (similarities and relevancy at 37 x 53 with 3 positives, 2 labels, 4 negatives, once resampled to a
decode size) and the HR net (5x7, 9x10).  Inputs come from the tests' reference modules; no test reads this.
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
from online_lang_splatting_amd.hr_net import HighResLanguageNet  # noqa: E402
from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec  # noqa: E402
from online_lang_splatting_amd.lang_encoder import LanguageEncoder  # noqa: E402
from online_lang_splatting_amd.lang_query import LanguageDecoder, LanguageQuery  # noqa: E402

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

# the HR net
net = HighResLanguageNet(DEV, RH.net_state(300))
for name, sizes, seed in (("5x7", ((5, 7), (10, 14), (20, 28)), 11), ("9x10", ((9, 10), (7, 9), (40, 37)), 12)):
    put(f"hr_net.{name}", net(*(t.to(DEV) for t in RH.make_inputs(sizes, seed))))

torch.cuda.synchronize()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(digests, f, indent=1, sort_keys=True)
print(f"lang_bits: {len(digests)} digests -> {args.out}")
