"""Torch restatement of the reference's single-stage language chain, dtype-generic and on the CPU: the yardstick of
tests/test_gpu_lang_single_stage.py (float64 = "truth", float32 = "ref32") at sizes too large to commit.

    utils/slam_backend.py:117-119             single_stage_ae: AutoencoderMLP([384,192,96,48,24,15], [24,48,96,192,384,384,768])
    utils/slam_backend.py:556-576 (:562 false)   clip_viz_dense.permute(0,2,3,1).view(-1,768) -> auto_model.encode ->
                                              .T.view(15,192,192), the keyframe's language target; nothing is trained online
    eval/evaluate_langslam.py:266-273         F.interpolate of the codes (:270), model.decode alone
    language/autoencoder/model.py:15-62       AutoencoderMLP: Linear, then BatchNorm1d / ReLU / Linear per encoder layer, Linear
                                              and ReLU / Linear per decoder layer, encode and decode end in x / x.norm(dim=-1)
    utils/slam_backend.py:142                 the module is in eval(): BatchNorm1d uses its running statistics

tests/test_lang_single_stage_ref_golden.py pins this module to arrays recorded from the reference's own module
(tests/golden/make_golden_lang_single_stage.py -> lang_single_stage.npz).
"""
import os
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

import lang_encoder_ref as RE
import lang_query_ref as RQ

ENCODER_DIMS = (384, 192, 96, 48, 24, 15)             # language.encoder_dims of a single-stage config
DECODER_DIMS = (24, 48, 96, 192, 384, 384, 768)       # language.decoder_dims
ENCODER_WIDTHS = (768,) + ENCODER_DIMS
DECODER_WIDTHS = (ENCODER_DIMS[-1],) + DECODER_DIMS
N_ENCODER = 396927                                    # 393951 Linear + 2976 BatchNorm
N_DECODER = 542544
BN_EPS = RE.BN_EPS
BN_NAMES = RE.BN_NAMES


def _encoder_state():
    out = []
    for k, (i, o) in enumerate(zip(ENCODER_WIDTHS, ENCODER_WIDTHS[1:])):
        out += [(f"encoder.{3 * k}.weight", (o, i)), (f"encoder.{3 * k}.bias", (o,))]
        if k < len(ENCODER_WIDTHS) - 2:
            out += [(f"encoder.{3 * k + 1}.{n}", (o,)) for n in BN_NAMES]
    return tuple(out)


ENCODER_STATE = _encoder_state()   # AutoencoderMLP.encoder in state_dict order, without num_batches_tracked
DECODER_STATE = tuple(e for k, (i, o) in enumerate(zip(DECODER_WIDTHS, DECODER_WIDTHS[1:]))
                      for e in ((f"decoder.{2 * k}.weight", (o, i)), (f"decoder.{2 * k}.bias", (o,))))


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lang_single_stage.npz"))


class SingleStageAutoencoder(nn.Module):
    """AutoencoderMLP(ENCODER_DIMS, DECODER_DIMS) in its construction order (the default initialisation under a seed is then
    the reference module's), with encode and decode restated."""

    def __init__(self):
        super().__init__()
        enc = []
        for i, d in enumerate(ENCODER_DIMS):
            if i == 0:
                enc.append(nn.Linear(768, d))
            else:
                enc += [nn.BatchNorm1d(ENCODER_DIMS[i - 1]), nn.ReLU(), nn.Linear(ENCODER_DIMS[i - 1], d)]
        self.encoder = nn.ModuleList(enc)
        dec = []
        for i, d in enumerate(DECODER_DIMS):
            if i == 0:
                dec.append(nn.Linear(ENCODER_DIMS[-1], d))
            else:
                dec += [nn.ReLU(), nn.Linear(DECODER_DIMS[i - 1], d)]
        self.decoder = nn.ModuleList(dec)

    def encode(self, x):
        for m in self.encoder:
            x = m(x)
        return x / x.norm(dim=-1, keepdim=True)

    def decode(self, x):
        for m in self.decoder:
            x = m(x)
        return x / x.norm(dim=-1, keepdim=True)


def module_state(seed):
    """-> (encoder state, decoder state) of the module's default initialisation under torch.manual_seed(seed), float32, in
    state_dict order.  The BatchNorm entries are not the identity (the default state, weight 1 / bias 0 / mean 0 / var 1, would
    hide a wrong plane order): drawn from lang_encoder_ref.encoder_state's ranges, running_mean ~ U(-0.2, 0.2), running_var ~
    U(0.05, 1.5), weight ~ U(0.5, 1.5), bias ~ U(-0.3, 0.3)."""
    torch.manual_seed(seed)
    sd = SingleStageAutoencoder().state_dict()
    g = torch.Generator().manual_seed(5000 + seed)
    ranges = dict(running_mean=(-0.2, 0.2), running_var=(0.05, 1.5), weight=(0.5, 1.5), bias=(-0.3, 0.3))
    enc = OrderedDict()
    for k, shape in ENCODER_STATE:
        layer, name = k.split(".")[1:]
        if int(layer) % 3 == 1:
            lo, hi = ranges[name]
            enc[k] = (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)).float()
        else:
            enc[k] = sd[k].clone()
        assert tuple(enc[k].shape) == tuple(shape), k
    dec = OrderedDict((k, sd[k].clone()) for k, _ in DECODER_STATE)
    assert all(tuple(dec[k].shape) == tuple(s) for k, s in DECODER_STATE)
    return enc, dec


def encoder_state(seed):
    return module_state(seed)[0]


def decoder_state(seed):
    return module_state(seed)[1]


def flatten_encoder(state):
    return torch.cat([state[k].detach().reshape(-1) for k, _ in ENCODER_STATE])


def flatten_decoder(state):
    return torch.cat([state[k].detach().reshape(-1) for k, _ in DECODER_STATE])


def module_from(state, dtype):
    """The restated module in eval() with `state`'s entries (encoder, decoder or both; the rest keeps what the constructor
    drew)."""
    m = SingleStageAutoencoder().to(dtype)
    missing = m.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=False)
    assert not missing.unexpected_keys
    return m.eval()


make_features = RE.make_features   # unit float32 rows [N,768] that share most of their direction, as CLIP rows do
rows_of = RE.rows_of               # [N,768] as it is; [768,h,w] or [B,768,h,w] -> permute(0,2,3,1).view(-1,768)


def unit_codes(n, seed):
    """Unit float32 code rows [n,15]."""
    g = torch.Generator().manual_seed(6000 + seed)
    v = torch.randn(n, ENCODER_DIMS[-1], generator=g, dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True)).float()


def encode(state, features, dtype, chunk=8192):
    """auto_model.encode(rows) in `dtype` -> [N,15]."""
    m = module_from(state, dtype)
    rows = rows_of(features).to(dtype)
    with torch.no_grad():
        return torch.cat([m.encode(rows[s:s + chunk]) for s in range(0, rows.shape[0], chunk)])


def decode(state, code_rows, dtype, chunk=8192):
    """model.decode(rows) in `dtype`: [n,15] -> [n,768]."""
    m = module_from(state, dtype)
    rows = code_rows.to(dtype)
    with torch.no_grad():
        return torch.cat([m.decode(rows[s:s + chunk]) for s in range(0, rows.shape[0], chunk)])


def similarities(codes, dec_state, phrases, dtype, decode_hw=None, chunk=8192):
    """codes [15,h,w] -> decode(codes) @ phrases.T as [K,H,W] in `dtype`: the codes resized to decode_hw first
    (evaluate_langslam.py:270, lang_query_ref.resize), then model.decode per pixel (:271-272) and get_relevancy's torch.mm."""
    m = module_from(dec_state, dtype)
    p = phrases.to(dtype)
    with torch.no_grad():
        c = codes.to(dtype)
        if decode_hw is not None and tuple(decode_hw) != tuple(c.shape[1:]):
            c = RQ.resize(c, decode_hw)
        h, w = c.shape[1:]
        rows = c.permute(1, 2, 0).reshape(-1, c.shape[0])
        out = torch.cat([torch.mm(m.decode(rows[s:s + chunk]), p.T) for s in range(0, rows.shape[0], chunk)])
    return out.T.reshape(-1, h, w).contiguous()


def least_norms(enc_state, features=None, dec_state=None, code_rows=None):
    """The smallest pre-norm |h6| of the encoder over `features` and |y| of the decoder over `code_rows`, in float64: how far a
    case is from the 0 / 0 of a zero row.  -> (|h6| or None, |y| or None)."""
    out = [None, None]
    with torch.no_grad():
        if features is not None:
            x = rows_of(features).double()
            for layer in module_from(enc_state, torch.float64).encoder:
                x = layer(x)
            out[0] = float(x.norm(dim=-1).min())
        if code_rows is not None:
            y = code_rows.double()
            for layer in module_from(dec_state, torch.float64).decoder:
                y = layer(y)
            out[1] = float(y.norm(dim=-1).min())
    return tuple(out)


# ---- the golden cases ------------------------------------------------------------------------------------------------------
# encode: key -> (shape of the input, seed): 70 rows, and a 9 x 13 channel-major map
ENCODE_CASES = OrderedDict([("rows70", ((70, 768), 0)), ("map9x13", ((768, 9, 13), 1))])
# decode: 70 unit code rows against 7 phrase rows; the full 768-wide decode is kept of every 7th row
DECODE_SEED, DECODE_ROWS, DECODE_PHRASES, DECODE_KEPT = 2, 70, 7, tuple(range(0, 70, 7))


def make_encode_case(key):
    """-> (encoder state, features in the case's shape)."""
    shape, seed = ENCODE_CASES[key]
    state = encoder_state(200 + seed)
    if len(shape) == 2:
        return state, make_features(shape[0], seed)
    _, h, w = shape
    return state, make_features(h * w, seed).t().contiguous().view(768, h, w)


def make_decode_case():
    """-> (decoder state, unit code rows [70,15], unit phrase rows [7,768])."""
    return decoder_state(200 + DECODE_SEED), unit_codes(DECODE_ROWS, DECODE_SEED), RQ.unit_rows(DECODE_PHRASES, DECODE_SEED)


# ---- query cases -----------------------------------------------------------------------------------------------------------
def object_phrases(dec_state, obj_codes, seed):
    """lang_query_ref.object_phrases for the single-stage decoder -> (raw, centred), float32 unit rows [n,768].  raw: the
    decoder's unit outputs f_k of the object codes.  centred: unit(unit(f_k - c) + 0.04 c) with c the mean output of 32 random
    unit codes: with default initialisation the decoder sends every code to nearly the same direction, and a phrase that
    matches what is particular about the object, as a text embedding does on trained weights, is what gives the relevancy a
    range that the mask's min / max normalisation can work on."""
    g = torch.Generator().manual_seed(3000 + seed)
    generic = torch.randn(32, 15, generator=g, dtype=torch.float64)
    generic = generic / generic.norm(dim=1, keepdim=True)
    c = decode(dec_state, generic, torch.float64).mean(dim=0)
    f = decode(dec_state, obj_codes.double(), torch.float64)
    u = f - c
    u = u / u.norm(dim=1, keepdim=True) + 0.04 * c
    return f.float(), (u / u.norm(dim=1, keepdim=True)).float()


def make_query_case(h, w, seed, n_pos, n_labels, n_neg=4):
    """-> dict(codes [15,h,w], dec_state, obj [n,15], pos, neg, labels): lang_query_ref.make_case without the online decoder."""
    n_obj = max(n_pos, n_labels)
    codes, obj = RQ.make_codes(h, w, seed, n_obj)
    dec_state = decoder_state(100 + seed)
    _, centred = object_phrases(dec_state, obj, seed)
    lab = centred[:max(n_labels, RQ.N_OBJECTS)].flip(0)[:n_labels].contiguous() if n_labels else None
    return dict(codes=codes, dec_state=dec_state, obj=obj, pos=centred[:n_pos].contiguous(), neg=RQ.unit_rows(n_neg, seed), labels=lab)


def query(case, dtype, thresh, decode_hw=None):
    """The whole query of `case` in `dtype` at the decode size: model.decode, the products, then lang_query_ref's statements of
    get_relevancy, the 30 x 30 mean, the mask and get_semantic_map.  Phrase rows are [pos | labels | neg]."""
    pos, neg, labels = case["pos"], case["neg"], case["labels"]
    n_lab = 0 if labels is None else labels.shape[0]
    phrases = torch.cat([pos] + ([labels] if n_lab else []) + [neg])
    out = dict(sims=similarities(case["codes"], case["dec_state"], phrases, dtype, decode_hw=decode_hw))
    out["sims_dec"] = out["sims"]
    out["relevancy"] = RQ.relevancy(out["sims"], pos.shape[0], neg.shape[0])
    out.update(RQ.localise(out["relevancy"], thresh))
    if n_lab:
        out["labels"], out["label_margin"] = RQ.semantic_map(out["sims"], pos.shape[0], n_lab, neg.shape[0])
    return out
