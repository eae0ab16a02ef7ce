"""Torch restatement of the reference's text-query path on a language code map, dtype-generic and on the CPU: the yardstick
of tests/test_gpu_lang_query.py (float64 = "truth", float32 = "ref32") at sizes too large to commit.

    eval/evaluate_onlinelangslam.py:266-287   F.interpolate of the codes (:270), model_online.decode, model.decode,
                                              F.interpolate of the 768-channel features (:274)
    language/autoencoder/model.py:58-62       AutoencoderMLP.decode (Linear / ReLU chain, x / x.norm(dim=-1, keepdim=True))
    eval/openclip_encoder.py:44-107           get_relevancy, get_max_across, get_semantic_map
    eval/evaluate_onlinelangslam.py:107-236   the 30 x 30 cv2.filter2D mean, 0.5 (avg + rel), max point, min / max, mask

tests/test_lang_query_ref_golden.py pins this module to arrays recorded from the reference's own modules and functions
(tests/golden/make_golden_lang_query.py -> lang_query.npz).  cv2 is not available where the golden file is made, so the
filter is RESTATED here from OpenCV's documented defaults (filter2D computes a correlation, anchor (-1,-1) = the kernel
centre (15,15) of a 30 x 30 kernel, so the window covers -15 .. +14; borderType BORDER_REFLECT_101 = gfedcb|abcdefgh|gfedcba)
and cross-checked there against scipy.ndimage.correlate(mode="mirror"): that part is pinned by restatement, not execution.

The feature image [N,768] is formed in row chunks only (in float64 it would take 5 GB at 1200 x 680); the statements per
row are the reference's.
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import lang_codec_ref as RC

WIDTHS = (32, 192, 256, 384, 512, 768)            # evaluate_onlinelangslam.py --decoder_dims behind the 32-wide code
ENCODER_DIMS = (512, 256, 128, 64, 32)            # --encoder_dims: built first, so it draws from the generator first
STATE = tuple(e for k, (i, o) in enumerate(zip(WIDTHS, WIDTHS[1:]))
              for e in ((f"decoder.{2 * k}.weight", (o, i)), (f"decoder.{2 * k}.bias", (o,))))
N_DECODER = 745536
WINDOW, ANCHOR = 30, 15
FEAT_ROW_STRIDE = 97   # the golden file keeps the features of every 97th row
EXCLUDED_CAP = 1e-3    # discrete outputs: at most 0.1 % of a map may lie within the tolerance of a decision


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lang_query.npz"))


class GeneralAutoencoder(nn.Module):
    """AutoencoderMLP(ENCODER_DIMS, WIDTHS[1:]) in its construction order (the default initialisation under a seed is then
    the reference module's); only decode is restated."""

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
        for i, d in enumerate(WIDTHS[1:]):
            if i == 0:
                dec.append(nn.Linear(ENCODER_DIMS[-1], d))
            else:
                dec += [nn.ReLU(), nn.Linear(WIDTHS[i], d)]
        self.decoder = nn.ModuleList(dec)

    def decode(self, x):
        for m in self.decoder:
            x = m(x)
        return x / x.norm(dim=-1, keepdim=True)


def decoder_state(seed):
    """The decoder entries of the module's default initialisation under torch.manual_seed(seed): float32, state_dict order."""
    torch.manual_seed(seed)
    sd = GeneralAutoencoder().state_dict()
    return OrderedDict((k, sd[k].clone()) for k, _ in STATE)


def flatten(state):
    return torch.cat([state[k].detach().reshape(-1) for k, _ in STATE])


def decoder_from(state, dtype):
    m = GeneralAutoencoder().to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=False)
    return m


# ---- the code map and the phrases of a case --------------------------------------------------------------------------------
N_OBJECTS = 3


def make_codes(h, w, seed, n_obj=N_OBJECTS):
    """A unit-norm code map [15,h,w] float32: a smooth background, N_OBJECTS discs of one code each, 5 % noise.
    -> (codes, object codes [n_obj,15] float32; the first N_OBJECTS are the discs', the others appear nowhere)."""
    g = torch.Generator().manual_seed(1000 + seed)
    low = torch.randn(1, 15, 4, 5, generator=g, dtype=torch.float64)
    bg = F.interpolate(low, size=(h, w), mode="bicubic", align_corners=True)[0]
    bg = bg / bg.norm(dim=0, keepdim=True)
    obj = torch.randn(max(n_obj, N_OBJECTS), 15, generator=g, dtype=torch.float64)
    obj = obj / obj.norm(dim=1, keepdim=True)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    c = bg.clone()
    for k in range(N_OBJECTS):
        cy, cx = (0.25 + 0.25 * k) * h, (0.2 + 0.3 * k) * w
        r = 0.16 * min(h, w) + 1.0
        inside = ((yy - cy) ** 2 + (xx - cx) ** 2) <= r * r
        c[:, inside] = obj[k][:, None]
    c = c + 0.05 * torch.randn(15, h, w, generator=g, dtype=torch.float64) / 15 ** 0.5
    c = c / c.norm(dim=0, keepdim=True)
    return c.float().contiguous(), obj.float()


def unit_rows(n, seed):
    g = torch.Generator().manual_seed(2000 + seed)
    v = torch.randn(n, 768, generator=g, dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True)).float()


def object_phrases(online_flat, dec_state, obj_codes, seed):
    """-> (raw, centred), float32 unit rows [n,768].  raw: the normalised decoder outputs f_k of the object codes, which no case
    uses as a phrase: with default
    initialisation the decoders send every code to nearly the same direction (cosines 0.998 - 1 between any two pixels), so
    against f_k the relevancy is 0.9999 everywhere and a mask normalised by min / max is rounding noise, in float32 torch as
    anywhere.  centred: unit(unit(f_k - c) + 0.04 c) with c the mean output of 32 random codes: a phrase that matches what
    is particular about the object, as a text embedding does on trained weights; its relevancy spans 0.41 - 0.61 and crosses 0.5
    at the object."""
    codec, dec = RC.codec_from(online_flat, torch.float64), decoder_from(dec_state, torch.float64)
    g = torch.Generator().manual_seed(3000 + seed)
    generic = torch.randn(32, 15, generator=g, dtype=torch.float64)
    generic = generic / generic.norm(dim=1, keepdim=True)
    with torch.no_grad():
        c = dec.decode(codec.decode(generic)).mean(dim=0)
        f = dec.decode(codec.decode(obj_codes.double()))
    u = f - c
    u = u / u.norm(dim=1, keepdim=True) + 0.04 * c
    return f.float(), (u / u.norm(dim=1, keepdim=True)).float()


# ---- the reference's statements --------------------------------------------------------------------------------------------
def resize(x, hw):
    """[C,h,w] -> [C,H,W]: F.interpolate(mode="bilinear", align_corners=False), the statement of :270 and :274."""
    return F.interpolate(x[None], size=tuple(hw), mode="bilinear", align_corners=False)[0]


def taps(n_in, n_out, dtype):
    """The taps of that interpolation along one axis (ATen UpSample.h: area_pixel_compute_source_index,
    guard_index_and_lambda), in `dtype`: (i0, i1, l0, l1)."""
    scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
    src = scale * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5
    src = torch.clamp(src, min=0)
    i0 = torch.clamp(src.long(), max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = torch.clamp(src - i0.to(dtype), 0, 1)
    return i0, i1, 1 - l1, l1


def resize_rows(x, ty, tx):
    """x [h,w,C] -> rows ty (a slice of taps(h, H)) x all columns tx = taps(w, W): [len(ty), W, C], the same interpolation
    written out so that an image too large to hold can be produced in row blocks (pinned to F.interpolate in the golden test)."""
    i0, i1, l0, l1 = ty
    j0, j1, m0, m1 = tx
    top, bot = x[i0], x[i1]
    a = m0[None, :, None] * top[:, j0] + m1[None, :, None] * top[:, j1]
    b = m0[None, :, None] * bot[:, j0] + m1[None, :, None] * bot[:, j1]
    return l0[:, None, None] * a + l1[:, None, None] * b


def features(codes_rows, codec, dec):
    """[n,15] -> [n,768]: model.decode(model_online.decode(rows)) (:271-272)."""
    return dec.decode(codec.decode(codes_rows))


def similarities(codes, online_flat, dec_state, phrases, dtype, decode_hw=None, out_hw=None, chunk=16384):
    """codes [15,h,w] -> embed @ p.T as [K,H,W] in `dtype`: codes resized to decode_hw (:270), decoded (:271-272), the features
    resized to out_hw when it differs (:274), then get_relevancy's torch.mm."""
    codec, dec = RC.codec_from(online_flat, dtype), decoder_from(dec_state, dtype)
    p = phrases.to(dtype)
    with torch.no_grad():
        c = codes.to(dtype)
        if decode_hw is not None and tuple(decode_hw) != tuple(c.shape[1:]):
            c = resize(c, decode_hw)
        h, w = c.shape[1:]
        rows = c.permute(1, 2, 0).reshape(-1, 15)
        if out_hw is None or tuple(out_hw) == (h, w):
            out = torch.cat([torch.mm(features(rows[s:s + chunk], codec, dec), p.T) for s in range(0, rows.shape[0], chunk)])
            return out.T.reshape(-1, h, w).contiguous()
        H, W = out_hw
        ty, tx = taps(h, H, dtype), taps(w, W, dtype)
        step = max(1, chunk // W)
        blocks = []
        for y0 in range(0, H, step):
            sl = [t[y0:y0 + step] for t in ty]
            lo, hi = int(sl[0].min()), int(sl[1].max())
            feat = features(rows[lo * w:(hi + 1) * w], codec, dec).view(hi - lo + 1, w, -1)
            up = resize_rows(feat, (sl[0] - lo, sl[1] - lo, sl[2], sl[3]), tx)
            blocks.append(torch.mm(up.reshape(-1, up.shape[-1]), p.T))
        return torch.cat(blocks).T.reshape(-1, H, W).contiguous()


def relevancy(sims, n_pos, n_neg):
    """sims [K,H,W] with the negatives as the last n_neg rows -> [n_pos,H,W]: get_relevancy's statements after the torch.mm,
    then get_max_across' probs[..., 0:1], per positive."""
    K, H, W = sims.shape
    output = sims.reshape(K, -1).T
    out = []
    for positive_id in range(n_pos):
        positive_vals = output[..., positive_id:positive_id + 1]
        negative_vals = output[..., K - n_neg:]
        repeated_pos = positive_vals.repeat(1, n_neg)
        s = torch.stack((repeated_pos, negative_vals), dim=-1)
        softmax = torch.softmax(10 * s, dim=-1)
        best_id = softmax[..., 0].argmin(dim=1)
        probs = torch.gather(softmax, 1, best_id[..., None, None].expand(best_id.shape[0], n_neg, 2))[:, 0, :]
        out.append(probs[..., 0:1])
    return torch.stack(out).view(n_pos, H, W)


def semantic_map(sims, first, n_labels, n_neg):
    """get_semantic_map on the rows [first, first + n_labels) and the negatives -> (labels int64 [H,W] with -1 for a negative,
    margin [H,W] = best minus second-best similarity, the value the decision hangs on)."""
    K, H, W = sims.shape
    output = torch.cat([sims[first:first + n_labels], sims[K - n_neg:]]).reshape(n_labels + n_neg, -1).T
    softmax = torch.softmax(10 * output, dim=-1)
    pred = torch.argmax(softmax, dim=-1)
    pred[pred >= n_labels] = -1
    top = output.topk(2, dim=-1).values
    return pred.view(H, W), (top[:, 0] - top[:, 1]).view(H, W)


def reflect101(i, n):
    """BORDER_REFLECT_101 index (numpy int array) into an axis of n elements, for any distance beyond the border."""
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def box_mean(x):
    """x [P,H,W] -> cv2.filter2D(x, -1, np.ones((30, 30)) / 900) per plane, restated: correlation with the window -15 .. +14
    on a reflect-101 border, in x's dtype."""
    P, H, W = x.shape
    iy = torch.from_numpy(reflect101(np.arange(-ANCHOR, H + WINDOW - 1 - ANCHOR), H)).to(x.device)
    ix = torch.from_numpy(reflect101(np.arange(-ANCHOR, W + WINDOW - 1 - ANCHOR), W)).to(x.device)
    padded = x[:, iy][:, :, ix]
    kernel = torch.full((1, 1, WINDOW, WINDOW), 1.0 / (WINDOW * WINDOW), dtype=torch.float64).to(device=x.device, dtype=x.dtype)
    return F.conv2d(padded[:, None], kernel)[:, 0]


def localise(rel, thresh):
    """rel [P,H,W] -> dict: smoothed (avg_filtered), blended (0.5 (avg + rel)), score (avg.max()), coords (every (x, y) of that
    maximum, as np.nonzero(...)[..., ::-1]), minmax of blended, normed (the map of :146-150 the threshold is applied to), mask."""
    avg = box_mean(rel)
    blended = 0.5 * (avg + rel)
    P = rel.shape[0]
    score = avg.reshape(P, -1).max(dim=1).values
    coords = [torch.nonzero(avg[k] == score[k]).flip(-1) for k in range(P)]
    normed, minmax = [], []
    for k in range(P):
        output = blended[k]
        minmax.append(torch.stack([torch.min(output), torch.max(output)]))
        output = output - torch.min(output)
        output = output / (torch.max(output) + 1e-9)
        output = output * (1.0 - (-1.0)) + (-1.0)
        normed.append(torch.clip(output, 0, 1))
    normed = torch.stack(normed)
    return dict(smoothed=avg, blended=blended, score=score, coords=coords, minmax=torch.stack(minmax), normed=normed,
                mask=(normed > thresh).to(torch.uint8))


def query(codes, online_flat, dec_state, pos, neg, labels, dtype, thresh=0.4, decode_hw=None, out_hw=None):
    """The whole path in `dtype`.  Phrase rows are [pos | labels | neg], as the library orders them."""
    n_pos, n_lab, n_neg = pos.shape[0], 0 if labels is None else labels.shape[0], neg.shape[0]
    phrases = torch.cat([pos] + ([labels] if n_lab else []) + [neg])
    out = dict(sims_dec=similarities(codes, online_flat, dec_state, phrases, dtype, decode_hw=decode_hw))
    hw = tuple(codes.shape[1:]) if out_hw is None else tuple(out_hw)
    if tuple(out["sims_dec"].shape[1:]) == hw:
        out["sims"] = out["sims_dec"]
    else:
        out["sims"] = similarities(codes, online_flat, dec_state, phrases, dtype, decode_hw=decode_hw, out_hw=hw)
    out["relevancy"] = relevancy(out["sims"], n_pos, n_neg)
    out.update(localise(out["relevancy"], thresh))
    if n_lab:
        out["labels"], out["label_margin"] = semantic_map(out["sims"], n_pos, n_lab, n_neg)
    return out


# ---- the golden cases ------------------------------------------------------------------------------------------------------
# key -> (h, w, decode_hw, out_hw, seed, positives, labels)
GOLDEN_CASES = OrderedDict([
    ("direct", (40, 48, None, None, 0, 3, 5)),
    ("resized", (36, 44, (24, 30), (36, 44), 1, 2, 0)),
])
THRESH = 0.4


def make_case(h, w, seed, n_pos, n_labels, n_neg=4):
    """-> dict(codes, online, dec_state, pos, neg, labels).  Positives and labels: centred object phrases (object_phrases), the
    labels in the opposite order.  Negatives: random unit rows."""
    n_obj = max(n_pos, n_labels)
    codes, obj = make_codes(h, w, seed, n_obj)
    online, dec_state = RC.initial_params(seed), decoder_state(100 + seed)
    _, centred = object_phrases(online, dec_state, obj, seed)
    lab = centred[:max(n_labels, N_OBJECTS)].flip(0)[:n_labels].contiguous() if n_labels else None
    return dict(codes=codes, online=online, dec_state=dec_state, pos=centred[:n_pos].contiguous(), neg=unit_rows(n_neg, seed),
                labels=lab)


# ---- the rule for discrete outputs -----------------------------------------------------------------------------------------
ULP2 = 4.0 * 2.0 ** -24


def tolerance(truth, ref32):
    """The continuous yardstick's bound on max|x - truth|: max(4 max|ref32 - truth|, 4 * 2^-24 max|truth|)."""
    truth = truth.double()
    return max(4.0 * float((ref32.double() - truth).abs().max()), ULP2 * float(truth.abs().max()))


def undecided(t64, t32, thresh):
    """Per discrete map, how many of the truth's pixels lie within the tolerance of their decision (they are excluded from the
    comparison, and may be at most EXCLUDED_CAP of the map): -> dict name -> count."""
    tol = tolerance(t64["normed"], t32["normed"])
    out = {f"mask[{p}]": int(((t64["normed"][p] - thresh).abs() <= tol).sum()) for p in range(t64["normed"].shape[0])}
    if "labels" in t64:
        out["labels"] = int((t64["label_margin"].abs() <= tolerance(t64["sims"], t32["sims"])).sum())
    return out
