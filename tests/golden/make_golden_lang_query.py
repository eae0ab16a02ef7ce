"""Generates tests/golden/lang_query.npz: the reference's OWN modules and functions for a text query on a code map, run on
the CPU in float64 ("truth", *_f64) and float32 ("ref32", *_f32).  Runs ONLY where the reference checkout exists; the
committed .npz is data (arrays only).

What is executed from the reference: EncoderDecoderOnline.decode and AutoencoderMLP.decode (language/autoencoder/model.py),
OpenCLIPNetwork.get_relevancy / get_max_across / get_semantic_map (eval/openclip_encoder.py, imported with open_clip and
torchvision stubbed; the network object is made with object.__new__ and positives, negatives, pos_embeds, neg_embeds,
semantic_embeds set by hand, so no CLIP model is loaded; the eval package itself is entered as a bare namespace, since its
__init__ imports colour tools that are not installed), and torch's own F.interpolate for the statements of
eval/evaluate_onlinelangslam.py:270-274.

What is NOT executed: cv2 is not installed here, so cv2.filter2D cannot be called.  The 30 x 30 mean is the restatement of
tests/lang_query_ref.py (OpenCV's documented defaults: correlation, anchor (15,15), BORDER_REFLECT_101), cross-checked below
against scipy.ndimage.correlate(mode="mirror"); `*_smoothed_f64` is scipy's result.  That part of the file is pinned by
restatement, not by running the reference's call.

Weights: no trained checkpoint exists where this file is made; both decoders carry nn.Linear's default initialisation under
a seed (the general one drawn through the reference's AutoencoderMLP constructor, encoder first).  Phrases
(lang_query_ref.object_phrases): the normalised decoder outputs of the case's object codes themselves cannot serve as
phrases: with default initialisation every pixel decodes to nearly the same direction, their relevancy is 0.9999 everywhere, and
the min / max normalised mask of the float32 reference run itself then differs from the float64 one in a third of the pixels
(measured: 627 of 1920).  As labels they leave margins of 1e-4 between the best and the second-best
similarity.  The positives and labels are those outputs centred on the mean decoder output, whose relevancy spans 0.41 - 0.61,
crosses 0.5 at the object and gives masks of 12 - 24 %; the negatives are random unit rows (purely random positives leave the
relevancy in 0.38 - 0.47, flat, and the mask as ill-conditioned).

Per case (tests/lang_query_ref.GOLDEN_CASES): codes [15,h,w], pos / neg / labels float32, the seeds of the weights; then in
both precisions relevancy [P,H,W] and the label map, in float64 the features of every 97th row and the resized codes, and of
the float32 run's features the largest error.  `*_excluded_ref32`: {the largest number of pixels of a discrete map that lie within
the float32 run's tolerance of their decision, the largest number that differ between the two runs}, both asserted to be at most
0.1 % of a map."""
import os
import sys
import types

import numpy as np
import torch
from scipy import ndimage
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OLSR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import lang_codec_ref as RC  # noqa: E402
import lang_query_ref as R  # noqa: E402

for name in ("lightning", "lightning.pytorch", "open_clip", "torchvision", "torchvision.models", "eval.colormaps"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["lightning.pytorch"].LightningModule = nn.Module
sys.modules["lightning"].pytorch = sys.modules["lightning.pytorch"]
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
sys.modules["eval.colormaps"].apply_pca_colormap = None
# the eval package's __init__ imports its colour tools (jaxtyping, matplotlib); the one module wanted here needs none of them
sys.modules["eval"] = types.ModuleType("eval")
sys.modules["eval"].__path__ = [os.path.join(REF, "eval")]

from eval.openclip_encoder import OpenCLIPNetwork  # noqa: E402
from language.autoencoder.model import AutoencoderMLP, EncoderDecoderOnline  # noqa: E402


def reference_models(case, seed, dtype):
    online = EncoderDecoderOnline().to(dtype)
    online.load_state_dict({k: v.to(dtype) for k, v in RC.unflatten(case["online"]).items()})
    torch.manual_seed(100 + seed)
    general = AutoencoderMLP(list(R.ENCODER_DIMS), list(R.WIDTHS[1:]))
    for k, v in case["dec_state"].items():   # the restated constructor draws what the reference's does
        assert torch.equal(general.state_dict()[k], v), k
    return online, general.to(dtype)


def clip_network(case, dtype):
    net = object.__new__(OpenCLIPNetwork)
    net.positives = tuple(f"positive {k}" for k in range(case["pos"].shape[0]))
    net.negatives = ("object", "things", "stuff", "texture")
    net.pos_embeds, net.neg_embeds = case["pos"].to(dtype), case["neg"].to(dtype)
    if case["labels"] is not None:
        net.semantic_embeds = case["labels"].to(dtype)
    return net


def run_reference(case, seed, decode_hw, out_hw, dtype):
    """evaluate_onlinelangslam.py:266-274 and the OpenCLIPNetwork calls of activate_stream / lerf_localization, one level."""
    online, general = reference_models(case, seed, dtype)
    net = clip_network(case, dtype)
    with torch.no_grad():
        sem_feat = case["codes"].to(dtype).permute(1, 2, 0)[None]   # [lvl,h,w,15], as np.load gives it
        lvl, h, w, _ = sem_feat.shape
        new_h, new_w = (h, w) if decode_hw is None else decode_hw
        out_h, out_w = (h, w) if out_hw is None else out_hw
        if (new_h, new_w) != (h, w):
            c15 = torch.nn.functional.interpolate(sem_feat.permute(0, 3, 1, 2), size=(new_h, new_w), mode="bilinear",
                                                  align_corners=False).permute(0, 2, 3, 1)
        else:
            c15 = sem_feat
        f32 = online.decode(c15.flatten(0, 2))
        restored = general.decode(f32).view(lvl, new_h, new_w, -1)
        if (out_h, out_w) != (new_h, new_w):
            restored_feat = torch.nn.functional.interpolate(restored.permute(0, 3, 1, 2), size=(out_h, out_w), mode="bilinear",
                                                            align_corners=False).permute(0, 2, 3, 1)
        else:
            restored_feat = restored
        out = dict(codes_resized=c15[0].permute(2, 0, 1), feat=restored_feat[0].reshape(-1, 768),
                   relevancy=net.get_max_across(restored_feat)[0])
        if case["labels"] is not None:
            out["labels"] = net.get_semantic_map(restored_feat)[0]
    return out


def main():
    out = dict(thresh=np.float64(R.THRESH), feat_row_stride=np.int32(R.FEAT_ROW_STRIDE),
               state_names=np.array([k for k, _ in R.STATE]), state_shapes=np.array([list(s) + [0] * (2 - len(s)) for _, s in R.STATE]))
    for key, (h, w, decode_hw, out_hw, seed, n_pos, n_lab) in R.GOLDEN_CASES.items():
        case = R.make_case(h, w, seed, n_pos, n_lab)
        out[f"{key}_codes"] = case["codes"].numpy()
        out[f"{key}_pos"], out[f"{key}_neg"] = case["pos"].numpy(), case["neg"].numpy()
        if n_lab:
            out[f"{key}_label_embeds"] = case["labels"].numpy()
        out[f"{key}_seed"] = np.int32(seed)
        r64 = run_reference(case, seed, decode_hw, out_hw, torch.float64)
        r32 = run_reference(case, seed, decode_hw, out_hw, torch.float32)
        sub = slice(None, None, R.FEAT_ROW_STRIDE)
        out[f"{key}_feat_f64"] = r64["feat"][sub].numpy()
        out[f"{key}_feat_f32_maxerr"] = np.float64((r32["feat"].double() - r64["feat"]).abs().max())
        out[f"{key}_codes_resized_f64"] = r64["codes_resized"].numpy()
        out[f"{key}_relevancy_f64"], out[f"{key}_relevancy_f32"] = r64["relevancy"].numpy(), r32["relevancy"].numpy()
        H, W = r64["relevancy"].shape[1:]
        # the filter: the restatement against scipy (correlate's window for an even size is -size//2 .. size//2 - 1)
        kernel = np.ones((R.WINDOW, R.WINDOW)) / (R.WINDOW ** 2)
        sm = np.stack([ndimage.correlate(p, kernel, mode="mirror") for p in out[f"{key}_relevancy_f64"]])
        mine = R.box_mean(r64["relevancy"]).numpy()
        assert np.abs(sm - mine).max() < 1e-13, np.abs(sm - mine).max()
        out[f"{key}_smoothed_f64"] = sm
        q64, q32 = (R.query(case["codes"], case["online"], case["dec_state"], case["pos"], case["neg"], case["labels"], dt,
                            thresh=R.THRESH, decode_hw=decode_hw, out_hw=out_hw) for dt in (torch.float64, torch.float32))
        q64["relevancy"], q32["relevancy"] = r64["relevancy"], r32["relevancy"]
        q64.update(R.localise(r64["relevancy"], R.THRESH)), q32.update(R.localise(r32["relevancy"], R.THRESH))
        l64 = q64
        differ = [int((q64["mask"] != q32["mask"]).sum(dim=(1, 2)).max())]
        if n_lab:
            out[f"{key}_labels_f64"], out[f"{key}_labels_f32"] = r64["labels"].numpy().astype(np.int32), r32["labels"].numpy().astype(np.int32)
            differ.append(int((r64["labels"] != r32["labels"]).sum()))
        # the discrete rule of the GPU tests, applied to the float32 run: pixels within the tolerance of their decision
        excluded = R.undecided(q64, q32, R.THRESH)
        assert max(excluded.values()) <= R.EXCLUDED_CAP * H * W and max(differ) <= R.EXCLUDED_CAP * H * W, (key, excluded, differ)
        out[f"{key}_excluded_ref32"] = np.int32([max(excluded.values()), max(differ)])
        excluded = (excluded, differ)
        rel = out[f"{key}_relevancy_f64"]
        print(f"{key}: {H} x {W}; relevancy {rel.min():.3f} .. {rel.max():.3f}, above 0.5 in {float((rel > 0.5).mean()):.3f} of the "
              f"pixels; mask covers {[round(float(m.float().mean()), 3) for m in l64['mask']]}; features ref32 error "
              f"{out[f'{key}_feat_f32_maxerr']:.3e}, relevancy ref32 error "
              f"{np.abs(out[f'{key}_relevancy_f32'].astype(np.float64) - rel).max():.3e}; ref32 discrete differences {excluded}")
    path = os.path.join(HERE, "lang_query.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
