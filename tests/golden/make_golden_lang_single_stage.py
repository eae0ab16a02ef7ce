"""Generates tests/golden/lang_single_stage.npz: the reference's OWN AutoencoderMLP (language/autoencoder/model.py) with the
single-stage dimensions of utils/slam_backend.py:117-119, AutoencoderMLP([384,192,96,48,24,15], [24,48,96,192,384,384,768]),
in eval(), run on the CPU in float64 ("truth", *_f64) and float32 ("ref32", *_f32).  Runs ONLY where the reference checkout
exists; the committed .npz is data (arrays only).

The module is imported with the stubs of make_golden_lang_encoder.py (lightning, open_clip, torchvision, matplotlib, sklearn
and eval.colormaps: none of them is touched by AutoencoderMLP).  Weights: no trained checkpoint exists where this file is
made; the Linear layers carry nn.Linear's default initialisation under a seed, drawn through the reference's constructor, and
the BatchNorm entries are drawn by lang_single_stage_ref.module_state.  The restated state is asserted equal to the module's.

Encode cases (lang_single_stage_ref.ENCODE_CASES: 70 rows, and a 9 x 13 channel-major map on the statement of
slam_backend.py:556-557): the input, both outputs [N,15], the float32 run's largest error, the smallest |h6|.
Decode case: 70 unit code rows against 7 unit phrase rows: the similarities decode(rows) @ phrases.T as [7,70] and the full
768-wide decode of every 7th row, both in both precisions, the smallest |y|.
Asserted: the smallest pre-norm |h6| and |y| in float64 are >= 0.1, so no row sits near the 0 / 0 of a zero row."""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OLSR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import lang_single_stage_ref as R  # noqa: E402

for name in ("lightning", "lightning.pytorch", "open_clip", "torchvision", "torchvision.models", "eval.colormaps",
             "matplotlib", "matplotlib.pyplot", "sklearn", "sklearn.decomposition"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["lightning.pytorch"].LightningModule = nn.Module
sys.modules["lightning"].pytorch = sys.modules["lightning.pytorch"]
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
sys.modules["eval.colormaps"].apply_pca_colormap = None
if not hasattr(sys.modules["sklearn.decomposition"], "IncrementalPCA"):
    sys.modules["sklearn.decomposition"].IncrementalPCA = None
if not hasattr(sys.modules["matplotlib"], "pyplot"):
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
sys.modules["eval"] = types.ModuleType("eval")
sys.modules["eval"].__path__ = [os.path.join(REF, "eval")]

from language.autoencoder.model import AutoencoderMLP  # noqa: E402


def reference_module(state, seed, dtype):
    """The reference's module under the case's seed with `state` (encoder or decoder entries) loaded, in eval()."""
    torch.manual_seed(200 + seed)
    m = AutoencoderMLP(list(R.ENCODER_DIMS), list(R.DECODER_DIMS))
    sd = m.state_dict()
    for k, v in state.items():      # the restated constructor draws what the reference's does
        if k.startswith("decoder.") or int(k.split(".")[1]) % 3 != 1:
            assert torch.equal(sd[k], v), k
    assert [k for k in sd if k.startswith("encoder.") and not k.endswith("num_batches_tracked")] == [k for k, _ in R.ENCODER_STATE]
    assert [k for k in sd if k.startswith("decoder.")] == [k for k, _ in R.DECODER_STATE]
    assert sum(v.numel() for k, v in sd.items() if k.startswith("encoder.") and not k.endswith("num_batches_tracked")) == R.N_ENCODER
    assert sum(v.numel() for k, v in sd.items() if k.startswith("decoder.")) == R.N_DECODER
    m.load_state_dict(state, strict=False)
    for k, v in state.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert all(b.eps == R.BN_EPS for b in m.encoder if isinstance(b, nn.BatchNorm1d))
    return m.to(dtype).eval()


def run_encode(state, seed, features, dtype):
    m = reference_module(state, seed, dtype)
    with torch.no_grad():
        x = features.to(dtype)
        if x.dim() == 3:            # slam_backend.py:556-557 on clip_viz_dense [1,768,h,w]
            x = x[None].permute(0, 2, 3, 1).reshape(-1, 768)
        return m.encode(x)


def main():
    out = dict(bn_eps=np.float64(R.BN_EPS))
    for key, (shape, seed) in R.ENCODE_CASES.items():
        state, features = R.make_encode_case(key)
        assert tuple(features.shape) == tuple(shape)
        r64, r32 = (run_encode(state, seed, features, dt) for dt in (torch.float64, torch.float32))
        least, _ = R.least_norms(state, features)
        assert least >= 0.1, (key, least)
        assert float((R.encode(state, features, torch.float64) - r64).abs().max()) <= 1e-12
        out[f"{key}_features"], out[f"{key}_seed"] = features.numpy(), np.int32(seed)
        out[f"{key}_out_f64"], out[f"{key}_out_f32"] = r64.numpy(), r32.numpy()
        out[f"{key}_out_f32_maxerr"] = np.float64((r32.double() - r64).abs().max())
        out[f"{key}_min_h6_norm"] = np.float64(least)
        print(f"{key}: input {tuple(features.shape)}, output {tuple(r64.shape)}; ref32 max error {out[f'{key}_out_f32_maxerr']:.3e}, "
              f"rms {float(((r32.double() - r64) ** 2).mean().sqrt()):.3e}; min |h6| {least:.3f}")
    dec_state, rows, phrases = R.make_decode_case()
    kept = list(R.DECODE_KEPT)
    _, least = R.least_norms(None, None, dec_state, rows)
    assert least >= 0.1, least
    out["decode_codes"], out["decode_phrases"], out["decode_kept"] = rows.numpy(), phrases.numpy(), np.array(kept, dtype=np.int32)
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        m = reference_module(dec_state, R.DECODE_SEED, dt)
        with torch.no_grad():
            feat = m.decode(rows.to(dt))
            out[f"decode_sims_{tag}"] = torch.mm(feat, phrases.to(dt).T).T.contiguous().numpy()
            out[f"decode_features_{tag}"] = feat[kept].numpy()
    mine = R.similarities(rows.t().reshape(15, 1, -1), dec_state, phrases, torch.float64)
    assert float((mine[:, 0] - torch.from_numpy(out["decode_sims_f64"])).abs().max()) <= 1e-12
    out["decode_min_y_norm"] = np.float64(least)
    err = np.abs(out["decode_sims_f32"].astype(np.float64) - out["decode_sims_f64"]).max()
    print(f"decode: {rows.shape[0]} code rows x {phrases.shape[0]} phrases; ref32 max error of the similarities {err:.3e}; "
          f"min |y| {least:.3f}")
    path = os.path.join(HERE, "lang_single_stage.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "lang_query.npz"))


if __name__ == "__main__":
    main()
