"""Generates tests/golden/lang_encoder.npz: the reference's OWN AutoencoderMLP (language/autoencoder/model.py) in eval(), its
encode run on the CPU in float64 ("truth", *_f64) and float32 ("ref32", *_f32) on the statement of utils/slam_backend.py:
556-559 (permute(0,2,3,1).view(-1,768) for a map).  Runs ONLY where the reference checkout exists; the committed .npz is
data (arrays only).

The module is imported with lightning, open_clip, torchvision, matplotlib, sklearn and eval.colormaps stubbed (none of them
is touched by AutoencoderMLP).  Weights: no trained checkpoint exists where this file is made; the Linear layers carry
nn.Linear's default initialisation under a seed, drawn through the reference's constructor, and the BatchNorm entries are
drawn by lang_encoder_ref.encoder_state (the default BatchNorm state is the identity up to eps).  The restated state is
asserted equal to the module's, entry for entry.

Per case (tests/lang_encoder_ref.GOLDEN_CASES: 70 rows, and a 9 x 13 channel-major map): the input, the seed, both outputs
[N,32], the float32 run's largest error and the smallest |h5| (asserted >= 0.1: no row sits near the 0 / 0 of a zero row)."""
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
import lang_encoder_ref as R  # noqa: E402

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
    torch.manual_seed(200 + seed)
    m = AutoencoderMLP(list(R.WIDTHS[1:]), list(R.RQ.WIDTHS[1:]))
    sd = m.state_dict()
    for k, v in state.items():      # the restated constructor draws what the reference's does
        if int(k.split(".")[1]) % 3 != 1:
            assert torch.equal(sd[k], v), k
    assert [k for k in sd if k.startswith("encoder.") and not k.endswith("num_batches_tracked")] == [k for k, _ in R.STATE]
    m.load_state_dict(state, strict=False)
    for k, v in state.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert all(b.eps == R.BN_EPS for b in m.encoder if isinstance(b, nn.BatchNorm1d))
    return m.to(dtype).eval()


def run_reference(state, seed, features, dtype):
    m = reference_module(state, seed, dtype)
    with torch.no_grad():
        x = features.to(dtype)
        if x.dim() == 3:            # slam_backend.py:556-557 on clip_viz_dense [1,768,h,w]
            x = x[None].permute(0, 2, 3, 1).reshape(-1, 768)
        return m.encode(x)


def main():
    out = dict(bn_eps=np.float64(R.BN_EPS), state_names=np.array([k for k, _ in R.STATE]),
               state_shapes=np.array([list(s) + [0] * (2 - len(s)) for _, s in R.STATE]))
    for key, (shape, seed) in R.GOLDEN_CASES.items():
        state, features = R.make_case(key)
        assert tuple(features.shape) == tuple(shape)
        r64, r32 = (run_reference(state, seed, features, dt) for dt in (torch.float64, torch.float32))
        least = R.least_h5_norm(state, features)
        assert least >= 0.1, (key, least)
        mine64 = R.encode(state, features, torch.float64)
        assert float((mine64 - r64).abs().max()) <= 1e-12
        out[f"{key}_features"], out[f"{key}_seed"] = features.numpy(), np.int32(seed)
        out[f"{key}_out_f64"], out[f"{key}_out_f32"] = r64.numpy(), r32.numpy()
        out[f"{key}_out_f32_maxerr"] = np.float64((r32.double() - r64).abs().max())
        out[f"{key}_min_h5_norm"] = np.float64(least)
        print(f"{key}: input {tuple(features.shape)}, output {tuple(r64.shape)}; ref32 max error {out[f'{key}_out_f32_maxerr']:.3e}, "
              f"rms {float(((r32.double() - r64) ** 2).mean().sqrt()):.3e}; min |h5| {least:.3f}")
    path = os.path.join(HERE, "lang_encoder.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
