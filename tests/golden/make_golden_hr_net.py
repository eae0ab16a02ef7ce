"""Generates tests/golden/hr_net.npz: the reference's OWN HighResLanguageFeatureNet (language/supervisedNet.py) in eval(), run
on the CPU in float64 ("truth", *_f64) and float32 ("ref32", *_f32) under no_grad, as utils/slam_backend.py:547-555 calls it.
Runs ONLY where the reference checkout exists; the committed .npz is data (arrays only).

The module is imported with pytorch_lightning stubbed (LightningModule = nn.Module; HighResLanguageFeatureNet does not touch
it).  Weights: no trained checkpoint exists where this file is made, and 80 MB of weights cannot be committed; the convolutions
carry their default initialisation under a seed, drawn through the reference's constructor, and the BatchNorm entries are drawn
by hr_net_ref.draw_batchnorm.  The restated state (hr_net_ref.net_state, what the tests regenerate from the seed) is asserted
equal to the module's, entry for entry.

Per case (hr_net_ref.GOLDEN_CASES): the three inputs, the seed, truth and ref32 at every pixel of the 32 output channels
hr_net_ref.GOLDEN_CHANNELS, and the max and rms error of the WHOLE ref32 output against truth."""
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
import hr_net_ref as R  # noqa: E402

sys.modules.setdefault("pytorch_lightning", types.ModuleType("pytorch_lightning"))
sys.modules["pytorch_lightning"].LightningModule = nn.Module

from language.supervisedNet import HighResLanguageFeatureNet  # noqa: E402


def reference_module(state, seed, dtype):
    torch.manual_seed(seed)
    m = HighResLanguageFeatureNet()
    sd = m.state_dict()
    assert [k for k in sd if not k.endswith("num_batches_tracked")] == [k for k, _ in R.STATE]
    bn = R.draw_batchnorm(seed)
    for k, v in state.items():      # the restated constructor draws what the reference's does
        if k not in bn:
            assert torch.equal(sd[k], v), k
    m.load_state_dict(state, strict=False)
    for k, v in state.items():
        assert torch.equal(m.state_dict()[k], v), k
    assert all(b.eps == R.BN_EPS for b in m.modules() if isinstance(b, nn.BatchNorm2d))
    return m.to(dtype).eval()


def run_reference(state, seed, inputs, dtype):
    m = reference_module(state, seed, dtype)
    with torch.no_grad():
        return m(*(x.to(dtype)[None] for x in inputs))[0]


def main():
    out = dict(bn_eps=np.float64(R.BN_EPS), channels=np.array(R.GOLDEN_CHANNELS, dtype=np.int32),
               state_names=np.array([k for k, _ in R.STATE]))
    ch = list(R.GOLDEN_CHANNELS)
    for key, (sizes, seed) in R.GOLDEN_CASES.items():
        state, inputs = R.make_case(key)
        r64, r32 = (run_reference(state, 300 + seed, inputs, dt) for dt in (torch.float64, torch.float32))
        mine64 = R.forward(state, *inputs, torch.float64)
        assert float((mine64 - r64).abs().max()) <= 1e-12
        emax, erms = R.err(r32, r64)
        for name, x in zip(("fv", "f3", "f2"), inputs):
            out[f"{key}_{name}"] = x.numpy()
        out[f"{key}_seed"] = np.int32(seed)
        out[f"{key}_out_f64"], out[f"{key}_out_f32"] = r64[ch].numpy(), r32[ch].numpy()
        out[f"{key}_out_f32_maxerr"], out[f"{key}_out_f32_rmserr"] = np.float64(emax), np.float64(erms)
        out[f"{key}_out_absmax"] = np.float64(r64.abs().max())
        print(f"{key}: sizes {sizes}, output {tuple(r64.shape)}, max |truth| {float(r64.abs().max()):.3f}; ref32 max error "
              f"{emax:.3e}, rms {erms:.3e}")
    path = os.path.join(HERE, "hr_net.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
