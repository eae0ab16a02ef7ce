"""Generates tests/golden/clip_trunk.npz: the reference's OWN ConvNextBlock and LayerNorm (language/sed/modeling/transformer/
convnext.py:52-116) in eval(), run on the CPU in float64 ("truth", *_f64) and float32 ("ref32", *_f32) under no_grad.
Runs ONLY where the reference checkout exists; the committed .npz is data (arrays only).

The module is imported with timm.models.layers stubbed (DropPath = nn.Identity, which is what drop_path = 0 selects anyway,
and trunc_normal_ = torch's; neither takes part in a forward).  Parameters: drawn by clip_trunk_ref.block_state on a coarse
grid (multiples of 2^-9: exact in float32, and the compressed file stays small) and loaded into the reference's module under
its own names; gamma is overwritten by a drawn vector in [0.05, 0.2], since the reference's default of 1e-6 would hide the
whole branch.

Per case of clip_trunk_ref.GOLDEN_CASES (C = 64 and 192, on 5 x 7 and 1 x 1 maps): the input, truth and ref32; per width the
drawn parameters p<C>_<name> under the packed names (conv_dw, norm, mlp.fc1, mlp.fc2, gamma) as int16 multiples of 2^-grid.  Plus the LayerNorm in both data formats on one
[64,5,7] map: ln_x, ln_w, ln_b, ln_last_f64 / _f32 (channels_last, on the permuted map) and ln_first_f64 / _f32."""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OLSR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REF, "language", "sed", "modeling", "transformer"))
import clip_trunk_ref as R  # noqa: E402

_layers = types.ModuleType("timm.models.layers")
_layers.DropPath, _layers.trunc_normal_ = nn.Identity, nn.init.trunc_normal_
sys.modules.setdefault("timm", types.ModuleType("timm"))
sys.modules.setdefault("timm.models", types.ModuleType("timm.models"))
sys.modules["timm.models.layers"] = _layers

from convnext import ConvNextBlock, LayerNorm  # noqa: E402

GRID = 9
# the reference module's parameter names for the packed ones
NAMES = {"conv_dw.weight": "dwconv.weight", "conv_dw.bias": "dwconv.bias", "norm.weight": "norm.weight", "norm.bias": "norm.bias",
         "mlp.fc1.weight": "pwconv1.weight", "mlp.fc1.bias": "pwconv1.bias", "mlp.fc2.weight": "pwconv2.weight",
         "mlp.fc2.bias": "pwconv2.bias", "gamma": "gamma"}


def run_block(state, x, dtype):
    m = ConvNextBlock(x.shape[0])
    assert m.norm.eps == R.EPS and isinstance(m.drop_path, nn.Identity)
    m.load_state_dict({NAMES[k]: v for k, v in state.items()}, strict=True)
    m = m.to(dtype).eval()
    with torch.no_grad():
        return m(x.to(dtype)[None])[0]


def run_ln(x, w, b, fmt, dtype):
    m = LayerNorm(x.shape[0], eps=R.EPS, data_format=fmt)
    m.load_state_dict({"weight": w, "bias": b})
    m = m.to(dtype).eval()
    with torch.no_grad():
        if fmt == "channels_first":
            return m(x.to(dtype)[None])[0]
        return m(x.to(dtype).permute(1, 2, 0)[None])[0].permute(2, 0, 1)


def main():
    out = dict(ln_eps=np.float64(R.EPS), grid=np.int32(GRID))
    for key, (c, h, w, seed) in R.GOLDEN_CASES.items():
        state, x = R.block_state(c, c, grid=GRID), R.make_map(c, h, w, seed)
        out[f"{key}_x"] = x.numpy()
        for k, v in state.items():          # once per width, as integers: the value times 2^GRID
            q = torch.round(v * 2.0 ** GRID)
            assert torch.equal(q / 2.0 ** GRID, v) and float(q.abs().max()) < 32768
            out[f"p{c}_{k}"] = q.to(torch.int16).numpy()
        t64, t32 = run_block(state, x, torch.float64), run_block(state, x, torch.float32)
        assert t32.dtype == torch.float32 and torch.isfinite(t64).all()
        out[f"{key}_out_f64"], out[f"{key}_out_f32"] = t64.numpy(), t32.numpy()
        print(f"{key}: max|truth| {float(t64.abs().max()):.3f}, max|branch| {float((t64 - x.double()).abs().max()):.3f}, "
              f"max|ref32 - truth| {float((t32.double() - t64).abs().max()):.3e}")
    st = R.block_state(9, 64, grid=GRID)
    x, w, b = R.make_map(64, 5, 7, 9), st["norm.weight"], st["norm.bias"]
    out.update(ln_x=x.numpy(), ln_w=w.numpy(), ln_b=b.numpy())
    for fmt, tag in (("channels_last", "last"), ("channels_first", "first")):
        out[f"ln_{tag}_f64"] = run_ln(x, w, b, fmt, torch.float64).numpy()
        out[f"ln_{tag}_f32"] = run_ln(x, w, b, fmt, torch.float32).numpy()
    path = os.path.join(HERE, "clip_trunk.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
