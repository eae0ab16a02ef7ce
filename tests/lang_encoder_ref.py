"""Torch restatement of the reference's general language encoder, dtype-generic and on the CPU: the yardstick of
tests/test_gpu_lang_encoder.py (float64 = "truth", float32 = "ref32") at sizes too large to commit.

    utils/slam_backend.py:556-559, :392-395   clip_viz_dense.permute(0,2,3,1).view(-1,768) -> auto_model.encode
    language/autoencoder/model.py:15-56       AutoencoderMLP: Linear 768 -> 512, then BatchNorm1d / ReLU / Linear down to
                                              256 -> 128 -> 64 -> 32, encode = the chain followed by x / x.norm(dim=-1)
    utils/slam_backend.py:142                 the module is in eval(): BatchNorm1d uses its running statistics

tests/test_lang_encoder_ref_golden.py pins this module to arrays recorded from the reference's own module
(tests/golden/make_golden_lang_encoder.py -> lang_encoder.npz).
"""
import os
from collections import OrderedDict

import numpy as np
import torch

import lang_query_ref as RQ

WIDTHS = (768, 512, 256, 128, 64, 32)     # clip_dim, then --encoder_dims of the two-stage chain
N_ENCODER = 572128                        # 568288 Linear + 3840 BatchNorm
BN_EPS = 1e-5                             # nn.BatchNorm1d's default
BN_NAMES = ("weight", "bias", "running_mean", "running_var")


def _state():
    out = []
    for k, (i, o) in enumerate(zip(WIDTHS, WIDTHS[1:])):
        out += [(f"encoder.{3 * k}.weight", (o, i)), (f"encoder.{3 * k}.bias", (o,))]
        if k < len(WIDTHS) - 2:
            out += [(f"encoder.{3 * k + 1}.{n}", (o,)) for n in BN_NAMES]
    return tuple(out)


STATE = _state()   # AutoencoderMLP.encoder in state_dict order, without num_batches_tracked
assert tuple(WIDTHS[1:]) == tuple(RQ.ENCODER_DIMS)


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lang_encoder.npz"))


class GeneralAutoencoder(RQ.GeneralAutoencoder):
    """lang_query_ref.GeneralAutoencoder (AutoencoderMLP in its construction order, so that the default initialisation under a
    seed is the reference module's) with encode restated."""

    def encode(self, x):
        for m in self.encoder:
            x = m(x)
        return x / x.norm(dim=-1, keepdim=True)


def encoder_state(seed):
    """The encoder entries of the module's default initialisation under torch.manual_seed(seed), with BatchNorm entries that
    are not the identity (the default state, weight 1 / bias 0 / mean 0 / var 1, would hide a wrong plane order):
    running_mean ~ U(-0.2, 0.2), running_var ~ U(0.05, 1.5), weight ~ U(0.5, 1.5), bias ~ U(-0.3, 0.3).  float32."""
    torch.manual_seed(seed)
    sd = GeneralAutoencoder().state_dict()
    g = torch.Generator().manual_seed(5000 + seed)
    ranges = dict(running_mean=(-0.2, 0.2), running_var=(0.05, 1.5), weight=(0.5, 1.5), bias=(-0.3, 0.3))
    out = OrderedDict()
    for k, shape in STATE:
        layer, name = k.split(".")[1:]
        if int(layer) % 3 == 1:
            lo, hi = ranges[name]
            out[k] = (lo + (hi - lo) * torch.rand(shape, generator=g, dtype=torch.float64)).float()
        else:
            out[k] = sd[k].clone()
        assert tuple(out[k].shape) == tuple(shape), k
    return out


def flatten(state):
    return torch.cat([state[k].detach().reshape(-1) for k, _ in STATE])


def encoder_from(state, dtype):
    """The restated module in eval() with `state`'s encoder (its decoder keeps whatever the constructor drew)."""
    m = GeneralAutoencoder().to(dtype)
    missing = m.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=False)
    assert not missing.unexpected_keys and all(not k.startswith("encoder.") for k in missing.missing_keys)
    return m.eval()


def make_features(N, seed):
    """Unit float32 rows [N,768] of randn + 2 (one shared randn row): CLIP rows share most of their direction."""
    g = torch.Generator().manual_seed(4000 + seed)
    shared = torch.randn(1, WIDTHS[0], generator=g, dtype=torch.float64)
    x = torch.randn(N, WIDTHS[0], generator=g, dtype=torch.float64) + 2.0 * shared
    return (x / x.norm(dim=1, keepdim=True)).float()


def rows_of(features):
    """[N,768] as it is; [768,h,w] or [B,768,h,w] -> permute(0,2,3,1).view(-1,768), the reference's statement."""
    if features.dim() == 2:
        return features
    if features.dim() == 3:
        features = features[None]
    return features.permute(0, 2, 3, 1).reshape(-1, WIDTHS[0])


def encode(state, features, dtype, chunk=8192):
    """auto_model.encode(rows) in `dtype` -> [N,32]."""
    m = encoder_from(state, dtype)
    rows = rows_of(features).to(dtype)
    with torch.no_grad():
        return torch.cat([m.encode(rows[s:s + chunk]) for s in range(0, rows.shape[0], chunk)])


def least_h5_norm(state, features):
    """The smallest |h5| over the rows, in float64: how far the case is from the 0 / 0 of a zero row."""
    m = encoder_from(state, torch.float64)
    x = rows_of(features).double()
    with torch.no_grad():
        for layer in m.encoder:
            x = layer(x)
    return float(x.norm(dim=-1).min())


# ---- the golden cases ------------------------------------------------------------------------------------------------------
# key -> (shape of the input, seed): 70 rows, and a 9 x 13 channel-major map
GOLDEN_CASES = OrderedDict([("rows70", ((70, 768), 0)), ("map9x13", ((768, 9, 13), 1))])


def make_case(key):
    """-> (encoder state, features in the case's shape)."""
    shape, seed = GOLDEN_CASES[key]
    state = encoder_state(200 + seed)
    if len(shape) == 2:
        return state, make_features(shape[0], seed)
    _, h, w = shape
    return state, make_features(h * w, seed).t().contiguous().view(WIDTHS[0], h, w)
