"""Torch restatement of the online language autoencoder and of one call of the reference's train_online_autoencoder
(utils/slam_backend.py:266-323 on language/autoencoder/model.py:314-354), dtype-generic: the yardstick of
tests/test_gpu_lang_codec.py at the sizes too large to commit, and the source of every per-row truth (codes).

    encode(x) = z / |z|, z = Linear(24,15)(relu(Linear(32,24)(x)));  decode(c) = y / |y|, y = Linear(24,32)(relu(Linear(15,24)(c)))
    loss = l1_loss(r, x) + 0.6 (1 - cosine_similarity(r, x, dim=1).mean()),  r = decode(encode(x))
    zero_grad, backward, torch.optim.Adam(lr).step()

tests/test_lang_codec_ref_golden.py pins this module to arrays recorded from the reference's own module
(tests/golden/make_golden_lang_codec.py -> lang_codec.npz).  Runs on the CPU.

Features.  Unit-norm float32 rows of a rank-6 mixture plus 10 % noise (the real features are unit-norm outputs of the
32-channel autoencoder's encode).  They are kept as int16 q with x = unit(q / 2^15): unit() is written with elementwise
float32 operations only (a column-by-column sum, sqrt, divide), which IEEE arithmetic makes the same bits everywhere, so the
recorded results belong to exactly the features a test rebuilds.

Tie rows.  A ReLU pre-activation or a residual r - x that rounds to the other side of zero in float32 flips one row's
contribution, which moves a mean gradient by ~1e-6, hundreds of times the float32 error of everything else.  The single-step
cases therefore redraw every row whose float64 |a1|, |a2| or |r - x| has an element below TAU on the case's parameters
(`redraw_ties`; at most 1 % of the rows, asserted)."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

STATE = (("encoder.0.weight", (24, 32)), ("encoder.0.bias", (24,)), ("encoder.2.weight", (15, 24)), ("encoder.2.bias", (15,)),
         ("decoder.0.weight", (24, 15)), ("decoder.0.bias", (24,)), ("decoder.2.weight", (32, 24)), ("decoder.2.bias", (32,)))
N_PARAMS = 2351
TAU = 1e-5
GOLDEN_NS, GOLDEN_SEEDS = (1000, 257), (0, 1, 2, 3)
CODE_ROW_STRIDE = 64   # the golden file keeps the codes of every 64th row


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lang_codec.npz"))


def golden_cases():
    """[(key prefix, N, seed)] in the file's order."""
    return [(f"n{N}_s{seed}", N, seed) for N in GOLDEN_NS for seed in GOLDEN_SEEDS]


class Codec(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = nn.Sequential(nn.Linear(32, 24), nn.ReLU(), nn.Linear(24, 15))
        self.decoder = nn.Sequential(nn.Linear(15, 24), nn.ReLU(), nn.Linear(24, 32))

    def encode(self, x):
        z = self.encoder(x)
        return z / z.norm(dim=-1, keepdim=True)

    def decode(self, c):
        y = self.decoder(c)
        return y / y.norm(dim=-1, keepdim=True)


def flatten(state):
    """state_dict (or named tensors) -> flat [2351] in state_dict order."""
    return torch.cat([state[k].detach().reshape(-1) for k, _ in STATE])


def unflatten(flat):
    out, off = OrderedDict(), 0
    for k, shape in STATE:
        n = int(np.prod(shape))
        out[k] = flat[off:off + n].reshape(shape)
        off += n
    assert off == N_PARAMS
    return out


def initial_params(seed):
    """nn.Linear's default initialisation under torch.manual_seed(seed): flat float32 [2351]."""
    torch.manual_seed(seed)
    return flatten(Codec().state_dict()).clone()


def codec_from(flat, dtype):
    m = Codec().to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in unflatten(torch.as_tensor(flat)).items()})
    return m


def unit(q):
    """int16 [N,32] -> float32 unit-norm rows, elementwise float32 operations only."""
    x = torch.from_numpy(np.asarray(q).astype(np.float32)) / 32768.0
    s = torch.zeros(x.shape[0], dtype=torch.float32)
    for k in range(x.shape[1]):
        s = s + x[:, k] * x[:, k]
    return x / torch.sqrt(s).unsqueeze(1)


def draw_q(n, generator):
    """n rows of the rank-6 mixture + 10 % noise, as int16."""
    basis = torch.randn(6, 32, generator=generator, dtype=torch.float64)
    basis = basis / basis.norm(dim=1, keepdim=True)
    coef = torch.randn(n, 6, generator=generator, dtype=torch.float64)
    x = coef @ basis
    x = x / x.norm(dim=1, keepdim=True)
    x = x + 0.1 * torch.randn(n, 32, generator=generator, dtype=torch.float64) / 32 ** 0.5   # |noise| ~ 0.1 |signal|
    x = x / x.norm(dim=1, keepdim=True)
    return torch.round(x * 32767.0).to(torch.int16).numpy()


def tie_rows(flat, x):
    """bool [N]: rows whose float64 |a1|, |a2| or |r - x| has an element below TAU on these parameters."""
    m = codec_from(flat, torch.float64)
    xd = x.double()
    with torch.no_grad():
        a1 = m.encoder[0](xd)
        c = m.encode(xd)
        a2 = m.decoder[0](c)
        r = m.decode(c)
    small = lambda t: (t.abs() < TAU).any(dim=1)  # noqa: E731
    return small(a1) | small(a2) | small(r - xd)


def redraw_ties(flat, q, generator):
    """Redraws tie rows of q (in place) until none is left.  -> rows redrawn in all."""
    n = 0
    for _ in range(20):
        bad = tie_rows(flat, unit(q)).numpy()
        k = int(bad.sum())
        if k == 0:
            assert n <= 0.01 * q.shape[0], (n, q.shape[0])
            return n
        n += k
        q[bad] = draw_q(k, generator)[:k]
    raise AssertionError("tie rows remain after 20 redraws")


def make_case(N, seed):
    """-> (flat parameters float32 [2351], q int16 [N,32], rows redrawn); features = unit(q).
    The features' generator is seeded N + seed.  (A first choice, 1000 + seed, redrew 3 of 257 rows for seed 0: 1.2 %, which
    the 1 % condition rejects; with N + seed the eight golden cases redraw 0 - 6 rows and N = 36 864 / 36 865 redraw 92 - 146.)"""
    flat = initial_params(seed)
    g = torch.Generator().manual_seed(N + seed)
    q = draw_q(N, g)
    n = redraw_ties(flat, q, g)
    return flat, q, n


def loss_terms(model, x):
    """The statements of the reference's step up to the loss.  -> (codes, [total, L1, 0.6 (1 - cos), mean cos])."""
    codes = model.encode(x)
    recon = model.decode(codes)
    l1 = F.l1_loss(recon, x)
    cos = F.cosine_similarity(recon, x, dim=1).mean()
    cos_term = 0.6 * (1 - cos)
    return codes, [l1 + cos_term, l1, cos_term, cos]


def train(flat, x, lr, steps, dtype, model=None):
    """`steps` calls of train_online_autoencoder on the same features, evaluated in `dtype`.
    -> dict(loss [steps,4], grad0 [2351] (the first step's gradient), codes_pre0, codes_post0 (before / after the first update),
            params [2351], codes_post (re-encoded after the last update)); `model`: any module with the Codec's interface."""
    m = model if model is not None else codec_from(flat, dtype)
    x = x.detach().to(dtype)
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    out = dict(loss=[])
    for i in range(steps):
        m.train()
        opt.zero_grad()
        codes, terms = loss_terms(m, x)
        terms[0].backward()
        if i == 0:
            out["grad0"] = flatten({k: p.grad for k, p in m.named_parameters()}).clone()
            out["codes_pre0"] = codes.detach().clone()
        opt.step()
        out["loss"].append(torch.stack([t.detach() for t in terms]))
        if i == 0 or i == steps - 1:
            with torch.no_grad():
                m.eval()
                post = m.encode(x).clone()
            if i == 0:
                out["codes_post0"] = post
            out["codes_post"] = post
    out["loss"] = torch.stack(out["loss"])
    out["params"] = flatten(m.state_dict()).clone()
    return out
