"""The map-edit case of tests/golden/map_edit.npz: a ~600-Gaussian language map (sh_degree 0, F = 15) and the sequence of
back-end operations it goes through.  Every input is drawn from one seeded CPU generator in a fixed order, so the fixture's
generator (which drives the reference's GaussianModel) and the tests (which drive online_lang_splatting_amd.gaussian_map)
see the same bits.  Values are built in bands so that no mask decision lies near a threshold (margins are asserted by the
generator).

`run(model, ops)` plays the sequence on any object with the reference's method names; `ops` adapts the few calls whose
form differs (the optimiser step, the split's noise)."""
import hashlib
import json

import numpy as np
import torch

P0, F, N_NEW, SEED = 600, 15, 40, 20261016
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "f_language")
LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20.0, opacity=0.05, scaling=1e-3, rotation=1e-3, f_language=2.5e-3)
PERCENT_DENSE = 0.01
DENSIFY_ARGS = (2e-4, 0.7, 1.0, 20)          # slam_backend.py:730-741 (densify_grad_threshold, gaussian_th, extent, size)
INIT_DENSIFY_ARGS = (2e-4, 0.005, 1.0, None)  # slam_backend.py:429-436 (init mode: no screen-size argument)


def _bands(g, n, bands):
    """n values, each from one of the (lo, hi) bands chosen uniformly, log-uniform inside the band."""
    pick = torch.randint(0, len(bands), (n,), generator=g)
    lo = torch.tensor([b[0] for b in bands], dtype=torch.float64)[pick]
    hi = torch.tensor([b[1] for b in bands], dtype=torch.float64)[pick]
    u = torch.rand(n, generator=g, dtype=torch.float64)
    return torch.exp(torch.log(lo) + u * (torch.log(hi) - torch.log(lo)))


def initial_map(g):
    P = P0
    xyz = torch.randn(P, 3, generator=g) * 2.0
    f_dc = torch.randn(P, 1, 3, generator=g) * 0.5
    f_rest = torch.zeros(P, 0, 3)
    # opacity logits: below sigmoid^-1(0.7) = 0.847 by >= 0.5, or above by >= 0.7
    op = torch.where(torch.rand(P, generator=g) < 0.15, -2.0 + 1.6 * torch.rand(P, generator=g),
                     1.6 + 2.4 * torch.rand(P, generator=g)).reshape(P, 1)
    # max(exp(scaling)) on axis 0, in a clone band, a split band or a big band (children of the big band stay clear of 0.1)
    smax = _bands(g, P, [(0.003, 0.009), (0.012, 0.08), (0.12, 0.15), (0.17, 0.3)])
    ratio = torch.cat([torch.ones(P, 1, dtype=torch.float64), 0.3 + 0.7 * torch.rand(P, 2, generator=g, dtype=torch.float64)], 1)
    scaling = torch.log(smax.view(P, 1) * ratio).float()
    rotation = torch.randn(P, 4, generator=g)
    language = torch.zeros(P, F)
    kf_id = torch.randint(0, 6, (P,), generator=g).int()
    n_obs = torch.randint(0, 5, (P,), generator=g).int()
    return dict(xyz=xyz, f_dc=f_dc, f_rest=f_rest, opacity=op, scaling=scaling, rotation=rotation, f_language=language,
                kf_id=kf_id, n_obs=n_obs)


def adam_grads(g, P):
    lang = torch.randn(P, F, generator=g) * 1e-3
    lang[torch.rand(P, generator=g) < 0.75] = 0.0   # most rows see no language gradient (and compress)
    return dict(xyz=torch.randn(P, 3, generator=g) * 1e-3, f_dc=torch.randn(P, 1, 3, generator=g) * 1e-3,
                f_rest=torch.zeros(P, 0, 3), opacity=torch.randn(P, 1, generator=g) * 1e-2,
                scaling=torch.randn(P, 3, generator=g) * 1e-3, rotation=torch.randn(P, 4, generator=g) * 1e-3,
                f_language=lang)


def view_stats(g, P, nviews=3):
    """Per view: (means2D.grad [P,3], visibility [P] bool, radii [P] int32).  The gradient norm of a row is a per-row level
    (far below or far above 2e-4) jittered by +-20 % per view; a fifth of the rows is visible in no view (0/0)."""
    level = _bands(g, P, [(1e-5, 1e-4), (3.5e-4, 2e-3)]).float()
    never = torch.rand(P, generator=g) < 0.2
    out = []
    for _ in range(nviews):
        vis = (torch.rand(P, generator=g) < 0.7) & ~never
        d = torch.randn(P, 2, generator=g)
        d = d / d.norm(dim=-1, keepdim=True)
        mag = level * (0.8 + 0.4 * torch.rand(P, generator=g))
        grad = torch.cat([d * mag.view(P, 1), torch.randn(P, 1, generator=g)], dim=1)
        radii = torch.where(vis, torch.randint(1, 30, (P,), generator=g, dtype=torch.int32), torch.zeros(P, dtype=torch.int32))
        out.append((grad, vis, radii))
    return out


def new_rows(g, n=N_NEW):
    smax = _bands(g, n, [(0.003, 0.009), (0.012, 0.08)])
    return dict(xyz=torch.randn(n, 3, generator=g) * 2.0, f_dc=torch.randn(n, 1, 3, generator=g) * 0.5,
                f_rest=torch.zeros(n, 0, 3), opacity=(1.6 + 2.4 * torch.rand(n, 1, generator=g)),
                scaling=torch.log(smax.view(n, 1) * torch.ones(n, 3, dtype=torch.float64)).float(),
                rotation=torch.randn(n, 4, generator=g))


STAGES = ("adam1", "stats1", "densify", "skipped_step", "adam2", "reset_nonvisible", "prune", "extend", "adam3", "stats2",
          "densify_init")


def run(model, ops, record):
    """Plays the sequence.  ops: step(model, grads, skip) / stats(model, views) / densify(model, args, z) /
    reset_nonvisible(model, filters) / prune(model, mask) / extend(model, rows, kf_id).  record(stage, model) after each
    stage."""
    g = torch.Generator().manual_seed(SEED)
    P = model.P
    for _ in range(3):
        ops.step(model, adam_grads(g, P), ())
    record("adam1", model)
    ops.stats(model, view_stats(g, P))
    record("stats1", model)
    z = torch.randn(P, 2, 3, generator=g)
    ops.densify(model, DENSIFY_ARGS, z)
    record("densify", model)
    P = model.P
    ops.step(model, adam_grads(g, P), "all")           # the iteration of the edit: every parameter replaced, no step
    record("skipped_step", model)
    for _ in range(2):
        ops.step(model, adam_grads(g, P), ())
    record("adam2", model)
    filters = [torch.rand(P, generator=g) < 0.5 for _ in range(2)]
    ops.reset_nonvisible(model, filters)
    ops.step(model, adam_grads(g, P), ("opacity",))    # the opacity parameter was replaced in this iteration
    record("reset_nonvisible", model)
    mask = torch.rand(P, generator=g) < 0.1
    ops.prune(model, mask)
    record("prune", model)
    ops.extend(model, new_rows(g), 7)
    record("extend", model)
    P = model.P
    ops.step(model, adam_grads(g, P), ())               # the next iteration's gradients
    record("adam3", model)
    ops.stats(model, view_stats(g, P))
    record("stats2", model)
    z = torch.randn(P, 2, 3, generator=g)
    ops.densify(model, INIT_DENSIFY_ARGS, z)
    record("densify_init", model)


def digest(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return f"{a.dtype.str}:{'x'.join(map(str, a.shape))}:" + hashlib.sha256(a.tobytes()).hexdigest()[:24]


def digests(state):
    return {k: digest(v) for k, v in state.items()}


def dumps(d):
    return json.dumps(d, sort_keys=True)
