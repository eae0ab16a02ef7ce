"""Generates tests/golden/map_edit.npz: the reference's OWN GaussianModel (gaussian_splatting/scene/gaussian_model.py) driven
through the back end's map edits on the CPU, for the case of tests/map_edit_case.py: Adam steps, densification statistics,
densify_and_prune with the mapping arguments, the skipped step of that iteration, reset_opacity_nonvisible (the opacity group
skips its step), prune_points, extend_from_pcd, one init-mode densify_and_prune.  Runs ONLY in the authoring container
(needs the reference checkout); the committed .npz is data: per stage a digest of every array of the map (parameters, both
Adam moments in bucket layout, per-group step counts, kfIDs, n_obs, accumulators), and the full arrays after the first
densify_and_prune.

The module imports with open3d, plyfile and simple_knn._C stubbed, the hard-coded device="cuda" of torch.zeros / empty / full /
ones remapped to the CPU, and torch.normal replaced by std * z from the case's recorded z (child k of source row j: z[j, k])."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OLSR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
import map_edit_case as case  # noqa: E402

for name in ("open3d", "plyfile", "simple_knn", "simple_knn._C"):
    m = types.ModuleType(name)
    sys.modules[name] = m
sys.modules["plyfile"].PlyData = sys.modules["plyfile"].PlyElement = object
sys.modules["simple_knn._C"].distCUDA2 = None
sys.modules["simple_knn"]._C = sys.modules["simple_knn._C"]


def _cpu(fn):
    def wrapped(*a, **k):
        if k.get("device") == "cuda":
            k["device"] = "cpu"
        return fn(*a, **k)
    return wrapped


for fname in ("zeros", "empty", "full", "ones"):
    setattr(torch, fname, _cpu(getattr(torch, fname)))

from gaussian_splatting.scene.gaussian_model import GaussianModel  # noqa: E402
from torch import nn  # noqa: E402

_Z = {}


def _normal(mean=None, std=None, *a, **k):
    zz = _Z["zz"]
    assert tuple(zz.shape) == tuple(std.shape), (zz.shape, std.shape)
    return std * zz


torch.normal = _normal


class Args:
    percent_dense = case.PERCENT_DENSE
    position_lr_init = case.LRS["xyz"]
    position_lr_final = 1.6e-6
    position_lr_delay_mult = 0.01
    position_lr_max_steps = 30000
    feature_lr = case.LRS["f_dc"]
    opacity_lr = case.LRS["opacity"]
    scaling_lr = case.LRS["scaling"]
    rotation_lr = case.LRS["rotation"]
    language_lr = case.LRS["f_language"]


def build():
    g = torch.Generator().manual_seed(case.SEED - 1)
    init = case.initial_map(g)
    gm = GaussianModel(0, config={"language": {"language_train": True, "lang_code_size": case.F}})
    gm.spatial_lr_scale = 1.0
    gm._xyz = nn.Parameter(init["xyz"].clone().requires_grad_(True))
    gm._features_dc = nn.Parameter(init["f_dc"].clone().requires_grad_(True))
    gm._features_rest = nn.Parameter(init["f_rest"].clone().requires_grad_(True))
    gm._opacity = nn.Parameter(init["opacity"].clone().requires_grad_(True))
    gm._scaling = nn.Parameter(init["scaling"].clone().requires_grad_(True))
    gm._rotation = nn.Parameter(init["rotation"].clone().requires_grad_(True))
    gm.training_setup(Args())
    # language starts at zero (training_setup); lr of f_rest is feature_lr / 20 as in the case
    gm.unique_kfIDs = init["kf_id"].clone()
    gm.n_obs = init["n_obs"].clone()
    gm.max_radii2D = torch.zeros(init["xyz"].shape[0])
    return gm


class Model:
    def __init__(self, gm):
        self.gm = gm

    @property
    def P(self):
        return self.gm.get_xyz.shape[0]


def params_of(gm):
    return dict(xyz=gm._xyz, f_dc=gm._features_dc, f_rest=gm._features_rest, opacity=gm._opacity, scaling=gm._scaling,
                rotation=gm._rotation, f_language=gm._language_feature)


def export(gm):
    P = gm.get_xyz.shape[0]
    p = params_of(gm)

    def moment(key):
        cols = []
        for n in case.GROUPS:
            st = gm.optimizer.state.get(p[n], None)
            cols.append(st[key].reshape(P, -1) if st is not None else torch.zeros_like(p[n]).reshape(P, -1))
        return torch.cat(cols, dim=1)
    steps = []
    for n in case.GROUPS:
        st = gm.optimizer.state.get(p[n], None)
        steps.append(int(st["step"]) if st is not None else 0)
    return dict(means3D=p["xyz"].detach(), shs=torch.cat([p["f_dc"], p["f_rest"]], dim=1).detach(),
                opacities=p["opacity"].detach().reshape(P, 1), scales=p["scaling"].detach(), rotations=p["rotation"].detach(),
                language=p["f_language"].detach(), exp_avg=moment("exp_avg"), exp_avg_sq=moment("exp_avg_sq"),
                kf_id=gm.unique_kfIDs.int(), n_obs=gm.n_obs.int(),
                stats=torch.cat([gm.xyz_gradient_accum, gm.denom], dim=1), max_radii=gm.max_radii2D.float(),
                group_steps=torch.tensor(steps, dtype=torch.int64))


def _margin(x, thr, what, rel=1e-3):
    x = x.double()
    near = (x - thr).abs() <= rel * abs(thr)
    assert not bool(near.any()), f"{what}: {int(near.sum())} value(s) within {rel} relative of {thr}"


class Ops:
    def step(self, m, grads, skip):
        gm = m.gm
        p = params_of(gm)
        for n in case.GROUPS:
            p[n].grad = None if (skip == "all" or n in skip) else grads[n].clone()
        gm.optimizer.step()
        gm.optimizer.zero_grad(set_to_none=True)

    def stats(self, m, views):
        gm = m.gm
        for grad, vis, radii in views:   # slam_backend.py:716-727
            gm.max_radii2D[vis] = torch.max(gm.max_radii2D[vis], radii[vis].float())
            vt = types.SimpleNamespace(grad=grad)
            gm.add_densification_stats(vt, vis)

    def densify(self, m, args, z):
        gm = m.gm
        max_grad, min_opacity, extent, max_screen_size = args
        grads = gm.xyz_gradient_accum / gm.denom
        grads[grads.isnan()] = 0.0
        smax = gm.get_scaling.max(dim=1).values
        _margin(grads.squeeze(1), max_grad, "gradient")
        _margin(smax, gm.percent_dense * extent, "clone / split scale")
        _margin(gm.get_opacity.squeeze(1), min_opacity, "opacity")
        if max_screen_size:
            _margin(smax, 0.1 * extent, "world-space size")
            _margin(smax / 1.6, 0.1 * extent, "world-space size of split children")
        sel = (grads.squeeze(1) >= max_grad) & (smax > gm.percent_dense * extent)   # the split's selection (originals)
        idx = torch.nonzero(sel).reshape(-1)
        _Z["zz"] = torch.cat([z[idx, k] for k in range(2)], dim=0)
        gm.densify_and_prune(max_grad, min_opacity, extent, max_screen_size)
        counts = dict(selected_split=int(sel.sum()), clone=int(((grads.squeeze(1) >= max_grad) & ~sel).sum()))
        return counts

    def reset_nonvisible(self, m, filters):
        m.gm.reset_opacity_nonvisible(filters)

    def prune(self, m, mask):
        m.gm.prune_points(mask)

    def extend(self, m, rows, kf_id):
        r = rows
        feats = torch.cat([r["f_dc"], r["f_rest"]], dim=1).transpose(1, 2).contiguous()   # [n, 3, (D+1)^2], as create_pcd_from_image
        m.gm.extend_from_pcd(r["xyz"].clone(), feats, None, r["scaling"].clone(), r["rotation"].clone(),
                             r["opacity"].clone(), kf_id)


def main():
    gm = build()
    m = Model(gm)
    rec, full = {}, {}

    def record(stage, model):
        st = export(model.gm)
        rec[stage] = case.digests(st)
        if stage == "densify":
            for k, v in st.items():
                full[f"densify_{k}"] = v.detach().cpu().clone().numpy()
        print(f"{stage:18s} P={model.P} steps={st['group_steps'].tolist()}")
    case.run(m, Ops(), record)
    out = os.path.join(HERE, "map_edit.npz")
    np.savez_compressed(out, digests=np.array(case.dumps(rec)), stages=np.array(list(case.STAGES)), **full)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
