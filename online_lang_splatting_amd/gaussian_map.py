"""The Gaussian map of the back end, with its optimiser state, edited on the device.

The reference's back end changes the number of Gaussians P all the time — a keyframe's new Gaussians
(`extend_from_pcd`), periodic `densify_and_prune` (clone, split, prune), the co-visibility `prune_points` of a full window —
and resets opacities (`reset_opacity`, `reset_opacity_nonvisible`); gaussian_splatting/scene/gaussian_model.py:283-961,
utils/slam_backend.py:418-445, 683-752.  Every such edit rebuilds the parameters AND the Adam moments
(`_prune_optimizer`, `cat_tensors_to_optimizer`, `replace_tensor_to_optimizer`).

`GaussianMap` owns the same state in the fused path's layout — parameter arrays, the `FusedAdam` moments in bucket layout
[P, 11 + 3M + F] with per-group step counts, the densification accumulators [P, 2] = {xyz_gradient_accum, denom} and
max_radii, kfID and n_obs — with spare capacity, and edits it with one primitive of the library (olsr_map_edit_plan /
olsr_map_edit_apply, include/olsr.h; csrc/k_map_edit.hip): out of place into a second set of buffers, ONE host read per
edit (the new P, to size the destination), the reference's row order and optimiser-state surgery.  Each edit returns
`src_index` (int32 [P_new]: the source row of every new row, -(k + 1) for appended row k) so that a caller can remap side
arrays of its own.

`MapSpec` is the torch specification of the same operations: the reference's own expressions on a `torch.optim.Adam`,
with the row bookkeeping added.  It runs on CPU or GPU and is used only as the reference of the tests (the precedent of
GradientBucket.capped_torch_formulation); tests/golden/map_edit.npz pins it to the reference's GaussianModel.
"""
import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from . import _abi
from ._host import ptr, stream_ptr
from ._lib import check, lib
from .frame_shard import FusedAdam, GradLayout

GROUPS = _abi.ADAM_GROUPS   # xyz, f_dc, f_rest, opacity, scaling, rotation, f_language


def opacity_logit(value: float) -> torch.Tensor:
    """The raw opacity whose sigmoid is `value`: logit(v) = log(v / (1 - v)), evaluated in fp32 on the CPU (the reset
    constants of reset_opacity / reset_opacity_nonvisible, gaussian_model.py:565-583).  [1, 1]."""
    v = torch.full((1, 1), value, dtype=torch.float32)
    return torch.log(v / (1 - v))


def quaternion_matrices(q: torch.Tensor) -> torch.Tensor:
    """[n, 4] quaternions (w, x, y, z; not necessarily unit) -> [n, 3, 3] rotation matrices of the normalised quaternions.
    Evaluated term by term in the order the reference's general_utils.build_rotation (:113-135) rounds them: the norm as
    ((w w + x x) + y y) + z z, every entry as 2 (a +- b) or 1 - 2 (a + b)."""
    w0, x0, y0, z0 = q.unbind(dim=1)
    n = torch.sqrt(w0 * w0 + x0 * x0 + y0 * y0 + z0 * z0).unsqueeze(1)
    w, x, y, z = (q / n).unbind(dim=1)
    entries = (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
               2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
               2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))
    return torch.stack(entries, dim=1).view(-1, 3, 3)


def covisibility_mask(n_obs, kf_id, window: Sequence[int], mode: str):
    """utils/slam_backend.py:683-716: "slam" prunes n_obs <= 3 among the Gaussians of the window's newer keyframes
    (kfID >= the third newest), "odometry" prunes n_obs < 3."""
    if mode == "odometry":
        return n_obs < 3
    if mode == "slam":
        return (n_obs <= 3) & (kf_id >= sorted(window, reverse=True)[2])
    raise ValueError(f"prune mode {mode!r}: 'slam' or 'odometry'")


# ------------------------------------------------------------------------------------------------------------------------
class MapSpec:
    """The torch specification of GaussianMap, written as the map as a whole: per parameter group a tensor shaped like the
    reference's (xyz [P,3], f_dc [P,1,3], f_rest [P,M-1,3], opacity [P,1], scaling [P,3], rotation [P,4], f_language [P,F]),
    its two Adam moments and its step count; the accumulators; kfID and n_obs.  Every topology edit is ONE gather: the row
    index of the new map into [old rows | new rows], with the moments of new rows zero; the split children's positions and
    scales are the only computed rows.  Adam is torch.optim.Adam(lr=0, eps=1e-15) itself, bound to this state for each step;
    a group skips a step by having no gradient, exactly as the reference's groups do after their parameter was replaced.
    The result equals the reference's GaussianModel bit for bit (tests/golden/map_edit.npz).  `src` after an edit: the source
    row of every row (-(k + 1) for appended row k).  CPU or GPU: the tensors' device."""

    def __init__(self, xyz, f_dc, f_rest, opacity, scaling, rotation, language, lrs: Dict[str, float], kf_id=None,
                 n_obs=None, percent_dense=0.01):
        P = xyz.shape[0]
        dev = xyz.device
        given = (xyz, f_dc, f_rest, opacity, scaling, rotation, language)
        self.t = {n: v.detach().to(torch.float32).clone().contiguous() for n, v in zip(GROUPS, given)}
        self.m = {n: torch.zeros_like(v) for n, v in self.t.items()}
        self.v = {n: torch.zeros_like(v) for n, v in self.t.items()}
        self.steps = {n: 0 for n in GROUPS}
        self.lrs = dict(lrs)
        self.kf_id = kf_id.to(dev).int().clone() if kf_id is not None else torch.zeros(P, dtype=torch.int32, device=dev)
        self.n_obs = n_obs.to(dev).int().clone() if n_obs is not None else torch.zeros(P, dtype=torch.int32, device=dev)
        self.accum = torch.zeros(P, 1, device=dev)
        self.denom = torch.zeros(P, 1, device=dev)
        self.max_radii = torch.zeros(P, device=dev)
        self.percent_dense = percent_dense
        self.src = torch.arange(P, device=dev)

    @classmethod
    def from_state(cls, st: Dict[str, torch.Tensor], lrs: Dict[str, float], device, percent_dense=0.01):
        """A specification holding `st` (the layout of export() / GaussianMap.state())."""
        f = lambda t: t.to(device=device, dtype=torch.float32)  # noqa: E731
        P, M = st["means3D"].shape[0], st["shs"].shape[1]
        shs = f(st["shs"])
        spec = cls(f(st["means3D"]), shs[:, :1] if M else torch.zeros(P, 0, 3, device=device), shs[:, 1:],
                   f(st["opacities"]).reshape(P, 1), f(st["scales"]), f(st["rotations"]), f(st["language"]), lrs,
                   kf_id=st["kf_id"].to(device), n_obs=st["n_obs"].to(device), percent_dense=percent_dense)
        c = 0
        for gi, n in enumerate(GROUPS):
            w = int(torch.tensor(spec.t[n].shape[1:]).prod())
            spec.m[n] = f(st["exp_avg"][:, c:c + w]).reshape(spec.t[n].shape).clone()
            spec.v[n] = f(st["exp_avg_sq"][:, c:c + w]).reshape(spec.t[n].shape).clone()
            spec.steps[n] = int(st["group_steps"][gi])
            c += w
        spec.accum = f(st["stats"][:, 0:1]).clone()
        spec.denom = f(st["stats"][:, 1:2]).clone()
        spec.max_radii = f(st["max_radii"]).clone()
        return spec

    @property
    def P(self):
        return self.t["xyz"].shape[0]

    def _device(self):
        return self.t["xyz"].device

    # ---- optimiser ----
    def step(self, grads: Dict[str, torch.Tensor], skip=()):
        """One torch.optim.Adam step over the groups with `grads` (group name -> gradient); groups in `skip` ("all": every
        group) have no gradient and do not step."""
        skip = set(GROUPS) if skip == "all" else set(skip)
        params, groups = {}, []
        for n in GROUPS:
            p = torch.nn.Parameter(self.t[n])
            if n not in skip:
                p.grad = grads[n].detach().to(self.t[n]).reshape(self.t[n].shape).clone()
            params[n] = p
            groups.append({"params": [p], "lr": self.lrs[n]})
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15, foreach=False)
        for n, p in params.items():
            opt.state[p] = {"step": torch.tensor(float(self.steps[n])), "exp_avg": self.m[n], "exp_avg_sq": self.v[n]}
        opt.step()
        for n, p in params.items():
            self.t[n] = p.detach()
            if n not in skip:
                self.steps[n] += 1

    def group_steps(self):
        return [self.steps[n] for n in GROUPS]

    # ---- the one edit: a gather into [old rows | new rows] ----
    def _rebuild(self, index, new=None, new_meta=None, zero_accumulators=False):
        """The map after an edit: row i of the result is row index[i] of [old rows | `new` rows] (new: group name -> rows,
        new_meta: (kf_id, n_obs, src) of the new rows).  Moments of new rows start at zero; the accumulators follow the rows
        or, zero_accumulators, are zero for every row (the reference's densification postfix)."""
        P = self.P
        dev = self._device()
        nn_ = 0 if new is None else new["xyz"].shape[0]

        def gather(old, extra):
            full = old if not nn_ else torch.cat([old, extra.to(old)], dim=0)
            return full.index_select(0, index)
        for n in GROUPS:
            zeros = None if not nn_ else torch.zeros((nn_,) + tuple(self.t[n].shape[1:]), device=dev)
            self.t[n] = gather(self.t[n], None if not nn_ else new[n])
            self.m[n] = gather(self.m[n], zeros)
            self.v[n] = gather(self.v[n], zeros)
        kf, no, src = new_meta if nn_ else (None, None, None)
        self.kf_id = gather(self.kf_id, kf)
        self.n_obs = gather(self.n_obs, no)
        self.src = gather(torch.arange(P, device=dev), src)
        if zero_accumulators:
            Pn = index.numel()
            self.accum, self.denom, self.max_radii = (torch.zeros(Pn, 1, device=dev), torch.zeros(Pn, 1, device=dev),
                                                      torch.zeros(Pn, device=dev))
        else:
            self.accum, self.denom = self.accum.index_select(0, index), self.denom.index_select(0, index)
            self.max_radii = self.max_radii.index_select(0, index)
        return self.src.int()

    # ---- edits ----
    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, z):
        """Clone (gradient >= max_grad, max(exp(scaling)) <= percent_dense extent), split into two children (gradient >=
        max_grad and larger; child k of row j: xyz + R(q) (exp(scaling) z[j, k]), scaling log(exp(scaling) / 1.6)), then drop
        the rows of [kept originals | clones | children 0 | children 1] whose sigmoid(opacity) < min_opacity or — when
        max_screen_size is truthy — max(exp(scaling)) > 0.1 extent.  The reference's max_radii2D > max_screen_size term never
        fires (its densification postfix has zeroed max_radii2D), so it is absent.  Accumulators end zero.  Returns src."""
        P, dev = self.P, self._device()
        t = self.t
        g = self.accum / self.denom
        g = torch.where(torch.isnan(g), torch.zeros_like(g), g)[:, 0]
        big_row = torch.exp(t["scaling"]).amax(dim=1) > self.percent_dense * extent
        clone = (g.abs() >= max_grad) & ~big_row
        split = (g >= max_grad) & big_row
        ci = torch.nonzero(clone).flatten()
        si = torch.nonzero(split).flatten()
        S = si.numel()
        # the split's rows see the map that already holds the clones: exp(scaling) of [rows | clones]
        scale_ext = torch.exp(torch.cat([t["scaling"], t["scaling"].index_select(0, ci)], dim=0))
        std = scale_ext.index_select(0, si).repeat(2, 1)                                    # [2S, 3], k-major
        noise = torch.cat([z[si, 0], z[si, 1]], dim=0).to(std)
        offset = torch.bmm(quaternion_matrices(t["rotation"].index_select(0, si)).repeat(2, 1, 1),
                           (std * noise).unsqueeze(-1)).squeeze(-1)
        child = dict((n, t[n].index_select(0, si).repeat((2,) + (1,) * (t[n].dim() - 1))) for n in GROUPS)
        child["xyz"] = offset + child["xyz"]
        child["scaling"] = torch.log(std / 1.6)
        # new rows: the clones (raw copies) then the children; both start with zero moments
        new = {n: torch.cat([t[n].index_select(0, ci), child[n]], dim=0) for n in GROUPS}
        src_new = torch.cat([ci, si.repeat(2)])
        meta = (self.kf_id.index_select(0, src_new), self.n_obs.index_select(0, src_new), src_new)
        index = torch.cat([torch.nonzero(~split).flatten(), P + torch.arange(ci.numel() + 2 * S, device=dev)])
        # candidates -> survivors: one more gather of the same rows
        cand_op = torch.cat([t["opacity"], new["opacity"]], dim=0).index_select(0, index)
        cand_sc = torch.cat([t["scaling"], new["scaling"]], dim=0).index_select(0, index)
        drop = (torch.sigmoid(cand_op) < min_opacity).flatten()
        if max_screen_size:
            drop = drop | (torch.exp(cand_sc).amax(dim=1) > 0.1 * extent)
        index = index[~drop]
        return self._rebuild(index, new, meta, zero_accumulators=True)

    def prune(self, mask):
        """Drop the rows where mask is True; moments and accumulators follow the kept rows.  Returns src."""
        return self._rebuild(torch.nonzero(~mask.to(self._device()).bool().flatten()).flatten())

    prune_points = prune

    def extend(self, xyz, f_dc, f_rest, opacity, scaling, rotation, kf_id):
        """Append ready rows: language zero, kfID = kf_id, n_obs 0, zero moments; every accumulator zeroed.  Returns src."""
        n, dev, P = xyz.shape[0], self._device(), self.P
        rows = dict(xyz=xyz, f_dc=f_dc, f_rest=f_rest, opacity=opacity, scaling=scaling, rotation=rotation,
                    f_language=torch.zeros(n, self.t["f_language"].shape[1], device=dev))
        meta = (torch.full((n,), int(kf_id), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                -1 - torch.arange(n, device=dev))
        return self._rebuild(torch.arange(P + n, device=dev), rows, meta, zero_accumulators=True)

    def _reset_opacity_to(self, value, keep=None):
        c = opacity_logit(value).to(self._device()).expand_as(self.t["opacity"])
        self.t["opacity"] = c.clone() if keep is None else torch.where(keep.view(-1, 1), self.t["opacity"], c)
        self.m["opacity"] = torch.zeros_like(self.t["opacity"])
        self.v["opacity"] = torch.zeros_like(self.t["opacity"])

    def reset_opacity(self):
        """Opacity sigmoid^-1(0.01) everywhere, opacity moments zero (the opacity group then skips its step)."""
        self._reset_opacity_to(0.01)

    def reset_opacity_nonvisible(self, visibility_filters):
        """Opacity sigmoid^-1(0.4) where no filter is set, opacity moments zero."""
        keep = torch.zeros(self.P, dtype=torch.bool, device=self._device())
        for f in visibility_filters:
            keep |= f.to(keep.device).flatten().bool()
        self._reset_opacity_to(0.4, keep)

    def covisibility_prune(self, visibilities, window, mode="slam"):
        """n_obs = the number of window views with n_touched > 0, then prune by covisibility_mask."""
        n_obs = torch.zeros(self.P, dtype=torch.int32, device=self._device())
        for vis in visibilities:
            n_obs += vis.to(n_obs.device).flatten().to(torch.int32)
        self.n_obs = n_obs
        return self.prune(covisibility_mask(self.n_obs, self.kf_id, window, mode))

    # ---- statistics ----
    def add_densification_stats(self, viewspace_grad, update_filter):
        """One view: accumulate |means2D.grad[:, :2]| and a count on the visible rows (gaussian_model.py:963-969)."""
        norm = torch.linalg.vector_norm(viewspace_grad[:, :2], dim=-1, keepdim=True)
        vis = update_filter.view(-1, 1)
        self.accum = torch.where(vis, self.accum + norm, self.accum)
        self.denom = torch.where(vis, self.denom + 1, self.denom)

    def update_max_radii(self, radii, update_filter):
        self.max_radii = torch.where(update_filter, torch.maximum(self.max_radii, radii.to(self.max_radii)), self.max_radii)

    def add_bucket_stats(self, densify, max_radii):
        """The fused path's form: a step's total bucket statistics ([P, 2] sums over the views, max_radii MAX)."""
        self.accum = self.accum + densify[:, 0:1].to(self.accum)
        self.denom = self.denom + densify[:, 1:2].to(self.denom)
        self.max_radii = torch.maximum(self.max_radii, max_radii.to(self.max_radii))

    # ---- the fused layout ----
    def export(self):
        P = self.P
        flat = lambda d: torch.cat([d[n].reshape(P, -1) for n in GROUPS], dim=1)  # noqa: E731
        t = self.t
        return dict(means3D=t["xyz"], shs=torch.cat([t["f_dc"], t["f_rest"]], dim=1), opacities=t["opacity"].reshape(P, 1),
                    scales=t["scaling"], rotations=t["rotation"], language=t["f_language"], exp_avg=flat(self.m),
                    exp_avg_sq=flat(self.v), kf_id=self.kf_id.int(), n_obs=self.n_obs.int(),
                    stats=torch.cat([self.accum, self.denom], dim=1), max_radii=self.max_radii,
                    group_steps=torch.tensor(self.group_steps(), dtype=torch.int64))


# ------------------------------------------------------------------------------------------------------------------------
class GaussianMap:
    """The map of the fused mapping path: parameters, FusedAdam state (per-group steps), accumulators, kfID, n_obs — sized
    to a capacity, edited on the device (olsr_map_edit_plan / _apply).  `params` holds contiguous views [:P] of the
    current buffers (RasterWorkspace / MappingStep take them as they are); every edit replaces the views — read
    `map.params` again after one.  Method names and arguments follow GaussianModel's.

    Host synchronisation: exactly one 4-byte read per topology edit (the new P, which sizes the destination: densify_and_prune,
    prune_points, covisibility_prune, extend, extend_from_rgbd); statistics, resets and Adam steps read nothing back."""

    PARAM_ROWS = dict(means3D=(3,), opacities=(1,), scales=(3,), rotations=(4,))

    def __init__(self, means3D, shs, opacities, scales, rotations, language, lrs: Dict[str, float], kf_id=None, n_obs=None,
                 capacity: Optional[int] = None, percent_dense=0.01, device=None):
        device = torch.device(device if device is not None else means3D.device)
        P = int(means3D.shape[0])
        self.M = int(shs.shape[1]) if shs is not None else 0
        self.F = int(language.shape[1]) if language is not None else 0
        self.layout = GradLayout(self.M, self.F)
        self.device, self.lrs, self.percent_dense = device, dict(lrs), percent_dense
        cap = int(capacity) if capacity is not None else self._grow(P)
        self._bufs = [self._alloc(max(cap, P)), None]
        self._front = 0
        self.P = P
        b = self._bufs[0]
        b["means3D"][:P].copy_(means3D.reshape(P, 3))
        if self.M:
            b["shs"][:P].copy_(shs.reshape(P, self.M, 3))
        b["opacities"][:P].copy_(opacities.reshape(P, 1))
        b["scales"][:P].copy_(scales.reshape(P, 3))
        b["rotations"][:P].copy_(rotations.reshape(P, 4))
        if self.F:
            b["language"][:P].copy_(language.reshape(P, self.F))
        for k in ("exp_avg", "exp_avg_sq", "stats"):
            b[k][:P].zero_()
        b["max_radii"][:P].zero_()
        b["kf_id"][:P].copy_(kf_id.reshape(P)) if kf_id is not None else b["kf_id"][:P].zero_()
        b["n_obs"][:P].copy_(n_obs.reshape(P)) if n_obs is not None else b["n_obs"][:P].zero_()
        self.adam = FusedAdam(0, self.layout, device)
        self.status = torch.zeros(8, dtype=torch.int32, device=device)
        self._scratch = torch.empty(0, dtype=torch.uint8, device=device)
        # groups that skip the next Adam step: a topology edit replaced every parameter ("all"), a reset the opacities
        self.pending_skip = set()
        self.edits = 0   # topology edits so far (MappingStep follows the map when this changes)
        self._views()

    @classmethod
    def from_state(cls, st: Dict[str, torch.Tensor], lrs: Dict[str, float], device, capacity=None, percent_dense=0.01):
        """A map holding `st` (the layout of MapSpec.export() / GaussianMap.state(): parameters, moments in bucket layout,
        kf_id, n_obs, stats, max_radii, group_steps)."""
        dev = torch.device(device)
        f = lambda k: st[k].to(device=dev, dtype=torch.float32)  # noqa: E731
        m = cls(f("means3D"), f("shs") if st["shs"].shape[1] else None, f("opacities"), f("scales"), f("rotations"),
                f("language") if st["language"].shape[1] else None, lrs, kf_id=st["kf_id"].to(dev).int(),
                n_obs=st["n_obs"].to(dev).int(), capacity=capacity, percent_dense=percent_dense, device=dev)
        m.adam.exp_avg.copy_(f("exp_avg"))
        m.adam.exp_avg_sq.copy_(f("exp_avg_sq"))
        m.stats.copy_(f("stats"))
        m.max_radii.copy_(st["max_radii"].to(dev).to(torch.int32))
        m.adam.group_steps = [int(x) for x in st["group_steps"]]
        m.adam.step_count = max(m.adam.group_steps)
        return m

    @classmethod
    def blank(cls, P, M, F, lrs: Dict[str, float], device, capacity=None, percent_dense=0.01):
        """A map of P rows whose parameters are still to be written (load_ply fills them on the device); moments, statistics,
        max_radii, kf_id and n_obs zero."""
        dev = torch.device(device)
        f32 = dict(dtype=torch.float32, device=dev)
        cap = max(int(capacity) if capacity is not None else cls._grow(P), P)
        m = cls(torch.empty(0, 3, **f32), torch.empty(0, M, 3, **f32) if M else None, torch.empty(0, 1, **f32),
                torch.empty(0, 3, **f32), torch.empty(0, 4, **f32), torch.empty(0, F, **f32) if F else None, lrs, capacity=cap,
                percent_dense=percent_dense, device=dev)
        m.P = int(P)
        b = m._bufs[m._front]
        for k in ("exp_avg", "exp_avg_sq", "stats", "max_radii", "kf_id", "n_obs"):
            b[k][:m.P].zero_()
        m._views()
        return m

    # ---- the map on disk (map_io.py) ----
    def save_ply(self, path):
        """GaussianModel.save_ply: point_cloud.ply with the raw parameters, packed on the device (map_io.save_ply)."""
        from . import map_io
        map_io.save_ply(self, path)

    @classmethod
    def load_ply(cls, path, lrs: Dict[str, float], device, F=None, capacity=None, percent_dense=0.01):
        """GaussianModel.load_ply: a map from a point_cloud.ply; optimiser state and accumulators zero (map_io.load_ply).
        F=None keeps the language channels the file has, F=0 drops them as the reference does."""
        from . import map_io
        return map_io.load_ply(path, lrs, device, F=F, capacity=capacity, percent_dense=percent_dense)

    def save_state(self, path):
        """state() as one .npz: the resumable form (map_io.save_state)."""
        from . import map_io
        map_io.save_state(self, path)

    @classmethod
    def load_state(cls, path, lrs: Dict[str, float], device, capacity=None, percent_dense=0.01):
        """The map save_state wrote, through from_state (map_io.load_state)."""
        from . import map_io
        return map_io.load_state(path, lrs, device, capacity=capacity, percent_dense=percent_dense)

    def new_gradients(self):
        """A backward since the last edit produced gradients for the current parameters: the next step updates every group
        again (MappingStep calls this at the start of each iteration)."""
        self.pending_skip = set()

    # ---- storage ----
    @staticmethod
    def _grow(P):
        return max(P + P // 4, P + 1024)

    def _alloc(self, cap):
        d, W = self.device, self.layout.width
        f32, i32 = dict(device=d, dtype=torch.float32), dict(device=d, dtype=torch.int32)
        return dict(means3D=torch.empty(cap, 3, **f32), shs=torch.empty(cap, self.M, 3, **f32),
                    opacities=torch.empty(cap, 1, **f32), scales=torch.empty(cap, 3, **f32),
                    rotations=torch.empty(cap, 4, **f32), language=torch.empty(cap, self.F, **f32),
                    exp_avg=torch.empty(cap, W, **f32), exp_avg_sq=torch.empty(cap, W, **f32),
                    kf_id=torch.empty(cap, **i32), n_obs=torch.empty(cap, **i32), stats=torch.empty(cap, 2, **f32),
                    max_radii=torch.empty(cap, **i32), cap=cap)

    @property
    def capacity(self):
        return self._bufs[self._front]["cap"]

    def _views(self):
        b, P = self._bufs[self._front], self.P
        self.params = dict(means3D=b["means3D"][:P], shs=b["shs"][:P] if self.M else None, opacities=b["opacities"][:P],
                           scales=b["scales"][:P], rotations=b["rotations"][:P],
                           language=b["language"][:P] if self.F else None)
        self.kf_id, self.n_obs = b["kf_id"][:P], b["n_obs"][:P]
        self.stats, self.max_radii = b["stats"][:P], b["max_radii"][:P]
        self.adam.exp_avg, self.adam.exp_avg_sq = b["exp_avg"][:P], b["exp_avg_sq"][:P]

    @staticmethod
    def _struct(b, P=None):
        def p(k):
            return ptr(b.get(k))
        return _abi.OlsrMapBuffers(**{k: p(k) for k in ("means3D", "shs", "opacities", "scales", "rotations", "language",
                                                         "exp_avg", "exp_avg_sq", "kf_id", "n_obs", "stats", "max_radii")})


    # ---- the edit primitive ----
    def _edit(self, ep: _abi.OlsrMapEditParams, drop_mask=None, z=None, append=None, P_new: Optional[int] = None):
        """P_new: the size after the edit when the caller knows it (a pure append: P + n) — the plan's status is then not
        read back and the edit makes no host synchronisation of its own."""
        L, P = lib(), self.P
        need = int(L.olsr_map_edit_scratch_bytes(P))
        if self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        src = self._struct(self._bufs[self._front])
        check(L.olsr_map_edit_plan(P, C.byref(ep), C.byref(src), drop_mask.data_ptr() if drop_mask is not None else None,
                                   self._scratch.data_ptr(), self.status.data_ptr(), stream_ptr(self.device)))
        if P_new is None:
            P_new = int(self.status[0].item())   # the edit's one host synchronisation: the destination's size
        back = 1 - self._front
        if self._bufs[back] is None or self._bufs[back]["cap"] < P_new:
            self._bufs[back] = None
            self._bufs[back] = self._alloc(max(self._grow(P_new), self.capacity))
        src_index = torch.empty(max(P_new, 1), dtype=torch.int32, device=self.device)[:P_new]
        dst = self._struct(self._bufs[back])
        app = self._struct(append) if append is not None else None
        check(L.olsr_map_edit_apply(P, self.M, self.F, C.byref(ep), C.byref(src), z.data_ptr() if z is not None else None,
                                    C.byref(app) if app is not None else None, self._scratch.data_ptr(),
                                    self.status.data_ptr(), P_new, self._bufs[back]["cap"], C.byref(dst),
                                    src_index.data_ptr() if P_new > 0 else None, stream_ptr(self.device)))
        self._front, self.P = back, P_new
        self.edits += 1
        self._views()
        self.pending_skip = set(GROUPS)   # every parameter was replaced: the reference's next optimizer.step() updates nothing
        return src_index

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, z: Optional[torch.Tensor] = None,
                          generator: Optional[torch.Generator] = None):
        """GaussianModel.densify_and_prune (clone, split with N = 2, prune).  z: float32 [P, 2, 3] standard normal noise
        indexed by SOURCE row (child k of row j uses z[j, k]); drawn here from `generator` when not given.  The reference's
        max_radii2D > max_screen_size term never fires (its densification_postfix zeroes max_radii2D first), and neither
        does it here; max_screen_size only switches the world-space term max(exp(scaling)) > 0.1 extent on.
        Returns src_index (int32 [P_new])."""
        if z is None:
            z = torch.randn(self.P, 2, 3, generator=generator, device=self.device)
        z = z.to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(z.shape) != (self.P, 2, 3):
            raise ValueError(f"z must be [P, 2, 3] = [{self.P}, 2, 3]")
        ep = _abi.OlsrMapEditParams(mode=_abi.MAP_EDIT_DENSIFY, n_append=0, append_kf_id=0,
                                    screen_size_term=1 if max_screen_size else 0, max_grad=max_grad, min_opacity=min_opacity,
                                    clone_max_scale=self.percent_dense * extent, big_scale=0.1 * extent)
        return self._edit(ep, z=z)

    def prune_points(self, mask: torch.Tensor):
        """GaussianModel.prune_points: drop the rows where mask is True (moments and accumulators follow the kept rows)."""
        mask = mask.to(device=self.device).reshape(self.P).to(torch.uint8).contiguous()
        ep = _abi.OlsrMapEditParams(mode=_abi.MAP_EDIT_MASK)
        return self._edit(ep, drop_mask=mask)

    def extend(self, means3D, shs, opacities, scales, rotations, kf_id: int, _known_size=False):
        """GaussianModel.extend_from_pcd with ready rows: language zero, kfID = kf_id, n_obs 0, zero moments; the
        accumulators of every row are zeroed (densification_postfix).  (_known_size: an append drops no row, so P_new =
        P + n needs no read of the plan's status — extend_from_rgbd, whose one host read has already happened.)"""
        n = int(means3D.shape[0])
        f32 = dict(device=self.device, dtype=torch.float32)
        app = dict(means3D=means3D.to(**f32).reshape(n, 3).contiguous(),
                   shs=shs.to(**f32).reshape(n, self.M, 3).contiguous() if self.M else None,
                   opacities=opacities.to(**f32).reshape(n).contiguous(), scales=scales.to(**f32).reshape(n, 3).contiguous(),
                   rotations=rotations.to(**f32).reshape(n, 4).contiguous())
        ep = _abi.OlsrMapEditParams(mode=_abi.MAP_EDIT_MASK, n_append=n, append_kf_id=int(kf_id))
        return self._edit(ep, append=app, P_new=self.P + n if _known_size else None)

    def extend_from_rgbd(self, image, depth, w2c, intrinsics, kf_id: int, *, init=False, downsample: Optional[int] = None,
                         seed: Optional[int] = None, exposure=None, rgb_boundary_threshold=0.01, point_size=0.05,
                         adaptive_pointsize=True):
        """GaussianModel.extend_from_pcd_seq — FrontEnd.add_new_keyframe + BackEnd.add_next_kf of the reference: the rows
        of the keyframe's new Gaussians from its RGB-D image (keyframe_seed.seed_rows, on the device), then `extend`.
        downsample: Dataset.pcd_downsample_init = 32 when `init`, else pcd_downsample = 64 (configs/rgbd/base_config.yaml:
        11-12); seed of the sampling hash: kf_id.  One host read in all (the number of new rows).  Returns src_index
        (int32 [P_new]: the old rows 0 .. P - 1, then -(k + 1) for new row k).  When the frame yields fewer than four rows
        (no three neighbours for their scales) nothing is appended and the map is left as it is."""
        from .keyframe_seed import seed_rows
        if downsample is None:
            downsample = 32 if init else 64
        rows = seed_rows(image, depth, w2c, intrinsics, downsample=int(downsample), seed=int(kf_id if seed is None else seed),
                         exposure=exposure, rgb_boundary_threshold=rgb_boundary_threshold, point_size=point_size,
                         adaptive_pointsize=adaptive_pointsize, M=max(self.M, 1))
        if int(rows["means3D"].shape[0]) == 0:
            return torch.arange(self.P, dtype=torch.int32, device=self.device)
        return self.extend(rows["means3D"], rows["shs"], rows["opacities"], rows["scales"], rows["rotations"], kf_id,
                           _known_size=True)

    def covisibility_prune(self, visibilities: Sequence[torch.Tensor], window: Sequence[int], mode="slam"):
        """The back end's co-visibility prune of a full window (slam_backend.py:683-716): n_obs = the number of window views
        with n_touched > 0, then prune_points.  `visibilities`: one bool / int [P] tensor per window view."""
        self.n_obs.zero_()
        for v in visibilities:
            self.n_obs.add_(v.to(device=self.device).reshape(self.P).to(torch.int32))
        return self.prune_points(covisibility_mask(self.n_obs, self.kf_id, window, mode))

    def _opacity_constant(self, value):
        return opacity_logit(value).to(self.device)   # (fp32 on the CPU, where tests/golden/map_edit.npz was recorded)

    def reset_opacity(self):
        """Every opacity to inverse_sigmoid(0.01); the opacity moments of every row zeroed; the opacity group skips the
        next step (its step count lags the others from then on)."""
        self.params["opacities"].copy_(self._opacity_constant(0.01).expand_as(self.params["opacities"]))
        self._zero_opacity_moments()

    def reset_opacity_nonvisible(self, visibility_filters: Sequence[torch.Tensor]):
        """Opacity inverse_sigmoid(0.4) on the Gaussians visible in none of the filters, the rest kept; opacity moments
        zeroed and the opacity step skipped as in reset_opacity."""
        vis = torch.zeros(self.P, dtype=torch.bool, device=self.device)
        for f in visibility_filters:
            vis |= f.to(device=self.device).reshape(self.P).bool()
        op = self.params["opacities"]
        op.copy_(torch.where(vis.view(-1, 1), op, self._opacity_constant(0.4)))
        self._zero_opacity_moments()

    def _zero_opacity_moments(self):
        c = self.layout.slices()["opacity"]
        self.adam.exp_avg[:, c].zero_()
        self.adam.exp_avg_sq[:, c].zero_()
        self.pending_skip.add("opacity")

    # ---- statistics and the optimiser step ----
    def add_densification_stats(self, bucket):
        """The step's total bucket (GradientBucket after the lane sum / exchange): its densify [P, 2] statistics are the
        reference's per-view add_densification_stats summed over the views, its max_radii the max_radii2D update."""
        self.stats.add_(bucket.densify)
        torch.maximum(self.max_radii, bucket.max_radii, out=self.max_radii)

    def step(self, buckets, lrs: Optional[Dict[str, float]] = None, skip=(), isotropic=None, activations=_abi.ACT_ALL):
        """FusedAdam over the map's parameters; the groups an edit since the last step replaced (pending_skip) and `skip`
        do not step.  isotropic / activations: FusedAdam.step's (the mapping loss's isotropic regulariser, formed inside
        the step).  Returns the set of groups that skipped."""
        sk = set(self.pending_skip) | (set(GROUPS) if skip == "all" else set(skip))
        self.pending_skip = set()
        if self.P > 0:
            self.adam.step(buckets, self.params, lrs if lrs is not None else self.lrs, skip=sk, isotropic=isotropic,
                           activations=activations)
        return sk

    @property
    def group_steps(self):
        return list(self.adam.group_steps)

    def state(self):
        """The map in the fused layout (views), for comparisons with MapSpec.export()."""
        b, P = self._bufs[self._front], self.P
        return dict(self.params, shs=b["shs"][:P], language=b["language"][:P], exp_avg=self.adam.exp_avg,
                    exp_avg_sq=self.adam.exp_avg_sq, kf_id=self.kf_id,
                    n_obs=self.n_obs, stats=self.stats, max_radii=self.max_radii,
                    group_steps=torch.tensor(self.group_steps, dtype=torch.int64))
