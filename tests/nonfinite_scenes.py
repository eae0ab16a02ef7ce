"""Scenes with planted non-finite and overflowing Gaussians: the rows an online optimiser produces when a Gaussian runs away.
CPU module, no GPU code: tests/test_nonfinite_scenes_cpu.py asks the oracle alone what they do, tests/test_gpu_nonfinite.py
holds the HIP rasteriser to it.

planted_scene(kind, P, W, H, F, seed, where, count) builds make_scene(P, W, H, F, seed) and overwrites `count` Gaussians,
chosen among those the unplanted scene's oracle run reports visible (radius > 0, and blending at least one pixel), at the rows `where` names:
"first" / "last" (row 0 / P - 1), "wave" (rows 63 / 64) and "block" (rows 255 / 256) where P allows, "all" (all of these in
turn), "upper" (rows 64 and 256, among the splats of radius <= 16 only, so that most of the frame lies outside their tile
rects and the containment statements have something to hold); a row that is not visible is replaced by the nearest visible one.  KINDS lists the classes; one value of the row is
overwritten unless the class says otherwise.

`prefiltered` stays False everywhere: with it set a culled point reaches the kernel's trap by design, as in the reference.
"""
import functools
import struct
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from parity_common import fwd_args  # (first: it puts the repository root on sys.path)
from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.scene import Scene, make_scene

NAN, INF = float("nan"), float("inf")
NEG_NAN_BITS = -0x400000  # 0xFFC00000 as int32: a quiet NaN with the sign bit set
SIZES = ((45, 30, 15), (64, 48, 16))  # (W, H, tile): 3 x 2 tiles of 15 (ragged at 16); 4 x 3 tiles of 16
P_VALUES = (1, 64, 65, 257)
F_VALUES = (0, 15)
SCALE_MULT = 0.3  # make_scene's splats fill these small frames; a third of their size leaves room around a planted one
TARGET_ROWS = dict(first=(0,), last=(-1,), wave=(63, 64), block=(255, 256), all=(0, -1, 63, 64, 255, 256),
                   upper=(64, 256, 0))  # the first row of the second wave and of the second block (row 0 where P has neither)


def _oracle():
    from oracle import oracle_C
    oracle_C.lib()
    return oracle_C


def oracle_forward(sc, tile, **kw):
    """The oracle's forward alone: dict(R, color, language, radii, depth, opacity, n_touched, point_list, keys, final_T,
    n_contrib, reached).  The state is released."""
    O = _oracle()
    O.TILE = tile
    O.lib().oracle_set_record(1)
    a = fwd_args(sc, None, **kw)
    if sc.F > 0:
        R, color, lang, radii, geom, _b, _i, depth, opac, nt = O.rasterize_language_gaussians(*a)
    else:
        R, color, radii, geom, _b, _i, depth, opac, nt = O.rasterize_gaussians(*a)
        lang = None
    out = dict(R=R, color=color, language=lang, radii=radii, depth=depth, opacity=opac, n_touched=nt)
    for k in ("point_list", "keys", "final_T", "n_contrib", "contrib_mask"):
        out[k] = O.get_field(geom, k)
    O.release(geom)
    O.lib().oracle_set_record(0)
    # reached[g]: the number of (pixel, list entry) visits in which Gaussian g is blended
    bits = np.unpackbits(out.pop("contrib_mask").numpy().view(np.uint8)).reshape(-1, 256).sum(1) if R else np.zeros(0)
    out["reached"] = torch.zeros(sc.P, dtype=torch.int64).index_add_(0, out["point_list"].long(), torch.from_numpy(bits).long())
    return out


def _row(sc, i):
    """Gaussian i of `sc` as a scene of its own (the radius of a Gaussian depends on no other)."""
    s = slice(i, i + 1)
    return Scene(sc.camera, sc.means3D[s].clone(), sc.opacities[s].clone(), sc.scales[s].clone(), sc.rotations[s].clone(),
                 sc.shs[s].clone(), None if sc.language is None else sc.language[s].clone(), sc.sh_degree, sc.bg, sc.F)


def radius_edge(sc, i, limit=1 << 20):
    """The largest float32 s with oracle radius(scales[i] = (s, s, s)) < limit and its successor (radius >= limit), by
    bisection over the float's bits between 1 and 1e12: the two sides of preprocess's `irad < (1 << 20)` hand-over."""
    one = _row(sc, i)

    def radius(bits):
        one.scales[0, :] = torch.tensor([bits], dtype=torch.int32).view(torch.float32)
        return int(oracle_forward(one, 15)["radii"][0])
    lo, hi = (struct.unpack("<i", struct.pack("<f", v))[0] for v in (1.0, 1e12))
    assert 0 < radius(lo) < limit <= radius(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if radius(mid) < limit:
            lo = mid
        else:
            hi = mid
    f = lambda b: struct.unpack("<f", struct.pack("<i", b))[0]  # noqa: E731
    return f(lo), f(hi)


# ------------------------------------------------------------------------------------------------ the classes
# t: dict of the scene's tensors (clones) plus colors_precomp / cov3D_precomp where the class renders from them; i: the row.
def _put(name, col, value):
    def fn(t, i, sc):
        if col is None:
            t[name][i] = value
        else:
            t[name][i, col] = value
    return fn


def _neg_nan_z(t, i, sc):
    t["means3D"].view(torch.int32)[i, 2] = NEG_NAN_BITS


def _scale_edge(side):
    def fn(t, i, sc):
        t["scales"][i, :] = radius_edge(sc, i)[side]
    return fn


def _negate_scale(t, i, sc):
    t["scales"][i, 1] = -t["scales"][i, 1]


def _times(name, factor):
    def fn(t, i, sc):
        t[name][i] = t[name][i] * factor
    return fn


# name -> (group, needs, fn); needs: None, "cov" (cov3D_precomp), "colors" (colors_precomp), "lang" (F > 0), "raw"
KINDS = {
    "mean_nan_x": ("mean", None, _put("means3D", 0, NAN)),
    "mean_inf_z": ("mean", None, _put("means3D", 2, INF)),
    "mean_ninf_y": ("mean", None, _put("means3D", 1, -INF)),
    "mean_negnan_z": ("mean", None, _neg_nan_z),
    "scale_nan": ("scale", None, _put("scales", 0, NAN)),
    "scale_inf": ("scale", None, _put("scales", 0, INF)),
    "scale_1e20": ("scale", None, _put("scales", 0, 1e20)),
    "scale_1e12": ("scale", None, _put("scales", None, 1e12)),
    "scale_below_2p20": ("scale", None, _scale_edge(0)),
    "scale_above_2p20": ("scale", None, _scale_edge(1)),
    "scale_zero": ("scale", None, _put("scales", None, 0.0)),
    "scale_negative": ("scale", None, _negate_scale),
    "rot_zero": ("rotation", None, _put("rotations", None, 0.0)),
    "rot_nan": ("rotation", None, _put("rotations", 2, NAN)),
    "rot_1e20": ("rotation", None, _times("rotations", 1e20)),
    "cov_nan": ("cov", "cov", _put("cov3D_precomp", 3, NAN)),
    "cov_inf": ("cov", "cov", _put("cov3D_precomp", 0, INF)),
    "cov_zero": ("cov", "cov", _put("cov3D_precomp", None, 0.0)),
    "op_nan": ("opacity", None, _put("opacities", 0, NAN)),
    "op_inf": ("opacity", None, _put("opacities", 0, INF)),
    "op_neg": ("opacity", None, _put("opacities", 0, -0.5)),
    "op_zero": ("opacity", None, _put("opacities", 0, 0.0)),
    "op_one": ("opacity", None, _put("opacities", 0, 1.0)),
    "op_two": ("opacity", None, _put("opacities", 0, 2.0)),
    "lang_nan": ("feature", "lang", _put("language", 3, NAN)),
    "sh_inf": ("feature", None, lambda t, i, sc: t["shs"].__setitem__((i, 0, 1), INF)),
    "color_nan": ("feature", "colors", _put("colors_precomp", 2, NAN)),
    # raw parameters, every OLSR_ACT_* flag set: `scales` holds log-scales, `opacities` logits, `rotations` any quaternion
    "raw_scale_89": ("raw", "raw", _put("scales", 0, 89.0)),        # exp overflows to +inf
    "raw_scale_m104": ("raw", "raw", _put("scales", None, -104.0)),  # exp underflows to 0
    "raw_op_pinf": ("raw", "raw", _put("opacities", 0, INF)),
    "raw_op_ninf": ("raw", "raw", _put("opacities", 0, -INF)),
    "raw_op_104": ("raw", "raw", _put("opacities", 0, 104.0)),      # sigmoid exactly 1
    "raw_op_m104": ("raw", "raw", _put("opacities", 0, -104.0)),    # sigmoid exactly 0
    "raw_rot_zero": ("raw", "raw", _put("rotations", None, 0.0)),   # the normalisation's 0 / max(0, 1e-12) = 0
    "raw_nan_mean": ("raw", "raw", _put("means3D", 1, NAN)),
    "raw_nan_scale": ("raw", "raw", _put("scales", 1, NAN)),
    "raw_nan_rot": ("raw", "raw", _put("rotations", 0, NAN)),
    "raw_nan_op": ("raw", "raw", _put("opacities", 0, NAN)),
}
FORWARD_ONLY = tuple(k for k, v in KINDS.items() if v[0] == "feature")
# what a mixture cycles through: the classes that need no precomputed array (those exclude scales / SH)
MIX = tuple(k for k, v in KINDS.items() if v[1] in (None, "lang"))
MIXTURES = ("mix_all", "all_planted", "copies64")
GEOMETRY_AND_OPACITY = tuple(k for k, v in KINDS.items() if v[0] in ("mean", "scale", "rotation", "cov", "opacity"))


@dataclass
class Planted:
    kind: str
    scene: Scene              # the planted scene (raw kinds: raw parameters in opacities / scales / rotations)
    base: Scene               # the scene before planting
    idx: torch.Tensor         # planted rows, int64, ascending
    kinds: list               # the class planted in each of them
    kw: dict = field(default_factory=dict)       # colors_precomp / cov3D_precomp of the planted scene (run_backend's **kw)
    base_kw: dict = field(default_factory=dict)  # ... of the scene before planting
    raw: bool = False
    forward_only: bool = False

    @property
    def activations(self):
        return _abi.ACT_ALL if self.raw else 0

    def activated(self, which="scene"):
        """What the oracle renders: the scene itself, or — raw kinds — its activation in float32 on the CPU.  The planted
        values activate to the same 0 / 1 / inf / NaN as on the device; ordinary rows differ from the device's expf in the
        last bit, which is why the GPU test compares raw kinds with the device's own activation, not with this."""
        sc = getattr(self, which)
        if not self.raw:
            return sc
        q = sc.rotations
        n = (q * q).sum(1, keepdim=True).sqrt()
        n = torch.where(n.isnan(), torch.full_like(n, 1e-12), n.clamp_min(1e-12))  # the device's fmaxf(|q|, 1e-12): F.normalize
        return Scene(sc.camera, sc.means3D, torch.sigmoid(sc.opacities), torch.exp(sc.scales),
                     q / n, sc.shs, sc.language, sc.sh_degree, sc.bg, sc.F)

    def deleted(self):
        """The planted scene without its planted rows (and the same of its precomputed arrays)."""
        keep = torch.ones(self.scene.P, dtype=torch.bool)
        keep[self.idx] = False
        sc = self.scene
        cut = lambda t: None if t is None else t[keep].contiguous()  # noqa: E731
        return (Scene(sc.camera, cut(sc.means3D), cut(sc.opacities), cut(sc.scales), cut(sc.rotations), cut(sc.shs),
                      cut(sc.language), sc.sh_degree, sc.bg, sc.F), {k: cut(v) for k, v in self.kw.items()}, keep)


def cov3d_of(sc):
    """[P, 6] upper triangle of R S S^T R^T in float32 (what a caller of cov3D_precomp hands in; its own rounding is of no
    concern: oracle and library read the same array)."""
    q = sc.rotations / sc.rotations.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    M = R * sc.scales.unsqueeze(1)
    S = M @ M.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()


def _pick(visible, P, where, count):
    rows = [r % P for r in TARGET_ROWS[where] if -P <= r < P]
    if where == "upper" and len(rows) > 1:
        rows = rows[:-1]
    vis = visible.nonzero().reshape(-1).tolist()
    assert vis, "no visible Gaussian to plant"
    chosen = []
    for k in range(count):
        free = [v for v in vis if v not in chosen]
        if not free:
            break
        r = rows[k % len(rows)]
        chosen.append(min(free, key=lambda v: (abs(v - r), v)))
    return sorted(chosen)


def _raw_of(sc, seed):
    g = torch.Generator().manual_seed(900 + seed)
    return Scene(sc.camera, sc.means3D, torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4)).contiguous(),
                 torch.log(sc.scales).contiguous(), (sc.rotations * (0.3 + 2 * torch.rand(sc.P, 1, generator=g))).contiguous(),
                 sc.shs, sc.language, sc.sh_degree, sc.bg, sc.F)


@functools.lru_cache(maxsize=None)
def planted_scene(kind, P, W, H, F, seed=0, where="all", count=1):
    """See the module's docstring.  Mixtures: "mix_all" plants every class of MIX once (count is ignored; at most the
    visible rows), "all_planted" plants EVERY row, cycling through MIX, "copies64" is 64 copies of one visible Gaussian, all in the tile of its mean and at
    one depth, alternately with a NaN scale (culled: radius 0) and a NaN opacity (each blends alpha = 0.99); P is ignored."""
    base = make_scene(P, W, H, F, seed=seed, scale_mult=SCALE_MULT)
    if kind == "copies64":
        vis = oracle_forward(base, 15)["radii"] > 0
        i = _pick(vis, P, "first", 1)[0]
        rep = lambda t: None if t is None else t[i:i + 1].repeat(*([64] + [1] * (t.dim() - 1))).contiguous()  # noqa: E731
        base = Scene(base.camera, rep(base.means3D), rep(base.opacities), rep(base.scales), rep(base.rotations), rep(base.shs),
                     rep(base.language), base.sh_degree, base.bg, F)
        P = 64
    need = KINDS[kind][1] if kind in KINDS else None
    assert need != "lang" or F > 0, "a language class needs language channels"
    raw = need == "raw"
    if raw:
        base = _raw_of(base, seed)
    base_kw = {}
    if need == "cov":
        base_kw["cov3D_precomp"] = cov3d_of(base)
    if need == "colors":
        base_kw["colors_precomp"] = torch.rand(P, 3, generator=torch.Generator().manual_seed(700 + seed)).contiguous()
    probe = Planted(kind, base, base, torch.empty(0, dtype=torch.int64), [], base_kw, base_kw, raw)
    seen = oracle_forward(probe.activated("base"), 15, **base_kw)
    # visible, and blended by at least one pixel: a planted row that hides behind saturated pixels would test nothing in the
    # composite
    visible = (seen["radii"] > 0) & (seen["reached"] > 0)
    if where == "upper" and bool((visible & (seen["radii"] <= 16)).any()):
        visible &= seen["radii"] <= 16
    if kind == "mix_all":
        kinds = [k for k in MIX if F > 0 or KINDS[k][1] != "lang"]
        idx = _pick(visible, P, "all", len(kinds))
    elif kind == "all_planted":
        idx = list(range(P))
        cyc = [k for k in MIX if F > 0 or KINDS[k][1] != "lang"]
        kinds = [cyc[i % len(cyc)] for i in idx]
    elif kind == "copies64":
        idx, kinds = list(range(64)), ["scale_nan", "op_nan"] * 32
    else:
        idx = _pick(visible, P, where, count)
        kinds = [kind] * len(idx)
    kinds = kinds[:len(idx)]
    t = dict(means3D=base.means3D.clone(), opacities=base.opacities.clone(), scales=base.scales.clone(),
             rotations=base.rotations.clone(), shs=base.shs.clone(), language=None if base.language is None else base.language.clone())
    for k, v in base_kw.items():
        t[k] = v.clone()
    for i, k in zip(idx, kinds):
        KINDS[k][2](t, i, base)
    sc = Scene(base.camera, t["means3D"], t["opacities"], t["scales"], t["rotations"], t["shs"], t["language"], base.sh_degree,
               base.bg, F)
    fwd_only = any(k in FORWARD_ONLY for k in kinds)
    return Planted(kind, sc, base, torch.tensor(idx, dtype=torch.int64), kinds, {k: t[k] for k in base_kw}, base_kw, raw, fwd_only)


def module_scenes():
    """(id, kind, P, W, H, tile, F, where, count) of every scene the two test files run: each class once at P = 257 on
    45 x 30 with 15 language channels, planted in rows 64 and 256, four of them also in all six boundary rows; the P and F edges and the 16-pixel tile on the
    classes that reach the most paths; the mixtures."""
    rows = []
    for kind in KINDS:
        rows.append((kind, 257, 45, 30, 15, 15, "upper", 2))
    for kind in ("mean_nan_x", "scale_1e12", "op_nan", "scale_nan"):
        rows.append((kind, 257, 45, 30, 15, 15, "all", 6))
    for P in (1, 64, 65):
        for kind in ("scale_nan", "scale_1e12", "op_nan", "mean_negnan_z"):
            rows.append((kind, P, 45, 30, 15, 0, "all", 2))
    for kind in ("scale_inf", "scale_above_2p20", "rot_zero", "op_two", "raw_scale_89"):
        rows.append((kind, 65, 64, 48, 16, 0, "all", 2))
    for kind in ("mean_nan_x", "scale_1e12", "op_nan", "scale_nan"):   # the 45 x 30 frame is ragged at 16-pixel tiles
        rows.append((kind, 257, 45, 30, 16, 15, "all", 6))
    for kind in ("mix_all", "all_planted", "copies64"):
        rows.append((kind, 257 if kind == "mix_all" else 65, 45, 30, 16, 15, "all" if kind != "copies64" else "first", 0))
    rows.append(("mix_all", 257, 45, 30, 15, 15, "all", 0))
    rows.append(("mix_all", 257, 64, 48, 16, 0, "all", 0))
    rows.append(("all_planted", 65, 45, 30, 15, 15, "all", 0))
    rows.append(("copies64", 65, 45, 30, 15, 15, "first", 0))
    return [(f"{k}-P{P}-{W}x{H}-t{tile}-F{F}-{where}{count}", k, P, W, H, tile, F, where, count) for k, P, W, H, tile, F, where, count in rows]


def scene_of(row):
    _id, kind, P, W, H, _tile, F, where, count = row
    return planted_scene(kind, P, W, H, F, seed=11, where=where, count=count)


def planted_tiles(out, idx, P):
    """Tiles (ids, a set) in which the oracle's lists hold a planted Gaussian."""
    pl, keys = out["point_list"].long(), out["keys"]
    if pl.numel() == 0:
        return set()
    hit = torch.isin(pl, idx)
    return set((keys[hit] >> 32).tolist())


def pixel_mask_of_tiles(tiles, W, H, tile):
    """bool [H, W]: the pixels of `tiles`."""
    gx = (W + tile - 1) // tile
    m = torch.zeros(H, W, dtype=torch.bool)
    for t in tiles:
        y, x = divmod(int(t), gx)
        m[y * tile:(y + 1) * tile, x * tile:(x + 1) * tile] = True
    return m


# ------------------------------------------------------------------------------------------------ the raw file of oracle/ubsan_main.cpp
def write_raw(path, rows=None):
    """Every scene of the module (the oracle's inputs, cotangents included) as one little-endian file for oracle/ubsan_main.cpp:
    int32 count, then per scene int32 {P, D, M, F, W, H, tile, has_colors, has_cov}, float32 {tan_fovx, tan_fovy}, and the
    float32 arrays background[3], means3D[3P], shs[3MP] (has_colors = 0), colors[3P] (has_colors = 1), language[FP],
    opacities[P], scales[3P] and rotations[4P] (has_cov = 0), cov3D[6P] (has_cov = 1), view[16], proj[16], proj_raw[16],
    campos[3], dL_dcolor[3HW], dL_dlanguage[FHW], dL_ddepth[HW]."""
    rows = module_scenes() if rows is None else rows
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(rows)))
        for row in rows:
            p = scene_of(row)
            sc, tile = p.activated(), row[5]
            cam = sc.camera
            col, cov = p.kw.get("colors_precomp"), p.kw.get("cov3D_precomp")
            M = sc.shs.shape[1]
            f.write(struct.pack("<9i", sc.P, sc.sh_degree, M, sc.F, cam.width, cam.height, tile, int(col is not None),
                                int(cov is not None)))
            f.write(struct.pack("<2f", cam.tanfovx, cam.tanfovy))
            dc, dl, dd = sc.cotangents(3)
            arrays = [sc.bg, sc.means3D, col if col is not None else sc.shs, sc.language, sc.opacities]
            arrays += [cov] if cov is not None else [sc.scales, sc.rotations]
            arrays += [cam.world_view_transform, cam.full_proj_transform, cam.projection_matrix, cam.camera_center, dc, dl, dd]
            for a in arrays:
                if a is not None:
                    f.write(np.ascontiguousarray(a.detach().float().numpy()).astype("<f4").tobytes())
    return len(rows)


if __name__ == "__main__":
    import sys
    print(f"{write_raw(sys.argv[1])} scenes written to {sys.argv[1]}")
