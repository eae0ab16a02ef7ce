"""Scenes on which DGR-D's own kernels, built on the host (oracle/ref_build.py, oracle/oracle_ref_dgrd.py), are compared
with the restatement tests/dgrd_oracle.py (tests/test_dgrd_ref_build_cpu.py) and with the product
(tests/test_gpu_dgrd_ref_build.py).  The pattern of tests/ref_scenes.py: every scene carries the conditions that make it
worth running, `conditions(name)` measures them on the DGR-D BUILD's own output and asserts them, runs are cached and
nothing modifies a cached result.

A scene is the dict tests/dgrd_oracle.py and oracle/oracle_ref_dgrd.py take: a make_scene scene plus a second opacity /
scale / rotation set.  All are small (P <= 1000, at most 64x48 pixels, 16-pixel tiles).
"""
import functools
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from online_lang_splatting_amd import _abi  # noqa: E402
from online_lang_splatting_amd.scene import Scene, default_camera, make_scene  # noqa: E402
from nonfinite_scenes import cov3d_of  # noqa: E402

TILE = 16
SEED = 3  # of the cotangents


def second_set(s, P, seed):
    """A second opacity / scale / rotation set over the Gaussians of scene dict `s` (which holds the first)."""
    g = torch.Generator().manual_seed(4242 + seed)
    s["opacities_lang"] = torch.rand(P, 1, generator=g) * 0.9 + 0.05
    s["scales_lang"] = s["scales"] * torch.exp(torch.randn(P, 3, generator=g) * 0.5)
    q = torch.randn(P, 4, generator=g)
    s["rotations_lang"] = q / q.norm(dim=1, keepdim=True)
    return g


def scene2(P, W, H, F=3, seed=0, border=False, large=0.08, **kw):
    """A make_scene scene plus a second set.  border: a handful of Gaussians sit just outside the image with a first set
    too small to reach it and a second set large enough (and the reverse), the case in which DGR-D reports the radius of
    a set that covers no tile (large: that set's scale, for a radius of 8 to 11 pixels at the image's focal length)."""
    kw.setdefault("max_sh_degree", 1)
    sc = make_scene(P, W, H, F, seed=seed, **kw)
    s = dict(camera=sc.camera, bg=sc.bg, means3D=sc.means3D.clone(), opacities=sc.opacities, scales=sc.scales.clone(),
             rotations=sc.rotations, shs=sc.shs, sh_degree=sc.sh_degree, language=sc.language)
    g = second_set(s, P, seed)
    if border:
        k = min(64, P // 4)
        z = 3.0
        # make_scene's default camera sits at the origin and looks down +z: pixel x = fx * X / Z + (W - 1) / 2.
        # 4.5 pixels right of the tile grid: the small set (radius 3) reaches no tile, the large one (radius 11) does.
        fx = W / 2.0
        gx = (W + 15) // 16
        x_out = ((gx * 16 + 4.5) - (W - 1) / 2.0) / fx * z
        ys = (torch.rand(k, generator=g) - 0.5) * (H / fx) * z * 0.8
        s["means3D"][:k] = torch.stack([torch.full((k,), x_out), ys, torch.full((k,), z)], 1)
        small = 0.0005
        s["scales"][: k // 2] = small
        s["scales_lang"][: k // 2] = large
        s["scales"][k // 2: k] = large
        s["scales_lang"][k // 2: k] = small
    return s


def _as_scene(s, sfx):
    """One set of a scene dict as a Scene (for cov3d_of)."""
    return Scene(s["camera"], s["means3D"], s["opacities" + sfx], s["scales" + sfx], s["rotations" + sfx], s["shs"],
                 s["language"], s["sh_degree"], s["bg"], s["language"].shape[1])


def _dense():
    # set 1 is faint right of the optical axis, so its pixels there walk their lists to the end; set 2 is four times as
    # large left of it, so the two sets' lists differ in length and in where they saturate
    s = scene2(1000, 64, 48, 3, seed=11)
    right = s["means3D"][:, 0:1] > 0
    s["opacities"] = torch.where(right, s["opacities"] * 0.02, s["opacities"]).contiguous()
    s["scales_lang"] = torch.where(~right, s["scales_lang"] * 4.0, s["scales_lang"]).contiguous()
    return s


def _sh(active, max_degree):
    s = scene2(300, 32, 32, 3, seed=20 + 4 * active + max_degree, max_sh_degree=max_degree, sh_degree=active)
    s["shs"][:, 0, :] *= 2.5  # SH_C0 * dc + 0.5 now leaves [0, 1] for many Gaussians: clamped channels
    return s


def _base(P=300, W=47, H=31, F=3, seed=5, **kw):
    return scene2(P, W, H, F, seed=seed, **kw)


def _colors(s):
    g = torch.Generator().manual_seed(701)
    s["colors_precomp"] = (torch.rand(s["means3D"].shape[0], 3, generator=g) * 1.4 - 0.2).contiguous()
    return s


def _precomp(s, *sfxs):
    for sfx in sfxs:
        s["cov3D_precomp" + sfx] = cov3d_of(_as_scene(s, sfx))
    return s


def _all_culled():
    s = _base(64, seed=9)
    s["means3D"][:, 2] = -s["means3D"][:, 2].abs() - 0.01  # behind the camera: p_view.z <= 0.2 for every one
    return s


# ---- one_zero_det: needles whose float32 2D covariance has determinant a*c - b*b == 0 although 0.3 sits on its diagonal
N_CAND, N_ONE, N_BOTH = 48, 3, 2


def _needle_candidates(W, H):
    """N_CAND needles 0.3-1 m in front of the camera, lying in the image plane: positions, scales, rotations, and per
    needle whether the plain oracle's preprocess finds det == 0 (it returns there: radius 0 inside the frustum)."""
    from oracle import oracle_C as O
    g = torch.Generator().manual_seed(977)
    n = N_CAND
    cam = default_camera(W, H)
    fx = W / 2.0
    z = torch.rand(n, generator=g) * 0.7 + 0.3
    x = (torch.rand(n, generator=g) - 0.5) * 0.6 * z * W / fx
    y = (torch.rand(n, generator=g) - 0.5) * 0.6 * z * H / fx
    means = torch.stack([x, y, z], 1).contiguous()
    # footprint variance L = (fx s / z)^2 of 1e8 .. 1e9: the range in which a*c and b*b round to the same float
    L = 10.0 ** (8.0 + torch.rand(n, generator=g))
    s_long = L.sqrt() * z / fx
    scales = torch.stack([s_long, torch.full((n,), 1e-4), torch.full((n,), 1e-4)], 1).contiguous()
    phi = torch.rand(n, generator=g) * math.pi
    rot = torch.stack([torch.cos(phi / 2), torch.zeros(n), torch.zeros(n), torch.sin(phi / 2)], 1).contiguous()
    O.TILE, O.BWD_MODE, O.FLAGS = TILE, _abi.BWD_REFERENCE, 0
    try:
        r = O.rasterize_gaussians(torch.zeros(3), means, torch.zeros(n, 3), torch.full((n, 1), 0.5), scales, rot, 1.0,
                                  torch.empty(0), cam.world_view_transform, cam.full_proj_transform, cam.projection_matrix,
                                  cam.tanfovx, cam.tanfovy, H, W, torch.empty(0), 0, cam.camera_center, False, False)
        radii, geom = r[2], r[3]
        O.release(geom)
    finally:
        O.TILE = 15
    return means, scales, rot, radii == 0


def _one_zero_det():
    W, H = 47, 31
    s = scene2(110, W, H, 3, seed=41)
    means, scales, rot, zero = _needle_candidates(W, H)
    zi = zero.nonzero().flatten().tolist()
    assert len(zi) >= 2 * N_ONE + N_BOTH, f"only {len(zi)} of {N_CAND} candidate needles have a zero determinant"
    nz = (~zero).nonzero().flatten().tolist()[:4]  # a few ordinary needles (det > 0) ride along
    rows = iter(range(s["means3D"].shape[0]))
    round_scale = torch.full((3,), 0.02)
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0])
    for n, c in enumerate(zi[: 2 * N_ONE + N_BOTH] + nz):
        i = next(rows)
        s["means3D"][i] = means[c]
        first = n < N_ONE or n >= 2 * N_ONE   # set 1 is the needle
        second = n >= N_ONE                    # set 2 is the needle (from 2 N_ONE on: both)
        if c in nz:
            first, second = n % 2 == 0, n % 2 == 1
        for sfx, needle in (("", first), ("_lang", second)):
            s["scales" + sfx][i] = scales[c] if needle else round_scale
            s["rotations" + sfx] = s["rotations" + sfx].clone()
            s["rotations" + sfx][i] = rot[c] if needle else ident
    return s


SCENES = {
    "dense": _dense,
    "ragged": lambda: scene2(600, 47, 31, 3, seed=3),
    "border": lambda: scene2(400, 47, 31, 3, seed=12, border=True, large=0.3),
    "sh_2_3": lambda: _sh(2, 3),
    "sh_3_3": lambda: _sh(3, 3),
    "colors_precomp": lambda: _colors(_base()),
    "cov3D_precomp": lambda: _precomp(_base(), ""),
    "cov3D_precomp_lang": lambda: _precomp(_base(), "_lang"),
    "both_precomp": lambda: _precomp(_base(), "", "_lang"),
    "scale_modifier_1.7": lambda: dict(_base(), scale_modifier=1.7),
    "background": lambda: _base(bg=torch.tensor([0.3, 0.6, 0.1])),
    "rotated_camera": lambda: _base(camera=default_camera(47, 31, yaw_deg=9, tx=0.2), max_sh_degree=2),
    "F15": lambda: _base(F=15),
    "single": lambda: _base(1, seed=2),
    "all_culled": _all_culled,
    "no_depth_cotangent": _base,
    "language_only": _base,
    "one_zero_det": _one_zero_det,
}
# what the GPU file runs against the build (one_zero_det: DESIGN.md section 0 row f4 states where the product differs)
GPU_SCENES = tuple(n for n in SCENES if n != "one_zero_det")


@functools.lru_cache(maxsize=None)
def spec(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def cotangents(name):
    """(dL_dcolor, dL_dlanguage, dL_ddepth or None)."""
    s = spec(name)
    cam = s["camera"]
    H, W, F = cam.height, cam.width, s["language"].shape[1]
    g = torch.Generator().manual_seed(99 + SEED)
    n = float(H * W)
    dc, dl, dd = (torch.randn(c, H, W, generator=g) / n for c in (3, F, 1))
    if name == "no_depth_cotangent":
        dd = None
    if name == "language_only":
        dc, dd = torch.zeros_like(dc), torch.zeros_like(dd)
    return dc, dl, dd


@functools.lru_cache(maxsize=None)
def ref_run(name):
    """(forward dict of the DGR-D build with the state fields under "fields", every gradient of its backward)."""
    from oracle import oracle_ref_dgrd as Rd
    s = spec(name)
    fwd = Rd.forward(s)
    fwd["fields"] = {k: Rd.get_field(fwd, k) for k in Rd.STATE_FIELDS}
    return fwd, Rd.backward_all(s, fwd, *cotangents(name))


@functools.lru_cache(maxsize=None)
def oracle_run(name, variant="default", mode=_abi.BWD_REFERENCE):
    """The same through the restatement tests/dgrd_oracle.py: (outputs, state fields, gradients, saved)."""
    import dgrd_oracle as D
    import ref_scenes
    s = spec(name)
    out, saved = D.forward(s, O=ref_scenes.oracle_module(variant))
    return out, D.state(saved), D.backward_all(s, saved, *cotangents(name), mode=mode), saved


def _per_pixel(fwd, sfx, W, H):
    """Per pixel of one set, from the build's own state: list length, and whether the pixel certainly saturated before
    its list ended / certainly walked it to the end.  A pixel stops when T (1 - alpha) < 1e-4 and keeps T from before
    that entry: with final_T > 0.01 no alpha <= 0.99 can have stopped it; it stopped early if the first blendable entry
    after its last contributor, which is not the list's last, takes final_T below 1e-4 (evaluated in float64, with a
    margin of 10 %)."""
    f = fwd["fields"]
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rg = f["ranges" + sfx].view(-1, 2).long()
    pl = f["point_list" + sfx].long()
    xy = f["means2D"].view(-1, 2).double()
    co = f["conic_opacity" + sfx].view(-1, 4).double()
    nc = f["n_contrib" + sfx].view(H, W).long()
    fT = f["final_T" + sfx].view(H, W).double()
    length = torch.zeros(H, W, dtype=torch.long)
    early = torch.zeros(H, W, dtype=torch.bool)
    for t in range(gx * gy):
        x0, y0 = (t % gx) * TILE, (t // gx) * TILE
        ys, xs = torch.meshgrid(torch.arange(y0, min(y0 + TILE, H)), torch.arange(x0, min(x0 + TILE, W)), indexing="ij")
        ids = pl[rg[t, 0]:rg[t, 1]]
        n = ids.numel()
        length[ys, xs] = n
        if n == 0:
            continue
        dx = xy[ids, 0][None, None, :] - xs[..., None].double()
        dy = xy[ids, 1][None, None, :] - ys[..., None].double()
        c = co[ids]
        power = -0.5 * (c[:, 0] * dx * dx + c[:, 2] * dy * dy) - c[:, 1] * dx * dy
        alpha = torch.minimum(torch.tensor(0.99, dtype=torch.float64), c[:, 3] * torch.exp(power))
        blend = (power <= 0) & (alpha >= 1.0 / 255.0)
        pos = torch.arange(n)[None, None, :]
        after = blend & (pos >= nc[ys, xs][..., None]) & (pos < n - 1)
        first = torch.where(after, pos, n).min(dim=-1).values
        has = first < n
        a_first = torch.gather(alpha, 2, first.clamp(max=n - 1)[..., None])[..., 0]
        early[ys, xs] = has & (fT[ys, xs] * (1.0 - a_first) < 0.9e-4)
    walked = (length > 0) & (fT > 0.01)
    return length, early, walked


def measure(name):
    """The measured values behind a scene's conditions, from the DGR-D build's own output."""
    s = spec(name)
    fwd, _ = ref_run(name)
    cam = s["camera"]
    W, H = cam.width, cam.height
    f = fwd["fields"]
    r1, r2 = fwd["radii"], fwd["radii_lang"]
    t1, t2 = f["tiles_touched"], f["tiles_touched_lang"]
    m = dict(P=s["means3D"].shape[0], R=fwd["R"], R_lang=fwd["R_lang"], visible=int(((r1 > 0) | (r2 > 0)).sum()),
             clamped=int(f["clamped"].sum()), partial_x=W % TILE, partial_y=H % TILE,
             only_set2_square=int(((r1 > 0) & (t1 == 0) & (t2 > 0)).sum()),
             only_set1_square=int(((r2 > 0) & (t2 == 0) & (t1 > 0)).sum()))
    for sfx in ("", "_lang"):
        rg = f["ranges" + sfx].view(-1, 2).long()
        m["longest_range" + sfx] = int((rg[:, 1] - rg[:, 0]).max()) if rg.numel() else 0
    if name == "dense":
        _, e1, w1 = _per_pixel(fwd, "", W, H)
        _, e2, w2 = _per_pixel(fwd, "_lang", W, H)
        m["early_1_walked_2"] = int((e1 & w2).sum())
        m["walked_1_early_2"] = int((w1 & e2).sum())
    if name == "one_zero_det":
        bad1 = ~torch.isfinite(f["conic_opacity"].view(-1, 4)[:, :3]).all(1)
        bad2 = ~torch.isfinite(f["conic_opacity_lang"].view(-1, 4)[:, :3]).all(1)
        m["nonfinite_conic_1_only"] = int((bad1 & ~bad2).sum())
        m["nonfinite_conic_2_only"] = int((bad2 & ~bad1).sum())
        # both determinants zero: preprocess returns before it writes anything (radii 0 inside the frustum)
        n = 2 * N_ONE + N_BOTH
        m["both_zero_early_return"] = int(((r1[:n] == 0) & (r2[:n] == 0)).sum())
    return m


def conditions(name):
    """Asserts the scene's conditions and returns the measured values."""
    m = measure(name)
    if name == "dense":
        assert m["longest_range"] > TILE * TILE and m["longest_range_lang"] > TILE * TILE, m
        assert m["early_1_walked_2"] + m["walked_1_early_2"] >= 1, m
    elif name in ("ragged", "border"):
        assert m["partial_x"] != 0 and m["partial_y"] != 0, m
    if name == "border":
        assert m["only_set2_square"] >= 1 and m["only_set1_square"] >= 1, m
    elif name.startswith("sh_"):
        assert m["clamped"] >= 1, m
    elif name == "single":
        assert m["P"] == 1 and m["R"] >= 1, m
    elif name == "all_culled":
        assert m["R"] == 0 and m["R_lang"] == 0 and m["visible"] == 0, m
    elif name == "one_zero_det":
        assert m["nonfinite_conic_1_only"] >= 2 and m["nonfinite_conic_2_only"] >= 2, m
        assert m["both_zero_early_return"] >= 1, m
    if name != "all_culled":
        assert m["R"] > 0 and m["R_lang"] > 0, m
    return m
