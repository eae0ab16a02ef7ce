"""The HIP rasteriser on non-finite and overflowing Gaussians (tests/nonfinite_scenes.py), pinned to the oracle.

Every scene of the module runs at its tile size — the 45 x 30 mixtures and boundary classes at both — in both binning modes
and both backward modes, against the oracle as it stands ("Non-finite inputs").

a  forward == oracle by bits (NaN where it has NaN): images, final_T, radii, n_touched; with the reference's binning also
   num_rendered, the sorted list and n_contrib; the exact binning keeps every pair that blends;
b  containment: a scene whose planted rows are all culled renders and differentiates like the scene without those rows,
   and pixels outside the planted rows' tiles keep the unplanted frame's bits;
c  backward: rows the oracle has finite and that are not planted meet the per-element criterion of tests/test_gpu_parity.py;
   every element of a planted row is of the oracle's class (finite / NaN / +inf / -inf) and, where finite, meets it too; the set
   of rows that turn non-finite equals the oracle's in BWD_EXACT and is a subset of it in BWD_REFERENCE (the fast composite
   skips recursion-only visits), with the one further deviation test_backward_row_by_row states; the
   ordered kernel equals the oracle's composite-level gradients by bits;
d  the raw-parameter path (all OLSR_ACT_* flags) equals the activations = 0 frame of olsr_debug_activate's values;
e  every depth-sort path gives one list on NaN depths of both signs and an infinite one, and a carried depth order changes
   nothing when rows turn NaN between two frames;
f  the feature classes are forward-only here: their non-finite pixels are exactly the oracle's (part of a).
tests/test_gpu_extents.py runs the mixture scene between guards."""
import pytest
import torch

import nonfinite_scenes as N
from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.scene import Scene
from parity_common import (COMPOSITE_KEYS, assert_elementwise, assert_ordered_equals_oracle, ordered_backward, run_backend,
                           same_bits)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = N.module_scenes()
IDS = [r[0] for r in ROWS]
MODES = (_abi.BWD_REFERENCE, _abi.BWD_EXACT)
BINNINGS = (_abi.BINNING_RECT, _abi.BINNING_ELLIPSE)
SEED = 3
RTOL = 1e-4                    # tests/test_gpu_parity.py: RTOL
COMPOSITE_WORST = 2e-4         # ... _check's composite_worst_bound
_CACHE = {}


def _device_activated(p, which="scene"):
    """Raw kinds: the scene with olsr_debug_activate's values (the device's own expf) in place of the raw arrays."""
    sc = getattr(p, which)
    if not p.raw:
        return sc
    from online_lang_splatting_amd import _lib
    op, s, q = _lib.debug_activate(_abi.ACT_ALL, *(t.to(DEV).contiguous() for t in (sc.opacities, sc.scales, sc.rotations)))
    return Scene(sc.camera, sc.means3D, op.cpu(), s.cpu(), q.cpu(), sc.shs, sc.language, sc.sh_degree, sc.bg, sc.F)


def _runs(hip, oracle, row, mode):
    """Oracle and library (both binnings) on one scene and backward mode, once."""
    key = (row[0], mode)
    if key not in _CACHE:
        p = N.scene_of(row)
        tile, sc = row[5], _device_activated(p)
        fo, go = run_backend(oracle, sc, None, SEED, tile, mode, **p.kw)
        for k in ("point_list", "n_contrib", "final_T"):
            fo[k] = oracle.get_field(fo["geom"], k)
        oracle.release(fo["geom"])
        hip_runs = {b: run_backend(hip, sc, torch.device(DEV), SEED, tile, mode, binning=b, **p.kw) for b in BINNINGS}
        torch.cuda.synchronize()
        _CACHE[key] = (p, sc, fo, go, hip_runs)
    return _CACHE[key]


def _field(hip, f, sc, tile, kind, name, dtype, count):
    hip.TILE = tile
    W, H = sc.camera.width, sc.camera.height
    return hip.state_field(kind, f[kind if kind != "image" else "img"], name, P=sc.P, F=sc.F, R=f["R"], W=W, H=H, dtype=dtype,
                           count=count).cpu()


# ------------------------------------------------------------------------------------------------ a, f: the forward
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_forward_equals_the_oracle(hip, oracle, row):
    import test_gpu_parity as TP
    p, sc, fo, go, runs = _runs(hip, oracle, row, _abi.BWD_REFERENCE)
    tile, W, H = row[5], row[3], row[4]
    for b, (f, _g) in runs.items():
        name = f"{row[0]} binning {b}"
        assert torch.equal(f["radii"].cpu(), fo["radii"]) and torch.equal(f["n_touched"].cpu(), fo["n_touched"]), name
        for k in ("color", "language", "depth", "opacity"):
            if fo[k] is not None and fo[k].numel():
                assert same_bits(f[k], fo[k]), f"{name}: forward {k}"
                # (f) the non-finite pixels are exactly the oracle's
                assert torch.equal(torch.isfinite(f[k].cpu()), torch.isfinite(fo[k])), f"{name}: non-finite pixels of {k}"
        assert same_bits(_field(hip, f, sc, tile, "image", "final_T", torch.float32, W * H), fo["final_T"]), name
    fr, fe = runs[_abi.BINNING_RECT][0], runs[_abi.BINNING_ELLIPSE][0]
    assert fr["R"] == fo["R"] and fe["R"] <= fo["R"]
    if fo["R"] > 0:
        assert torch.equal(_field(hip, fr, sc, tile, "binning", "point_list", torch.int32, fr["R"]), fo["point_list"])
        assert torch.equal(_field(hip, fr, sc, tile, "image", "n_contrib", torch.int32, W * H), fo["n_contrib"])
        # the exact lists: an order-preserving sub-list of the reference's that keeps every blending instance
        kr, flr, _ = TP._tile_pairs(hip, fr, sc, tile)
        if fe["R"] > 0:
            ke, fle, _ = TP._tile_pairs(hip, fe, sc, tile)
            keep = torch.isin(kr, ke)
            assert int(keep.sum()) == ke.numel() and torch.equal(kr[keep], ke) and torch.equal(flr[keep], fle)
        else:
            keep = torch.zeros_like(kr, dtype=torch.bool)
        assert int((flr[~keep] != 0).sum()) == 0, "the exact binning dropped an instance that blends"


# ------------------------------------------------------------------------------------------------ b: containment
def _surviving(t, keep):
    return t.reshape(keep.numel(), -1)[keep.to(t.device)]


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_planting_is_contained(hip, oracle, row):
    p, sc, fo, go, runs = _runs(hip, oracle, row, _abi.BWD_REFERENCE)
    tile, W, H = row[5], row[3], row[4]
    dev = torch.device(DEV)
    base_sc = _device_activated(p, "base")
    planted_out = N.oracle_forward(sc, tile, **p.kw)
    base_out = N.oracle_forward(base_sc, tile, **p.base_kw)
    tiles = N.planted_tiles(planted_out, p.idx, sc.P) | N.planted_tiles(base_out, p.idx, sc.P)
    outside = ~N.pixel_mask_of_tiles(tiles, W, H, tile)
    all_culled = bool((fo["radii"][p.idx] == 0).all()) and int(p.idx.numel()) < sc.P
    for b in BINNINGS:
        f, g = runs[b]
        fb, _ = run_backend(hip, base_sc, dev, SEED, tile, _abi.BWD_REFERENCE, binning=b, **p.base_kw)
        for k in ("color", "language", "depth", "opacity"):
            if fo[k] is not None and fo[k].numel():
                assert same_bits(f[k].cpu()[:, outside], fb[k].cpu()[:, outside]), (row[0], b, k)
        if not all_culled:
            continue
        # every planted row is culled: the frame and the gradients of the scene without those rows.  (The cotangents depend
        # on the frame alone, not on P; the deleted rows' gradients are zero.)
        cut, cut_kw, keep = p.deleted()
        if p.raw:
            cut = _device_activated(N.Planted(p.kind, cut, cut, p.idx, p.kinds, raw=True))
        fd, gd = run_backend(hip, cut, dev, SEED, tile, _abi.BWD_REFERENCE, binning=b, **cut_kw)
        for k in ("color", "language", "depth", "opacity"):
            if fo[k] is not None and fo[k].numel():
                assert same_bits(f[k], fd[k]), (row[0], b, k)
        assert torch.equal(f["radii"].cpu()[keep], fd["radii"].cpu()) and torch.equal(f["n_touched"].cpu()[keep], fd["n_touched"].cpu())
        assert f["R"] == fd["R"]
        for k in gd:
            if gd[k].numel() and k in g and g[k].shape[0] == sc.P:
                assert_elementwise(_surviving(g[k], keep), gd[k].reshape(int(keep.sum()), -1), f"{row[0]}:{b}:{k}", COMPOSITE_WORST)
                assert float(_surviving(g[k], ~keep).abs().max()) == 0, (row[0], b, k)


# ------------------------------------------------------------------------------------------------ c: the backward
def _class_of(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf."""
    t = t.detach().cpu().float()
    return t.isnan().long() + 2 * (t == float("inf")).long() + 3 * (t == float("-inf")).long()


@pytest.mark.parametrize("mode", MODES, ids=["reference", "exact"])
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_backward_row_by_row(hip, oracle, row, mode):
    """One deviation is asserted as what it is: a Gaussian no pixel blended has no partial-gradient row
    and skips the per-Gaussian chain — exact zeros where the reference's chain multiplies a zero by its NaN covariance.
    Rows planted with a feature class are forward-only: their own elements are not class-checked, every other statement
    holds for them and for the scenes that contain them."""
    p, sc, fo, go, runs = _runs(hip, oracle, row, mode)
    P = sc.P
    planted = torch.zeros(P, dtype=torch.bool)
    planted[p.idx] = True
    checked = planted.clone()   # planted rows whose elements are class-checked: all but the feature classes'
    for i, k in zip(p.idx.tolist(), p.kinds):
        if k in N.FORWARD_ONLY:
            checked[i] = False
    rowless = torch.ones(P, dtype=torch.bool)   # the oracle's composite-level gradients of the row are all exact zeros
    for k in COMPOSITE_KEYS:
        if go[k].numel():
            rowless &= (go[k].reshape(P, -1) == 0).all(1)
    for b, (f, g) in runs.items():
        for k in go:
            if not go[k].numel() or k not in g:
                continue
            name = f"{row[0]}:mode {mode}:binning {b}:{k}"
            want, got = go[k].reshape(P, -1).clone(), g[k].detach().cpu().float().reshape(P, -1)
            got_bad = (~torch.isfinite(got)).any(1)
            if k not in COMPOSITE_KEYS:
                zeroed = rowless & (~torch.isfinite(want)).any(1) & ~got_bad
                assert bool((got[zeroed] == 0).all()), f"{name}: a row without partial gradients is neither the oracle's nor zero"
                want[zeroed] = 0.0
            want_bad = (~torch.isfinite(want)).any(1)
            extra, missing = got_bad & ~want_bad, want_bad & ~got_bad
            # rows made non-finite: the oracle's set; in the reference mode a subset of it
            assert not bool(extra.any()), (f"{name}: rows {extra.nonzero().reshape(-1).tolist()} are non-finite here and finite in "
                                           f"the oracle ({int(extra.sum())} of {P}; the oracle has {int(want_bad.sum())} non-finite)")
            if mode == _abi.BWD_EXACT:
                assert not bool(missing.any()), f"{name}: rows {missing.nonzero().reshape(-1).tolist()} are finite here, not in the oracle"
            # untouched rows: finite in the oracle, not planted — the criterion of tests/test_gpu_parity.py on those rows only
            rows = ~want_bad & ~planted & ~got_bad
            if bool(rows.any()):
                a_, b_ = got[rows].double(), want[rows].double()
                scale = float(b_.abs().max())
                err = float((a_ - b_).abs().max())
                assert err <= RTOL * (scale + 1e-30), f"{name}: max-norm rel {err / (scale + 1e-30):.2e}"
                if k in COMPOSITE_KEYS:
                    assert_elementwise(got[rows], want[rows], name, COMPOSITE_WORST)
            # planted rows: every element of the oracle's class, and where finite within the same criterion
            if not bool(checked.any()):
                continue
            cw, cg = _class_of(want[checked]), _class_of(got[checked])
            if mode == _abi.BWD_EXACT:
                assert torch.equal(cw, cg), f"{name}: planted rows: classes {cg.tolist()} vs the oracle's {cw.tolist()}"
            else:
                assert bool(((cw == cg) | (cg == 0)).all()), f"{name}: planted rows: classes {cg.tolist()} vs {cw.tolist()}"
            fin = (cw == 0) & (cg == 0)
            if bool(fin.any()):
                finite_scale = float(want[torch.isfinite(want)].abs().max()) if bool(torch.isfinite(want).any()) else 0.0
                d = (got[checked][fin].double() - want[checked][fin].double()).abs()
                tol = RTOL * want[checked][fin].double().abs() + 1e-6 * finite_scale
                assert bool((d <= tol).all()), f"{name}: planted rows: finite elements off by up to {float((d / (tol + 1e-300)).max()):.2f} tolerances"


@pytest.mark.parametrize("row", [r for r in ROWS if r[1] in N.GEOMETRY_AND_OPACITY], ids=lambda r: r[0])
def test_ordered_backward_equals_the_oracle(hip, oracle, row):
    """olsr_debug_backward_ordered, the reference's association on the GPU, on the geometry and opacity classes."""
    for mode in MODES:
        p, sc, fo, go, runs = _runs(hip, oracle, row, mode)
        if sc.P == 0 or fo["R"] == 0:
            continue
        for b, (f, _g) in runs.items():
            if f["R"] == 0:
                continue
            gord = ordered_backward(hip, sc, f, SEED, row[5], mode, **p.kw)
            assert_ordered_equals_oracle(go, gord, where=f"{row[0]}:mode {mode}:binning {b}:ordered:")


# ------------------------------------------------------------------------------------------------ d: the raw-parameter path
def _cam(c, dev):
    return dict(viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev),
                projmatrix_raw=c.projection_matrix.to(dev), campos=c.camera_center.to(dev), tanfovx=c.tanfovx, tanfovy=c.tanfovy)


def _workspace_frame(hip, ws, sc, act, tile, extra=None):
    """One forward on a RasterWorkspace: images, R, final_T, n_contrib and the sorted list."""
    dev = torch.device(DEV)
    W, H = sc.camera.width, sc.camera.height
    ws.set_scene(bg=sc.bg.to(dev), means3D=sc.means3D.to(dev).contiguous(), shs=sc.shs.to(dev), sh_degree=sc.sh_degree,
                 language=sc.language.to(dev) if sc.F else None, opacities=sc.opacities.to(dev).contiguous(),
                 scales=sc.scales.to(dev).contiguous(), rotations=sc.rotations.to(dev).contiguous(), activations=act,
                 **_cam(sc.camera, dev))
    out = {k: v.clone() for k, v in ws.forward().items()}
    R, overflow = ws.rendered()
    assert not overflow
    hip.TILE = tile
    out["R"] = R
    out["final_T"] = hip.state_field("image", ws.img, "final_T", W=W, H=H, dtype=torch.float32, count=W * H).clone()
    out["n_contrib"] = hip.state_field("image", ws.img, "n_contrib", W=W, H=H, dtype=torch.int32, count=W * H).clone()
    out["point_list"] = (hip.state_field("binning", ws.binning, "point_list", R=ws.capacity, F=ws.F, dtype=torch.int32, count=R).clone()
                         if R else torch.empty(0, dtype=torch.int32))
    return out


def _same_frame(a, b, where):
    assert a["R"] == b["R"], where
    for k in a:
        if k != "R" and a[k] is not None:
            assert same_bits(a[k], b[k]), (where, k)


@pytest.mark.parametrize("binning", BINNINGS, ids=["rect", "ellipse"])
@pytest.mark.parametrize("row", [r for r in ROWS if r[1] in N.KINDS and N.KINDS[r[1]][1] == "raw"], ids=lambda r: r[0])
def test_raw_parameter_path_equals_the_activated_frame(hip, row, binning):
    """All OLSR_ACT_* flags on the raw arrays == activations = 0 on olsr_debug_activate's values: tests/test_gpu_activations.py's
    equality, on log-scales whose exp overflows or underflows, logits whose sigmoid is exactly 0 or 1, and NaNs."""
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    p = N.scene_of(row)
    tile, sc = row[5], p.scene
    ws = RasterWorkspace(sc.P, row[3], row[4], sc.F, sc.shs.shape[1], 1 << 16, torch.device(DEV), binning=binning, tile=tile)
    fused = _workspace_frame(hip, ws, sc, _abi.ACT_ALL, tile)
    unfused = _workspace_frame(hip, ws, _device_activated(p), 0, tile)
    again = _workspace_frame(hip, ws, sc, _abi.ACT_ALL, tile)
    _same_frame(fused, unfused, f"{row[0]} fused vs un-fused")
    _same_frame(again, fused, f"{row[0]} fused again")


# ------------------------------------------------------------------------------------------------ e: sort and carry
def _mixture():
    return [r for r in ROWS if r[1] == "mix_all" and r[5] == 15][0]


def test_every_depth_sort_path_gives_one_list(hip, oracle):
    """NaN depths of both signs (keys 0x7FC00000 and 0xFFC00000, above every real depth) and an infinite depth among the
    keys: the one-launch sort, the radix passes and the passes over every Gaussian give the oracle's list."""
    from test_gpu_extents import _forced
    row = _mixture()
    p = N.scene_of(row)
    assert {"mean_nan_x", "mean_negnan_z", "mean_inf_z"} <= set(p.kinds)
    _p, sc, fo, _go, _runs_ = _runs(hip, oracle, row, _abi.BWD_REFERENCE)
    lists = {}

    def run(name, knobs):
        def body(L):
            knobs(L)
            f, _ = run_backend(hip, sc, torch.device(DEV), SEED, row[5], _abi.BWD_REFERENCE, binning=_abi.BINNING_RECT)
            lists[name] = _field(hip, f, sc, row[5], "binning", "point_list", torch.int32, f["R"])
        _forced(body)
    run("one_launch", lambda L: None)
    run("small_off", lambda L: L.olsr_debug_sort_small(0))
    run("compact_off", lambda L: (L.olsr_debug_sort_small(0), L.olsr_debug_sort_compact(0)))
    for name, pl in lists.items():
        assert torch.equal(pl, fo["point_list"]), name


def test_carried_depth_order_when_rows_turn_nan(hip):
    """Two frames through a RasterWorkspace with the order carry on; the planted rows turn NaN between the frames.  The second
    frame's lists and images equal those of a fresh workspace."""
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    row = _mixture()
    p = N.scene_of(row)
    tile, dev = row[5], torch.device(DEV)
    mk = lambda **kw: RasterWorkspace(p.scene.P, row[3], row[4], p.scene.F, p.scene.shs.shape[1], 1 << 16, dev, tile=tile, **kw)  # noqa: E731
    carry, fresh = mk(carry_order=True), mk()
    first = _workspace_frame(hip, carry, p.base, 0, tile)
    assert first["R"] > 0
    second = _workspace_frame(hip, carry, p.scene, 0, tile)
    want = _workspace_frame(hip, fresh, p.scene, 0, tile)
    _same_frame(second, want, "carried order, rows turned NaN")
    third = _workspace_frame(hip, carry, p.scene, 0, tile)   # and the order it left behind serves the next frame
    _same_frame(third, want, "carried order, NaN rows again")
