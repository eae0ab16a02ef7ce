"""The aimed families of tests/tile_cull_scenes.py and the float64 model of tests/tile_cull_ref.py, proved on the oracle alone
(no GPU).  With `record` the (Gaussian, tile) pairs whose list entry some pixel of the oracle's composite blended and `rect`
the pairs of the oracle's own lists, every family and both tile edges must give

    record  <=  core  <=  may  <=  rect                    (sets of pairs)

with may sharp: |may \\ core| <= 1 % of |may| per family - a condition on the families' inputs, not a measurement - and every
family must hit what it aims at.  tests/test_gpu_tile_cull.py then holds the HIP lists between core and may.
"""
import numpy as np
import pytest

import tile_cull_ref as ref
import tile_cull_scenes as cs

CASES = [(name, tile) for name in cs.FAMILIES for tile in cs.TILES]
SHARPNESS = 0.01


def _ids(c):
    return f"{c[0]}_t{c[1]}"


@pytest.fixture(params=CASES, ids=_ids)
def case(request, oracle):
    name, tile = request.param
    return cs.make(name, tile), cs.reference(name, tile)


def _has(keys, tile, g, P):
    return np.isin(np.asarray(tile, dtype=np.int64) * P + np.asarray(g, dtype=np.int64), keys)


def test_chain_and_sharpness(case):
    fam, r = case
    m = r["model"]
    assert np.array_equal(m.rect, r["rect"]), "get_rect restated: the model's rect is not the oracle's lists"
    assert ref.is_subset(r["record"], m.core), f"record is not inside core: {np.setdiff1d(r['record'], m.core)[:5]}"
    assert ref.is_subset(m.core, m.may)
    assert ref.is_subset(m.may, m.rect)
    band = m.may.size - m.core.size
    share = band / max(m.may.size, 1)
    print(f"{fam.name} tile {fam.tile}: P={fam.scene.P} rect={m.rect.size} may={m.may.size} core={m.core.size} "
          f"record={r['record'].size} full={int(m.full.sum())} none={int(m.none.sum())} "
          f"band share |may - core| / |may| = {100.0 * share:.3f} %  p max = {m.p.max():.4f}")
    assert m.may.size > 0 and m.core.size > 0
    assert share <= SHARPNESS, f"may is not sharp on this family: {100.0 * share:.3f} %"


def test_core_is_the_pixel_column_minimum(case):
    """The other closed form: a pair of the rect is in core exactly when some integer pixel column of the tile (<= W - 1) has
    min over the band of q <= t2 (min_q_box on a box one column wide)."""
    fam, r = case
    m, pre, T, P = r["model"], r["pre"], fam.tile, fam.scene.P
    tile, g = ref.split_key(m.rect, P)
    sel = ~m.full[g] & ~m.none[g]
    tile, g = tile[sel], g[sel]
    tx, ty = tile % m.gx, tile // m.gx
    co, mm = pre.conic_opacity.astype(np.float64), pre.means2D.astype(np.float64)
    Y0, Y1 = (ty * T).astype(np.float64), np.minimum(ty * T + T - 1, fam.H - 1).astype(np.float64)
    best = np.full(g.shape, np.inf)
    for k in range(T):
        col = (tx * T + k).astype(np.float64)
        q = ref.min_q_box(mm[g, 0], mm[g, 1], co[g, 0], co[g, 1], co[g, 2], col, col, Y0, Y1)
        best = np.minimum(best, np.where(col <= fam.W - 1, q, np.inf))
    in_core = np.isin(tile * P + g, m.core)
    t2 = m.t2[g]
    assert bool(in_core[best <= t2 * (1 - 1e-9)].all()), "a tile whose pixel column reaches inside the contour is not in core"
    assert bool((best[in_core] <= t2[in_core] * (1 + 1e-9)).all()), "core holds a tile that no pixel column reaches"


def test_family_hits_its_target(case):
    fam, r = case
    m, info, P = r["model"], fam.info, fam.scene.P
    g = np.arange(P)
    if fam.name in ("graze", "extreme", "far"):
        aimed = _has(r["record"], info["aimed_tile"], g, P)
        pos, neg = info["eps"] > 0, info["eps"] < 0
        if fam.name == "far":
            neg = neg & (info["sense"] > 0)          # (a splat that covers all but the corner blends the tile's other pixels)
        hit, miss = aimed[pos].mean(), (~aimed[neg]).mean()
        print(f"{fam.name} tile {fam.tile}: aimed pair recorded for {100 * hit:.1f} % of the positive margins, absent for "
              f"{100 * miss:.1f} % of the negative ones")
        assert hit >= 0.95 and miss >= 0.95
    if fam.name == "graze":
        # every margin below the kernel's own (2e-3 in the logarithm) is inside core
        small = np.abs(info["eps"]) <= 1e-4
        assert _has(m.core, info["aimed_tile"], g, P)[small].all()
    if fam.name == "gap":
        rows_rect = np.bincount(m.row_g, weights=(m.row_rect[:, 1] > m.row_rect[:, 0]), minlength=P)
        rows_may = np.bincount(m.row_g, weights=(m.row_may[:, 1] > m.row_may[:, 0]), minlength=P)
        assert (rows_rect > rows_may).mean() >= 0.5
        n_may = np.bincount(ref.split_key(m.may, P)[1], minlength=P)
        n_core = np.bincount(ref.split_key(m.core, P)[1], minlength=P)
        thin = info["half"] <= 0.45
        assert (n_may[thin] == 0).all(), "a needle that fits between two pixel lines reaches a tile"
        assert (n_core[~thin] >= 2).all(), "a needle wider than the gap misses one of its two sides"
    if fam.name == "extreme":
        row = (m.row_g[:, None] == g[None, :]) & (m.row_ty[:, None] == (info["aimed_tile"] // m.gx)[None, :])
        star = (row & m.star_only[:, None]).any(axis=0)
        near = (np.abs(info["eps"]) <= 1e-4) & np.isnan(info["core_px"])
        in_core, in_may = _has(m.core, info["aimed_tile"], g, P), _has(m.may, info["aimed_tile"], g, P)
        print(f"extreme tile {fam.tile}: span through the star point alone for {int(star.sum())} of {P}")
        assert star[in_may].all(), "the aimed row has a band edge inside the contour"
        assert in_core[near].all() and in_core[info["eps"] > 0].all() and not in_may[info["eps"] <= -1e-2].any()
        assert in_core[info["core_px"] > 0].all() and not in_may[info["core_px"] < 0].any()
    if fam.name == "border":
        far_edge = info["past_far_edge"]
        assert far_edge.sum() >= 50
        assert _has(m.rect, info["aimed_tile"][far_edge], g[far_edge], P).all()
        assert not _has(m.may, info["aimed_tile"][far_edge], g[far_edge], P).any()
        outside = (info["beyond"] > 0) & (info["aimed_tile"] < 0)      # contours that end before pixel line 0
        assert np.bincount(ref.split_key(m.may, P)[1], minlength=P)[outside].sum() == 0
    if fam.name == "floor":
        n_core = np.bincount(ref.split_key(m.core, P)[1], minlength=P)
        n_may = np.bincount(ref.split_key(m.may, P)[1], minlength=P)
        assert (n_core[~info["on_corner"]] == 1).all() and (n_may[info["on_corner"]] == 0).all()
        rec = np.bincount(ref.split_key(r["record"], P)[1], minlength=P)
        assert rec[~info["on_corner"] & (info["o255"] >= 1.0 + 2.0 ** -22)].all() and not rec[info["o255"] < 1.0 - 2.0 ** -22].any()
    if fam.name == "gate":
        pre = r["pre"]
        co = pre.conic_opacity.astype(np.float64)
        det = co[:, 0] * co[:, 2] - co[:, 1] ** 2
        vis = pre.radii > 0
        reasons = dict(det=int((vis & m.full & ~(det > 0)).sum()), t2=int((vis & m.full & ~(m.t2 < 1e6)).sum()),
                       radius=int((vis & m.full & (pre.radii >= (1 << 20))).sum()), exact=int((vis & ~m.full).sum()))
        print(f"gate tile {fam.tile}: {reasons}")
        assert reasons["det"] >= 10 and reasons["exact"] >= 50
        tile, gg = ref.split_key(m.rect, P)
        assert np.array_equal(m.core[np.isin(ref.split_key(m.core, P)[1], np.nonzero(m.full)[0])], m.rect[m.full[gg]])
