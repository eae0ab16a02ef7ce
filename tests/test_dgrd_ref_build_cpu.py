"""The restatement of the disentangled rasteriser against DGR-D's own kernel source.  No GPU needed.

tests/dgrd_oracle.py restates DGR-D (submodules/diff-gaussian-rasterization-disentangle-optim) as two passes of the plain
oracle plus a radius rule.  Here that restatement is held to the thing it restates: DGR-D's forward.cu, backward.cu and
rasterizer_impl.cu, compiled unmodified as host C++ over the execution model of oracle/ref_shim/ (oracle/ref_build.py) and
driven through DGR-D's own LanguageRasterizer entry points (oracle/ref_entry_dgrd.cpp, oracle/oracle_ref_dgrd.py).  Blocks
run in ascending tile order there, which is the order of the oracle's ordered accumulation, so every comparison but one
is an equality on bits (NaN for NaN, -0 == +0):

  * forward: R and R_lang, radii, radii_lang, n_touched(_lang), the opacity images, every list (point_list, ranges,
    n_contrib, final_T of both sets) and the per-Gaussian state on the rows both sides write.  DGR-D writes both sets'
    rows of a Gaussian as soon as ONE square covers a tile; a pass of the restatement writes the rows of its own set's
    non-empty squares.  Rows of a set whose square is empty feed no list and no gradient, and are not compared;
  * the colour, language and depth images against the restatement on liboracle_plain.so (multiply and add, what a
    contraction-off build performs): equal; against liboracle.so (fmaf): within 2 (n_contrib + 1) 2^-24 max|f| per pixel
    and channel with each set's own n_contrib;
  * backward: the 8 composite-level tensors and the 9 per-Gaussian ones.  This executes the restatement's claims: the
    language recursion is not skip-guarded, thread 0's feature gradient is the one added, set 2 yields no mean or pose
    gradient (dL_dmeans2D, dL_dmeans3D and dL_dtau equal pass 1's alone);
  * the radius rule on the border scene: disentangled._merge_radii and the restatement's torch.where on the two passes'
    signed radii reproduce the build's radii and radii_lang;
  * a guard: the restatement with the language loop skip-guarded and block-summed (the plain oracle's exact mode) is
    seen to FAIL the backward comparison on the dense scene.

Scenes and their conditions (asserted on the build's own output before anything is compared): tests/dgrd_scenes.py.
"""
import pytest
import torch

import dgrd_scenes as S
from online_lang_splatting_amd import _abi
from parity_common import first_difference

from oracle import oracle_ref_dgrd as Rd

pytestmark = pytest.mark.skipif(not Rd.available(),
                                reason="oracle/_ref holds no DGR-D build and the reference tree is absent")

NAMES = tuple(S.SCENES)
PER_SET = ("cov3D", "conic_opacity", "tiles_touched")
IMAGES = (("color", ""), ("language", "_lang"), ("depth", ""))


def _diff(a, b):
    if not a.is_floating_point():
        bad = a.reshape(-1).long() != b.reshape(-1).long()
        return f"{int(bad.sum())} of {a.numel()} integers differ, first at {int(bad.nonzero()[0])}" if bool(bad.any()) else None
    d = first_difference(a, b)
    return None if d is None else f"{d[3]} of {a.numel()} elements differ, first at {d[0]}: {d[1]!r} vs {d[2]!r}"


def _eq(a, b, what):
    assert a.numel() == b.numel(), f"{what}: {a.numel()} vs {b.numel()} elements"
    d = _diff(a, b)
    assert d is None, f"{what}: {d}"


@pytest.fixture(scope="module", params=NAMES)
def scene(request):
    """The scene's name, once its conditions hold on the DGR-D build's own output (the values go to -s output)."""
    m = S.conditions(request.param)
    print(f"\n{request.param}: {m}")
    return request.param


def test_forward_equals_restatement(scene):
    fr, _ = S.ref_run(scene)
    out, st, _, _ = S.oracle_run(scene)
    assert (fr["R"], fr["R_lang"]) == (out["R1"], out["R2"]), f"{scene}: num_rendered"
    for k in ("radii", "radii_lang", "n_touched", "n_touched_lang", "opacity", "opacity_lang"):
        _eq(fr[k], out[k], f"{scene}: {k}")
    f = fr["fields"]
    P = fr["radii"].numel()
    for sfx in ("", "_lang"):
        for k in ("point_list", "ranges", "n_contrib", "final_T"):
            _eq(f[k + sfx], st[k + sfx], f"{scene}: {k + sfx}")
        rows = f["tiles_touched" + sfx] > 0
        for k in PER_SET:
            _eq(f[k + sfx].view(P, -1)[rows], st[k + sfx].view(P, -1)[rows], f"{scene}: {k + sfx} of the set's own squares")
        # a set whose square is empty has no tile in the build either
        assert bool((st["tiles_touched" + sfx][~rows] == 0).all()), f"{scene}: tiles_touched{sfx}"
    vis = (fr["radii"] > 0) | (fr["radii_lang"] > 0)
    for k in ("means2D", "depths"):
        _eq(f[k].view(P, -1)[vis], st[k].view(P, -1)[vis], f"{scene}: {k} of the visible Gaussians")
    if S.spec(scene).get("colors_precomp") is None:
        rows = f["tiles_touched"] > 0
        for k in ("rgb", "clamped"):
            _eq(f[k].view(P, 3)[rows], st[k].view(P, 3)[rows], f"{scene}: {k}")
        # DGR-D forward.cu:398-403: an empty first square with a visible second set gets colour 0
        assert bool((f["rgb"].view(P, 3)[vis & ~rows] == 0).all()), f"{scene}: rgb of an empty first square"


def test_forward_images_equal_plain_restatement(scene):
    fr, _ = S.ref_run(scene)
    out, _, _, _ = S.oracle_run(scene, "plain_accum")
    for k, _sfx in IMAGES:
        _eq(fr[k], out[k], f"{scene}: DGR-D build vs plain-accumulation restatement: {k} image")


def image_bound(name, fwd, key, sfx):
    """[C,H,W]: 2 (n_contrib + 1) 2^-24 max|f| per pixel and channel, with the set's own n_contrib (ref_scenes.image_bound)."""
    s = S.spec(name)
    f = fwd["fields"]
    col = s.get("colors_precomp")
    feats = dict(color=col if col is not None else f["rgb"].view(-1, 3), language=s["language"],
                 depth=f["depths"].view(-1, 1))[key]
    H, W = fwd["opacity"].shape[-2:]
    n = f["n_contrib" + sfx].view(1, H, W).double()
    return 2.0 * (n + 1.0) * 2.0 ** -24 * feats.abs().max(dim=0).values.double().view(-1, 1, 1)


def test_forward_images_within_derived_bound(scene):
    fr, _ = S.ref_run(scene)
    out, _, _, _ = S.oracle_run(scene)
    for k, sfx in IMAGES:
        fin = torch.isfinite(fr[k])
        assert bool((fin == torch.isfinite(out[k])).all()), f"{scene}: {k}: non-finite pixels differ"
        bound = image_bound(scene, fr, k, sfx)
        err = (out[k].double() - fr[k].double()).abs()
        ok = (err <= bound) | ~fin
        print(f"{scene}: {k}: max |restatement - DGR-D build| {err[fin].max().item() if bool(fin.any()) else 0.0:.3e}")
        assert bool(ok.all()), f"{scene}: {k}: {int((~ok).sum())} values outside 2 (n_contrib + 1) 2^-24 max|f|"


def test_backward_equals_restatement(scene):
    _, gr = S.ref_run(scene)
    _, _, go, _ = S.oracle_run(scene)
    for k in Rd.COMPOSITE_KEYS + Rd.CHAIN_KEYS:
        _eq(gr[k], go[k], f"{scene}: backward: {k}")
    if scene != "all_culled":
        for k in ("dL_dconic_lang", "dL_dopacity_lang", "dL_dlanguage", "dL_dcov3D_lang"):
            assert bool((gr[k] != 0).any()), f"{scene}: {k} is all zero"


def test_chain_entry_replays_the_backward(scene):
    """refd_backward_chain (what the GPU file runs on the product's gradients) on the build's own composite-level
    gradients gives the build's own per-Gaussian gradients."""
    fr, gr = S.ref_run(scene)
    got = Rd.backward_chain(S.spec(scene), fr, gr)
    for k in Rd.CHAIN_KEYS:
        _eq(got[k], gr[k], f"{scene}: chain: {k}")


def test_backward_chain_equals_restatement(scene):
    """DGR-D's three per-Gaussian kernels against the restatement's chain, on gradients neither made.  A set whose
    square covers no tile is in no list, so no composite backward gives it a gradient: those rows are zero here too.
    (DGR-D's chain runs on them all the same when the other set is visible - it gates on the merged radii - and must
    then produce the zeros that the restatement's pass, which skips them, leaves.)"""
    import dgrd_oracle as D
    fr, _ = S.ref_run(scene)
    saved = S.oracle_run(scene)[3]
    s = S.spec(scene)
    P = s["means3D"].shape[0]
    g = torch.Generator().manual_seed(4242)
    comp = dict(dL_dmeans2D=torch.randn(P, 3, generator=g) * 1e-3, dL_dconic=torch.randn(P, 2, 2, generator=g) * 1e-2,
                dL_dconic_lang=torch.randn(P, 2, 2, generator=g) * 1e-2, dL_dcolors=torch.randn(P, 3, generator=g) * 1e-3,
                dL_ddepths=torch.randn(P, 1, generator=g) * 1e-3)
    for k in comp:
        rows = fr["fields"]["tiles_touched_lang" if k == "dL_dconic_lang" else "tiles_touched"] == 0
        comp[k][rows] = 0.0
    want = D.backward_chain(s, saved, comp)
    got = Rd.backward_chain(s, fr, comp)
    for k in Rd.CHAIN_KEYS:
        _eq(got[k], want[k], f"{scene}: chain: {k}")
    if scene != "all_culled":
        assert all(bool((want[k] != 0).any()) for k in ("dL_dmeans3D", "dL_dcov3D", "dL_dcov3D_lang", "dL_dtau"))


def test_radius_rule_on_the_border_scene():
    from online_lang_splatting_amd.disentangled import _merge_radii
    S.conditions("border")
    fr, _ = S.ref_run("border")
    out, _, _, _ = S.oracle_run("border")
    r1, r2 = out["raw_radii"]
    assert int(((r1 < 0) & (r2 > 0)).sum()) >= 1 and int(((r2 < 0) & (r1 > 0)).sum()) >= 1
    radii, radii_lang = _merge_radii(r1, r2)
    _eq(radii, fr["radii"], "border: _merge_radii: radii")
    _eq(radii_lang, fr["radii_lang"], "border: _merge_radii: radii_lang")
    _eq(out["radii"], fr["radii"], "border: the restatement's rule: radii")
    _eq(out["radii_lang"], fr["radii_lang"], "border: the restatement's rule: radii_lang")


def test_a_wrong_restatement_is_seen_to_fail():
    """The language loop skip-guarded and summed over the block (the plain oracle's exact mode) instead of DGR-D's
    unguarded recursion and thread 0's feature gradient: the dense scene tells them apart."""
    S.conditions("dense")
    _, gr = S.ref_run("dense")
    _, _, wrong, _ = S.oracle_run("dense", "default", _abi.BWD_EXACT)
    assert _diff(gr["dL_dlanguage"], wrong["dL_dlanguage"]) is not None
    assert _diff(gr["dL_dconic_lang"], wrong["dL_dconic_lang"]) is not None


def test_both_builds_were_used():
    from oracle import ref_build
    used = {(S.TILE, S.spec(n)["language"].shape[1]) for n in NAMES}
    assert set(ref_build.DGRD_BUILDS) <= used, (ref_build.DGRD_BUILDS, used)
