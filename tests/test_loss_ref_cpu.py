"""tests/loss_ref.py (the float32 restatement the GPU loss kernels are pinned to, tests/test_gpu_loss_pinned.py) held to the
reference: on the vectors the reference's own get_loss_mapping / get_loss_tracking produced (tests/golden/mapping_loss.npz and
the planted decisions of tests/golden/loss_edges.npz), and on oracle/loss_oracle.py run in float64.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loss_ref as LR  # noqa: E402
from oracle import loss_oracle  # noqa: E402

F32 = np.float32
CASES = LR.load_cases("mapping_loss") + LR.load_cases("loss_edges")
EDGES = [c for c in CASES if c[0].startswith("loss_edges")]
IDS = [c[0] for c in CASES]


def test_the_fixtures_hold_the_cases_the_tests_count_on():
    assert sum(1 for c in CASES if c[0].startswith("mapping_loss") and not c[1]) == 3
    assert sum(1 for c in CASES if c[0].startswith("mapping_loss") and c[1]) == 2
    assert len(EDGES) == 9
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "loss_edges.npz")) < 100 * 1000


def _within_ulps(got, gold, n):
    """|got - gold| <= n float32 ulp of gold, elementwise (both finite)."""
    got, gold = np.asarray(got, dtype=F32), np.asarray(gold, dtype=F32)
    return bool((np.abs(got.astype(np.float64) - gold.astype(np.float64)) <= n * np.spacing(np.abs(gold)).astype(np.float64)).all())


def _candidates_that_fit(c, tracking, keys, ulps=2):
    """The e^a candidates with which every cotangent in `keys` has the golden's zero pattern and sign and, with `ulps`, each
    magnitude within that many float32 ulp of the golden's."""
    cands = LR.ea_candidates(np.array([c["a"][0], c["b"][0]]), (not tracking) and bool(int(c["init"])))
    fit = []
    for ea in cands:
        r = LR.ref_for_case(c, tracking, ea=ea)
        good = True
        for k in keys:
            assert np.isfinite(c[k]).all() and r[k].dtype == F32 and r[k].shape == c[k].shape
            good &= bool(np.array_equal(r[k] == 0, c[k] == 0)) and bool(np.array_equal(np.sign(r[k]), np.sign(c[k])))
            if ulps is not None:
                good &= _within_ulps(r[k], c[k], ulps)
        if good:
            fit.append(ea)
    return fit


@pytest.mark.parametrize("name,tracking,c", CASES, ids=IDS)
def test_cotangents_have_the_references_decisions_and_magnitudes(name, tracking, c):
    """Zero pattern and sign are the golden's exactly, on all three cotangents; the colour and the language magnitudes are
    within 2 float32 ulp.  Not 0: torch's autograd forms the constant in another order — the mean's 1 / (3 H W) first, then
    alpha, then the mask and e^a, where the kernel forms alpha / (3 H W) once and multiplies by the sign, the mask and e^a:
    products rounded at different places, half an ulp each.  e^a: the correctly rounded value or a float32 neighbour (torch's
    expf is not correctly rounded either); ONE candidate must serve every output of the case."""
    assert _candidates_that_fit(c, tracking, ["d_depth"], ulps=None)
    assert _candidates_that_fit(c, tracking, ["d_image", "d_depth"] if tracking else ["d_image", "d_depth", "d_lang"], ulps=None)
    assert _candidates_that_fit(c, tracking, ["d_image"] if tracking else ["d_image", "d_lang"]), name


@pytest.mark.parametrize("name,tracking,c", CASES, ids=IDS)
def test_depth_cotangent_magnitude_is_within_2_ulp(name, tracking, c):
    """The depth cotangent's magnitude, (1 - alpha) / (H W), within 2 float32 ulp of the golden's.  The weight 1 - alpha is
    the one the reference forms: in double from its Python alpha, rounded to float32 where it meets the tensor
    (olsr_loss_params.one_minus_alpha, which the Python wrappers fill in that way).  1.f - float32(alpha), what the library
    falls back to when the field is 0, carries alpha's own rounding enlarged alpha / (1 - alpha) times: 3 ulp off on
    mapping_loss c0, c2 and t0."""
    assert _candidates_that_fit(c, tracking, ["d_depth"]), name


def _oracle64(c, tracking, alpha=None):
    d = lambda k: torch.from_numpy(np.asarray(c[k], dtype=np.float64))  # noqa: E731
    # the thresholds as the kernel holds them (float32, widened); no float32 lies between float32(0.01) and 0.01, so the
    # depth and opacity masks, which the reference writes as literals, decide alike in either precision
    kw = dict(alpha=float(F32(float(c["alpha"]))) if alpha is None else alpha, rgb_boundary_threshold=float(F32(float(c["thr"]))))
    if tracking:
        H, W = c["gt_depth"].shape
        return loss_oracle.tracking_loss_and_grads(d("image"), d("depth"), d("opacity"), d("gt_image"), d("gt_depth"),
                                                   torch.from_numpy(c["grad_mask"]).view(1, H, W) > 0.5, d("a"), d("b"), **kw)
    return loss_oracle.mapping_loss_and_grads(d("image"), d("depth"), None, d("gt_image"), d("gt_depth"), None, d("a"), d("b"),
                                              initialization=bool(int(c["init"])), **kw)


def _rel(got, want, floor):
    got, want = float(got), float(want)
    if not np.isfinite(want):
        return (np.isnan(got) and np.isnan(want)) or got == want
    return abs(got - want) <= 1e-12 * abs(want) + floor


@pytest.mark.parametrize("name,tracking,c", CASES, ids=IDS)
def test_float64_sums_agree_with_the_oracle_in_float64(name, tracking, c):
    """The statement evaluated in float64 (e^a = exp of the float32 a in double) against autograd on the oracle in float64: 1e-12
    relative (plus 4 float64 ulp of the sum of magnitudes, the floor of two float64 summation orders under cancellation).
    The language term is the exception: ATen computes the bilinear weights in the INPUT's precision, so the oracle in
    float64 resizes with float64 weights while the kernel, like the reference's float32 run, uses float32 weights.  It is held
    instead to the float64 sum over the float32 weights formed another way — two dense weight matrices, Wy g Wx^T — and the
    float64-weight oracle is held to that by the weights' own error."""
    a = F32(c["a"][0])
    init = (not tracking) and bool(int(c["init"]))
    r = LR.ref_for_case(c, tracking, ea=np.exp(np.float64(a)), dtype=np.float64)
    # The product's two weights, float32(alpha) and float32(1 - alpha) formed in double, are the reference's own pair and belong
    # to no single alpha: the oracle, which takes one, runs once with alpha = float32(alpha) for the colour term and once with
    # alpha = 1 - one_minus_alpha (exact in double, and 1 minus it is one_minus_alpha again) for the depth term.
    o = _oracle64(c, tracking)
    od = _oracle64(c, tracking, alpha=1.0 - float(r["one_minus_alpha"]))
    assert 1.0 - (1.0 - float(r["one_minus_alpha"])) == float(r["one_minus_alpha"])
    eps = 4 * 2.0 ** -52
    assert _rel(r["loss"][1], o["rgb"], eps * r["loss_mag"][1]), (r["loss"][1], float(o["rgb"]))
    assert _rel(r["loss"][2], od["depth"], eps * r["loss_mag"][2]), (r["loss"][2], float(od["depth"]))
    if not init:
        assert _rel(r["dexp"][0], o["dL_da"], eps * r["dexp_mag"][0]), (r["dexp"][0], float(o["dL_da"]))
        assert _rel(r["dexp"][1], o["dL_db"], eps * r["dexp_mag"][1]), (r["dexp"][1], float(o["dL_db"]))
    else:
        assert r["dexp"][0] == 0 and r["dexp"][1] == 0 and float(o["dL_da"]) == 0
    # the float64 cotangents are the oracle's: same decisions, magnitudes to 1e-12
    np.testing.assert_allclose(r["d_image"], o["dL_dimage"].numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["d_depth"], od["dL_ddepth"].numpy(), rtol=1e-12, atol=0)
    if tracking:
        return
    H, W = c["image"].shape[1:]
    Fc, lh, lw = c["gt_lang"].shape

    def dense(n_out, n_in):
        i0, i1, l0, l1 = LR.bilinear_index(n_out, n_in)
        M = np.zeros((n_out, n_in))
        np.add.at(M, (np.arange(n_out), i0), l0.astype(np.float64))
        np.add.at(M, (np.arange(n_out), i1), l1.astype(np.float64))
        return M
    g64 = c["gt_lang"].astype(np.float64)
    t = np.einsum("yi,cij,xj->cyx", dense(H, lh), g64, dense(W, lw))
    np.testing.assert_allclose(r["t64"], t, rtol=0, atol=8 * 2.0 ** -52 * float(np.abs(g64).max()))
    with np.errstate(all="ignore"):
        lang = float(np.abs(c["lang"].astype(np.float64) - t).sum()) / (Fc * H * W)
    assert _rel(r["loss"][3], lang, eps * r["loss_mag"][3]), (r["loss"][3], lang)
    # float64 weights against float32 weights: src = scale (dst + 0.5) - 0.5 carries three roundings of a number below the
    # target's size, l0 = 1 - l1 one more; the interpolant is continuous and piecewise linear with slope <= 2 max|g| per axis
    t_aten = torch.nn.functional.interpolate(torch.from_numpy(g64)[None], size=(H, W), mode="bilinear", align_corners=False)[0]
    werr = 2.0 ** -24 * (3 * (lw + lh) + 2) * 2 * float(np.abs(g64).max())
    assert float(np.abs(t_aten.numpy() - r["t64"]).max()) <= werr


@pytest.mark.parametrize("name,tracking,c", [c for c in CASES if np.isfinite(c[2]["loss"]).all()],
                         ids=[c[0] for c in CASES if np.isfinite(c[2]["loss"]).all()])
def test_float32_terms_are_the_float64_statement_rounded(name, tracking, c):
    """The float32 terms (the truth of the GPU sums) against the float64 statement with the same e^a: each |rgb| term is formed
    by at most 5 roundings of numbers no larger than e^a |x| + |b| + |gt| (product, sum, two masked products, difference; the
    opacity weight), each |depth| term by 3 of |depth| + |gt_depth|, each |language| term by 4 of mag and one of |l| + mag.
    Also the loss the reference returned, a float32 mean in torch's order: within 1e-5 of the sums of magnitudes."""
    ea = LR.ea_candidates(np.array([c["a"][0], c["b"][0]]), (not tracking) and bool(int(c["init"])))[0]
    r32 = LR.ref_for_case(c, tracking, ea=ea)
    r64 = LR.ref_for_case(c, tracking, ea=ea, dtype=np.float64)
    u = 2.0 ** -24
    x, gt = np.abs(c["image"]).astype(np.float64), np.abs(c["gt_image"]).astype(np.float64)
    use = r32["use_exposure"]
    scale0 = float(((float(ea) * x + abs(float(c["b"][0])) if use else x) + gt).sum())
    scale1 = float((np.abs(c["depth"]).astype(np.float64).reshape(-1) + np.abs(c["gt_depth"]).astype(np.float64).reshape(-1)).sum())
    assert abs(r32["sums"][0] - r64["sums"][0]) <= 6 * u * scale0
    assert abs(r32["sums"][1] - r64["sums"][1]) <= 4 * u * scale1
    if not tracking:
        scale2 = float(np.abs(c["lang"]).astype(np.float64).sum() + 6 * r32["mag"].sum())
        assert abs(r32["sums"][2] - r64["sums"][2]) <= 6 * u * scale2
    total = r32["loss"][0]
    assert abs(total - float(c["loss"])) <= 1e-5 * (r32["loss_mag"][1] + r32["loss_mag"][2] + r32["loss_mag"][3])


def _around(v):
    v = F32(v)
    return np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))


def test_every_planted_edge_occurs():
    """The decisions of the header, each counted in the inputs of loss_edges.npz: an edge that a later regeneration loses
    fails here instead of passing unexercised (as "the border case must occur" in test_gpu_disentangled.py)."""
    n = dict.fromkeys(["thr_below", "thr_equal", "thr_above", "thr_equal_three_channels", "depth_below", "depth_equal",
                       "depth_above", "opacity_below", "opacity_equal", "opacity_above", "tie_rgb", "tie_depth", "tie_lang",
                       "grad_mask_zero_on_live_pixel", "target_larger", "target_smaller", "target_identity", "target_1x1",
                       "nan_live", "inf_live", "nan_masked", "nan_language", "source_clamped_at_0", "i1_equals_i0",
                       "initialization"], 0)
    for name, tracking, c in EDGES:
        r = LR.ref_for_case(c, tracking)
        gt = c["gt_image"]
        gsum = (gt[0] + gt[1]) + gt[2]
        lo, eq, hi = _around(float(c["thr"]))
        n["thr_below"] += int((gsum == lo).sum())
        n["thr_equal"] += int((gsum == eq).sum())
        n["thr_above"] += int((gsum == hi).sum())
        n["thr_equal_three_channels"] += int(((gsum == eq) & ((gt != 0).sum(0) >= 2)).sum())
        assert not ((gsum == eq) & (r["m"] != 0)).any() and not ((gsum == lo) & (r["m"] != 0)).any()   # > is strict
        lo, eq, hi = _around(0.01)
        gd = c["gt_depth"]
        n["depth_below"] += int((gd == lo).sum())
        n["depth_equal"] += int((gd == eq).sum())
        n["depth_above"] += int((gd == hi).sum())
        assert not ((gd <= eq) & (r["md"] != 0)).any()
        finite = np.isfinite(c["image"]).all(0)
        live = (r["m"] != 0)
        n["tie_rgb"] += int(((r["terms"][0] == 0) & live[None] & finite[None]).sum())
        n["tie_depth"] += int(((r["terms"][1] == 0) & (r["md"] != 0)).sum())
        n["nan_live"] += int((np.isnan(c["image"]).any(0) & live).sum())
        n["inf_live"] += int((np.isinf(c["image"]).any(0) & live).sum())
        n["nan_masked"] += int((np.isnan(c["image"]).any(0) & ~live).sum())
        if tracking:
            lo, eq, hi = _around(0.95)
            op, valid = c["opacity"][0], gd > F32(0.01)
            n["opacity_below"] += int(((op == lo) & valid).sum())
            n["opacity_equal"] += int(((op == eq) & valid).sum())
            n["opacity_above"] += int(((op == hi) & valid).sum())
            assert not ((op <= eq) & (r["md"] != 0)).any() and ((op == hi) & valid & (r["md"] != 0)).any()
            n["grad_mask_zero_on_live_pixel"] += int(((c["grad_mask"].reshape(gsum.shape) == 0) & (gsum > F32(float(c["thr"])))
                                                      & finite).sum())
            continue
        n["initialization"] += int(c["init"])
        H, W = c["image"].shape[1:]
        _, lh, lw = c["gt_lang"].shape
        n["tie_lang"] += int((r["terms"][2] == 0).sum())
        n["nan_language"] += int(np.isnan(c["lang"]).sum())
        n["target_larger"] += int(lh > H and lw > W)
        n["target_smaller"] += int(1 < lh < H and 1 < lw < W)
        n["target_identity"] += int((lh, lw) == (H, W))
        n["target_1x1"] += int((lh, lw) == (1, 1))
        for n_out, n_in in ((H, lh), (W, lw)):
            scale = F32(n_in) / F32(n_out)
            src = scale * (np.arange(n_out, dtype=F32) + F32(0.5)) - F32(0.5)
            i0, i1, _, _ = LR.bilinear_index(n_out, n_in)
            n["source_clamped_at_0"] += int((src < 0).sum())
            n["i1_equals_i0"] += int((i1 == i0).sum())
    missing = [k for k, v in n.items() if v == 0]
    assert not missing, (missing, n)


def test_a_poisoned_pixel_has_a_zero_cotangent_and_poisons_its_sums():
    """What the reference returned for the non-finite cases, and that the restatement says the same: sign(NaN) = 0, so the NaN
    pixel's cotangent is 0; NaN * 0 = NaN, so the masked NaN poisons the mean all the same; +inf keeps a finite cotangent."""
    seen = 0
    for name, tracking, c in EDGES:
        nan_px = np.isnan(c["image"])
        if not nan_px.any() and (tracking or not np.isnan(c["lang"]).any()):
            continue
        seen += 1
        r = LR.ref_for_case(c, tracking)
        assert np.isnan(float(c["loss"])) and np.isnan(r["loss"][0])
        assert (c["d_image"][nan_px] == 0).all() and (r["d_image"][nan_px] == 0).all()
        if nan_px.any():
            inf_px = np.isinf(c["image"])
            assert inf_px.any() and np.isfinite(c["d_image"][inf_px]).all() and (c["d_image"][inf_px] != 0).all()
            assert np.isnan(float(c["d_a"][0])) and np.isnan(r["dexp"][0])
            assert np.isfinite(float(c["d_b"][0])) and np.isfinite(r["dexp"][1])      # dab = 0 at a NaN, the mask at +inf
            assert np.isnan(r["loss"][1]) and np.isfinite(r["loss"][2])             # colour poisoned, depth clean
        else:
            assert np.isfinite(r["loss"][1]) and np.isfinite(r["loss"][2]) and np.isnan(r["loss"][3])
            assert (c["d_lang"][np.isnan(c["lang"])] == 0).all()
    assert seen == 3
