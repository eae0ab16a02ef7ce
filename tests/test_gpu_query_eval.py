"""olsr_mask_smooth / olsr_query_eval / olsr_image_psnr (HIP) and online_lang_splatting_amd.query_eval on the GPU.

Smoothing and scoring are integer arithmetic: every comparison below is exact.  The smoothing's yardstick is what the
reference's own `smooth` returned (tests/golden/query_eval.npz); the counts' yardstick is the numpy restatement of
tests/query_eval_ref.py.  The PSNR is held to the reference's float64 value within the error of the reference's own float32
run, but no less than 4 * 2^-24 relative on the mse (query_eval_ref.psnr_tolerance)."""
import math

import numpy as np
import pytest
import torch

import query_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def Z():
    return R.golden()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("h,w", R.SMOOTH_SIZES)
def test_smoothing_equals_the_reference(hip, Z, h, w):
    from online_lang_splatting_amd import smooth_masks
    masks, want = Z[f"smooth_{h}x{w}_in"], Z[f"smooth_{h}x{w}_out"]
    got = smooth_masks(_dev(masks))
    assert got.dtype == torch.uint8 and tuple(got.shape) == masks.shape
    first = got.cpu().numpy()
    for k, kind in enumerate(R.MASK_KINDS):
        assert np.array_equal(first[k], want[k]), (kind, int((first[k] != want[k]).sum()))
    assert np.array_equal(smooth_masks(_dev(masks)).cpu().numpy(), first)                      # the same bits again
    assert np.array_equal(smooth_masks(_dev(masks * np.uint8(255))).cpu().numpy(), want)      # 255 in place of 1
    # planes that start at odd addresses: a stack of three inside a larger buffer, one byte in
    if (h * w) % 2:
        buf = torch.zeros(3 * h * w + 1, dtype=torch.uint8, device=DEV)
        view = buf[1:].view(3, h, w)
        view.copy_(_dev(masks[:3]))
        assert view.data_ptr() % 2 == 1 and np.array_equal(smooth_masks(view).cpu().numpy(), want[:3])
    one = smooth_masks(_dev(masks[0]))   # [H,W] in, [H,W] out
    assert tuple(one.shape) == (h, w) and np.array_equal(one.cpu().numpy(), want[0])


def _evaluator():
    """An evaluator for result dicts alone: its LanguageQuery is never asked."""
    from online_lang_splatting_amd import QueryEvaluator
    from online_lang_splatting_amd.lang_query import LanguageQuery
    q = object.__new__(LanguageQuery)
    q.device = torch.device(DEV)
    return QueryEvaluator(q)


# two tiles each way, neither extent a multiple of the tile or of 4
SH, SW = 70, 75


def _scoring_case():
    """Seven phrases; smoothed maps with hand-placed maxima (2.0 over a field below 1), maxima in different tiles."""
    rng = np.random.default_rng(5)
    P = 7
    mask = (rng.random((P, SH, SW)) < 0.5).astype(np.uint8)
    gt = (rng.random((P, SH, SW)) < 0.4).astype(np.uint8)
    gt[3] *= 255                                # any byte != 0 is set
    sm = rng.random((P, SH, SW)).astype(np.float32)
    boxes, off = [], [0]

    def phrase(p, maxima, bxs):
        for x, y in maxima:
            sm[p, y, x] = 2.0
        boxes.extend(bxs)
        off.append(len(boxes))

    mask[0], gt[0] = 0, 0                                                # a union of 0: iou NaN
    phrase(0, [(10, 10)], [(5, 5, 20, 20)])
    phrase(1, [(3, 2), (70, 66)], [(68, 60, 74, 69)])                    # the first maximum outside, a later one inside
    phrase(2, [(3, 2), (70, 66), (40, 30)], [(10, 10, 30, 25)])          # every maximum outside
    phrase(3, [(64, 63)], [(64, 10, 70, 63)])                            # exactly on the box's corner
    phrase(4, [(30, 65)], [(35, 69, 25, 60)])                            # x1 > x2, y1 > y2
    phrase(5, [(12, 12)], [])                                            # no box, between two phrases that have some
    phrase(6, [(66, 5)], [(0, 0, 10, 10), (60, 0, 74.5, 5.0)])           # only the second box hits
    return mask, sm, gt, np.float32(boxes).reshape(-1, 4), np.int32(off)


def test_scoring_equals_the_restatement(hip):
    mask, sm, gt, boxes, off = _scoring_case()
    want = R.score_image(mask, sm, gt, boxes, off)
    assert want["hit"].tolist() == [1, 1, 0, 1, 1, 0, 1] and want["n_max"].tolist() == [1, 2, 3, 1, 1, 1, 1]
    assert want["union"][0] == 0 and math.isnan(want["iou"][0]) and want["union"][1:].min() > 0
    ev = _evaluator()
    result = dict(mask=_dev(mask), smoothed=_dev(sm), score=_dev(sm.reshape(len(sm), -1).max(axis=1)))
    for offsets in (off, off.tolist(), _dev(off)):   # an array, a list, a device tensor
        got = ev.evaluate(result, _dev(gt), _dev(boxes), offsets)
        for k in ("intersection", "union", "n_max", "hit"):
            assert got[k].tolist() == want[k].tolist(), k
        assert np.array_equal(got["iou"], want["iou"], equal_nan=True) and got["iou"].dtype == np.float64
        assert np.array_equal(got["mask_smoothed"].cpu().numpy(), want["mask_smoothed"])
        assert got["accuracy"] == 5 / 7 and math.isnan(got["mean_iou"])
    # the first maximum in row-major order alone would have said 0 for phrase 1
    first = np.unravel_index(np.argmax(sm[1]), sm[1].shape)
    assert R.localise(np.where(np.arange(SH * SW).reshape(SH, SW) == first[0] * SW + first[1], 2.0, 0.0), boxes[1:2]) == (1, 0)
    # the table of offsets in device memory, straight at the C entry
    from online_lang_splatting_amd._lib import check, lib
    P = len(mask)
    d = dict(mask=result["mask"], sm=result["smoothed"], score=result["score"], gt=_dev(gt), boxes=_dev(boxes), off=_dev(off),
             out=torch.empty((P, 4), dtype=torch.int32, device=DEV),
             scratch=torch.empty(lib().olsr_query_eval_scratch_bytes(P, SH, SW), dtype=torch.uint8, device=DEV))
    check(lib().olsr_query_eval(P, SH, SW, d["mask"].data_ptr(), d["sm"].data_ptr(), d["score"].data_ptr(), d["gt"].data_ptr(),
                                d["boxes"].data_ptr(), d["off"].data_ptr(), d["out"].data_ptr(), None, d["scratch"].data_ptr(),
                                None))
    assert d["out"].cpu().numpy().tolist() == np.stack([want[k] for k in ("intersection", "union", "n_max", "hit")], 1).tolist()
    # no boxes at all
    none = ev.evaluate(result, _dev(gt), torch.zeros((0, 4), device=DEV), [0] * 8)
    assert none["hit"].tolist() == [0] * 7 and none["n_max"].tolist() == want["n_max"].tolist()
    with pytest.raises(RuntimeError, match=r"\(7, 70, 74\)"):
        ev.evaluate(result, _dev(gt[:, :, :-1]), _dev(boxes), off)
    with pytest.raises(RuntimeError, match="box_offsets"):
        ev.evaluate(result, _dev(gt), _dev(boxes), off[:-1])
    with pytest.raises(RuntimeError, match="uint8"):
        ev.evaluate(result, _dev(gt).float(), _dev(boxes), off)


def test_end_to_end_on_a_queried_code_map(hip):
    """evaluate(codes) at 24 x 40 equals smooth + IoU + localisation restated on the mask and the smoothed relevancy that
    LanguageQuery.relevancy itself returned; summary() over two images is the mean of the images' means."""
    import lang_query_ref as Q
    from online_lang_splatting_amd import QueryEvaluator
    from test_gpu_lang_query import _query
    from test_lang_query_ref_golden import golden_case
    case, _, _ = golden_case(Q.golden(), "direct")
    q = _query(case)
    codes = case["codes"].to(DEV)
    H, W = 24, 40
    n_pos = case["pos"].shape[0]
    rng = np.random.default_rng(9)
    ev, ev_dict = QueryEvaluator(q), QueryEvaluator(q)
    means, accs = [], []
    for image in range(2):
        gt = np.zeros((n_pos, H, W), np.uint8)
        for p in range(n_pos):
            y, x = rng.integers(0, H - 8), rng.integers(0, W - 12)
            gt[p, y:y + 8 + 4 * image, x:x + 12] = 1
        boxes = np.float32([[0, 0, W - 1, H - 1], [0, 0, 3, 3], [W, H, W + 5, H + 5]][:n_pos])   # all, a corner, outside
        off = np.arange(n_pos + 1, dtype=np.int32)
        got = ev.evaluate(codes, _dev(gt), _dev(boxes), off, out_hw=(H, W))
        r = q.relevancy(codes, out_hw=(H, W))
        assert tuple(r["mask"].shape) == (n_pos, H, W)
        want = R.score_image(r["mask"].cpu().numpy(), r["smoothed"].cpu().numpy(), gt, boxes, off)
        assert np.array_equal(want["n_max"] >= 1, np.ones(n_pos, bool)) and want["hit"][0] == 1
        for k in ("intersection", "union", "n_max", "hit"):
            assert got[k].tolist() == want[k].tolist(), k
        assert np.array_equal(got["mask_smoothed"].cpu().numpy(), want["mask_smoothed"])
        assert np.array_equal(got["iou"], want["iou"], equal_nan=True)
        assert got["mean_iou"] == sum(want["iou"].tolist()) / n_pos and got["accuracy"] == int(want["hit"].sum()) / n_pos
        again = ev_dict.evaluate(r, _dev(gt), _dev(boxes), off)   # the dict relevancy() returned, in place of the codes
        assert again["intersection"].tolist() == want["intersection"].tolist() and again["hit"].tolist() == want["hit"].tolist()
        means.append(got["mean_iou"])
        accs.append(got["accuracy"])
    s = ev.summary()
    assert s["mean_iou"] == sum(means) / 2 and s["accuracy"] == sum(accs) / 2 and s["images"] == 2
    assert ev_dict.summary() == s
    ev.reset()
    assert ev.summary() == dict(mean_iou=0, accuracy=0, images=0)


def test_psnr_against_the_reference(hip, Z):
    from online_lang_splatting_amd import query_eval
    image, gt = Z["psnr_image"], Z["psnr_gt"]
    assert image.shape == R.PSNR_SHAPE and (image < 0).any() and (image > 1).any() and (gt == 0).any()
    mse64, mse32 = float(Z["mse_f64"]), float(Z["mse_f32"])
    tol = R.psnr_tolerance(mse64, mse32)
    s, n = query_eval.psnr_sums(_dev(image), _dev(gt)).tolist()
    assert n == int((gt > 0).sum())
    err = abs(s / n - mse64) / mse64
    print(f"mse {s / n!r} against {mse64!r}: relative error {err:.3e}, allowed {tol:.3e} (the reference's float32 run: "
          f"{abs(mse32 - mse64) / mse64:.3e})")
    assert err <= tol
    got = query_eval.psnr(_dev(image), _dev(gt))
    # d psnr = 10 / ln 10 * d mse / mse
    assert abs(got - float(Z["psnr_f64"])) <= 10.0 / math.log(10.0) * tol * 1.0000001
    assert query_eval.psnr(_dev(image), _dev(gt)) == got   # the same bits again
    # an array that is not 16-byte aligned takes the scalar loads: the same bits
    buf = torch.zeros(2, image.size + 1, dtype=torch.float32, device=DEV)
    a, g = buf[0, 1:].view(*image.shape), buf[1, 1:].view(*image.shape)
    a.copy_(_dev(image))
    g.copy_(_dev(gt))
    assert a.data_ptr() % 16 == 4 and query_eval.psnr_sums(a, g).tolist() == [s, n]
    assert math.isnan(query_eval.psnr(_dev(image), torch.zeros_like(_dev(gt)))) and math.isnan(float(Z["psnr_empty_f32"]))


def test_frame_metrics_ssim_is_the_fused_ssim(hip, Z):
    from online_lang_splatting_amd import frame_metrics, losses, query_eval
    image, gt = _dev(Z["psnr_image"]), _dev(Z["psnr_gt"])
    m = frame_metrics(image, gt)
    assert m["ssim"] == float(losses.ssim(torch.clamp(image, 0.0, 1.0), gt))
    assert m["psnr"] == query_eval.psnr(image, gt)
