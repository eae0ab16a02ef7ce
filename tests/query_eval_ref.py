"""numpy restatement of the 2-D evaluation's query scoring (include/olsr.h, "scoring text queries"; csrc/k_query_eval.hip), and
the cases of tests/golden/query_eval.npz.

`smooth` restates eval/utils.py:47-56 without its loop (an integral image gives every clamped window's count); the golden file
holds what the reference's own loop returned for the masks below, and tests/test_query_eval_cpu.py holds this restatement to it
bit for bit.  `iou_counts` and `localise` restate eval/evaluate_onlinelangslam.py:160-161 and :203-223: those statements sit
inside functions that call cv2 and write files, so they cannot be recorded from the reference and are pinned here instead.
`psnr_reference` is utils/eval_utils.py:153, :171-173 around the reference's psnr (recorded in the golden file)."""
import os

import numpy as np

SCALE = 3   # eval/utils.py:50

# (H, W): the least legal size; a window wider than the map; one tile edge exactly; odd planes (planes 1.. of a stack start
# unaligned); across a 64-wide and a 64-high tile edge with the halo on both sides and a width that is no multiple of 4
SMOOTH_SIZES = ((2, 2), (5, 9), (8, 8), (37, 71), (66, 130))
MASK_KINDS = ("half_a", "half_b", "third", "ones", "zeros", "checkerboard", "last_row_and_column")
PSNR_SHAPE = (3, 37, 71)


def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_eval.npz"))


def make_masks(h, w, seed=0):
    """uint8 [len(MASK_KINDS),h,w] of 0 / 1: density 0.5 twice (the most ties) and 0.3, all ones, all zeros, a checkerboard
    (ties only in the even-area windows at the border), and a mask whose only ones are the last row and the last column."""
    rng = np.random.default_rng(1000 * h + w + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    last = np.zeros((h, w), np.uint8)
    last[-1, :] = 1
    last[:, -1] = 1
    planes = [rng.random((h, w)) < 0.5, rng.random((h, w)) < 0.5, rng.random((h, w)) < 0.3, np.ones((h, w)), np.zeros((h, w)),
              (yy + xx) % 2, last]
    return np.stack([np.asarray(p).astype(np.uint8) for p in planes])


def window_sums(x):
    """Per pixel the sum of x over rows max(0, i-3) .. min(i+4, h-1) - 1 and the same columns (the reference's slice), and the
    window's area.  x [h,w], h, w >= 2."""
    h, w = x.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = np.cumsum(np.cumsum(x.astype(np.int64), axis=0), axis=1)
    r0, r1 = np.maximum(0, np.arange(h) - SCALE), np.minimum(np.arange(h) + SCALE + 1, h - 1)
    c0, c1 = np.maximum(0, np.arange(w) - SCALE), np.minimum(np.arange(w) + SCALE + 1, w - 1)
    s = ii[r1][:, c1] - ii[r0][:, c1] - ii[r1][:, c0] + ii[r0][:, c0]
    return s, (r1 - r0)[:, None] * (c1 - c0)[None, :]


def smooth(mask):
    """eval/utils.py `smooth` of a 0 / 1 mask [h,w] (a byte != 0 counts as 1): np.argmax(np.bincount(window)) is 1 iff the
    ones outnumber the zeros strictly."""
    ones, area = window_sums(np.asarray(mask) != 0)
    return (2 * ones > area).astype(np.uint8)


def iou_counts(gt, smoothed_mask):
    """(:160-161) -> (intersection, union)"""
    return int(np.sum(np.logical_and(gt, smoothed_mask))), int(np.sum(np.logical_or(gt, smoothed_mask)))


def localise(smoothed, boxes):
    """(:203-223) for one head: smoothed [h,w] float, boxes [n,4] -> (n_max, hit)."""
    score = smoothed.max()
    coord = np.asarray(np.nonzero(smoothed == score)).transpose(1, 0)[..., ::-1]   # (x, y) rows
    hit = 0
    for box in np.asarray(boxes).reshape(-1, 4):
        x1, y1, x2, y2 = box
        x_min, x_max = min(x1, x2), max(x1, x2)
        y_min, y_max = min(y1, y2), max(y1, y2)
        for c in coord:
            if c[0] >= x_min and c[0] <= x_max and c[1] >= y_min and c[1] <= y_max:
                hit = 1
                break
        if hit:
            break
    return len(coord), hit


def score_image(mask, smoothed, gt, boxes, box_offsets):
    """All of a query's phrases: mask, gt uint8 [P,h,w], smoothed float [P,h,w] -> dict of int64 [P] arrays intersection, union,
    n_max, hit, the float64 iou (0 / 0 = NaN) and the smoothed masks."""
    P = mask.shape[0]
    out = dict(intersection=np.zeros(P, np.int64), union=np.zeros(P, np.int64), n_max=np.zeros(P, np.int64),
               hit=np.zeros(P, np.int64), mask_smoothed=np.stack([smooth(m) for m in mask]))
    for p in range(P):
        out["intersection"][p], out["union"][p] = iou_counts(gt[p] != 0, out["mask_smoothed"][p])
        out["n_max"][p], out["hit"][p] = localise(smoothed[p], np.asarray(boxes)[box_offsets[p]:box_offsets[p + 1]])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["iou"] = out["intersection"].astype(np.float64) / out["union"].astype(np.float64)
    return out


def make_psnr_case(seed=0):
    """image, gt float32 PSNR_SHAPE: the image leaves [0, 1] on both sides, a fifth of gt's elements are 0 (not in the mask)."""
    rng = np.random.default_rng(77 + seed)
    gt = rng.random(PSNR_SHAPE).astype(np.float32)
    gt[rng.random(PSNR_SHAPE) < 0.2] = 0.0
    image = (gt + rng.normal(0.0, 0.15, PSNR_SHAPE)).astype(np.float32)
    image[0, 0, :4] = (-0.5, 1.5, -1e-3, 1.0 + 1e-3)
    gt[0, 0, :4] = (0.25, 0.75, 0.5, 0.5)
    assert (image < 0).sum() > 10 and (image > 1).sum() > 10 and (gt == 0).sum() > 100
    return image, gt


PSNR_FLOOR = 4.0 * 2.0 ** -24   # relative, on the mse: the float32 subtraction; the double sums add nothing visible


def psnr_tolerance(mse64, mse32):
    """The allowed relative error of an mse against the reference's float64 value: the error of the reference's own float32
    run, but no less than PSNR_FLOOR."""
    return max(abs(float(mse32) - float(mse64)) / float(mse64), PSNR_FLOOR)
