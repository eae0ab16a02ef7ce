"""The 2-D evaluation's query scoring without a GPU: the numpy restatement equals what the reference's own `smooth` returned
(tests/golden/query_eval.npz), the symbols load, the constants mirror include/olsr.h, every argument error returns OLSR_ERR_ARG
before anything touches the device (the pointers below are never dereferenced), and the host layer refuses CPU tensors, wrong
dtypes and wrong shapes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import query_eval_ref as R
from online_lang_splatting_amd import _abi

ENTRIES = ("olsr_mask_smooth", "olsr_query_eval_scratch_bytes", "olsr_query_eval", "olsr_image_psnr_scratch_bytes",
           "olsr_image_psnr")
PTR = 0x1000
P, H, W = 3, 37, 71


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def Z():
    return R.golden()


@pytest.mark.parametrize("h,w", R.SMOOTH_SIZES)
def test_restatement_equals_the_recorded_smooth(Z, h, w):
    masks, want = Z[f"smooth_{h}x{w}_in"], Z[f"smooth_{h}x{w}_out"]
    assert np.array_equal(masks, R.make_masks(h, w))   # the generator's inputs are the ones a test can rebuild
    assert masks.shape == want.shape == (len(R.MASK_KINDS), h, w)
    for k, kind in enumerate(R.MASK_KINDS):
        assert np.array_equal(R.smooth(masks[k]), want[k]), kind
        assert np.array_equal(R.smooth(masks[k] * np.uint8(255)), want[k]), kind   # a byte != 0 counts as 1
    assert want[R.MASK_KINDS.index("ones")].all() and not want[R.MASK_KINDS.index("zeros")].any()
    assert not want[R.MASK_KINDS.index("last_row_and_column")].any()   # neither ever enters a window


def test_restated_counts_on_a_hand_made_image():
    sm = np.zeros((6, 8), np.float32)
    sm[1, 2] = sm[4, 6] = 2.0   # a plateau of two: the first in row-major order at (x, y) = (2, 1)
    assert R.localise(sm, np.float32([[5, 3, 7, 5]])) == (2, 1)       # only the later one lies inside
    assert R.localise(sm, np.float32([[3, 2, 5, 3]])) == (2, 0)
    assert R.localise(sm, np.float32([[6, 4, 2, 1]])) == (2, 1)       # x1 > x2, y1 > y2; both on the edge
    assert R.localise(sm, np.zeros((0, 4), np.float32)) == (2, 0)
    assert R.iou_counts(np.zeros((2, 2), bool), np.zeros((2, 2), np.uint8)) == (0, 0)
    r = R.score_image(np.zeros((1, 6, 8), np.uint8), sm[None], np.zeros((1, 6, 8), np.uint8), np.zeros((0, 4)), [0, 0])
    assert np.isnan(r["iou"][0]) and r["n_max"][0] == 2 and r["hit"][0] == 0


def test_symbols_constants_and_exports(L):
    from online_lang_splatting_amd import _lib
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "olsr.h")).read()
    for s in ENTRIES:
        assert hasattr(L, s) and s in _lib.EXPORTS and s + "(" in header
    for line in ("#define OLSR_QUERY_EVAL_MAX_PLANES 65535", "#define OLSR_QUERY_EVAL_MAX_EXTENT 1048576"):
        assert line in header, line
    assert (_abi.QUERY_EVAL_MAX_PLANES, _abi.QUERY_EVAL_MAX_EXTENT) == (65535, 1048576)
    assert _abi.QUERY_EVAL_RESULT == ("intersection", "union", "n_max", "hit")
    # 16 bytes per phrase and 64 x 64 tile, and the parked offsets
    small, big = L.olsr_query_eval_scratch_bytes(P, H, W), L.olsr_query_eval_scratch_bytes(7, 680, 1200)
    assert small >= 16 * P * 2 + 4 * (P + 1) and big >= 16 * 7 * 11 * 19 + 4 * 8 and big > small
    assert L.olsr_image_psnr_scratch_bytes() >= 16
    import online_lang_splatting_amd as pkg
    for name in ("query_eval", "QueryEvaluator", "smooth_masks", "frame_metrics"):
        assert getattr(pkg, name) is not None and name in pkg.__all__
    for name in ("smooth_masks", "QueryEvaluator", "psnr", "frame_metrics"):
        assert hasattr(pkg.query_eval, name)


def _errors(L, fn, ok, rows, prefix):
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert fn(*args) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error().startswith(prefix), (what, L.olsr_last_error())


SIZES = [("P = 0", {0: 0}), ("P < 0", {0: -1}), ("P above the grid", {0: 65536}), ("H = 1", {1: 1}), ("H = 0", {1: 0}),
         ("H < 0", {1: -H}), ("W = 1", {2: 1}), ("W = 0", {2: 0}), ("W < 0", {2: -W}), ("H above 2^20", {1: (1 << 20) + 1}),
         ("H W above int32", {1: 1 << 16, 2: 1 << 16})]


def test_mask_smooth_argument_errors(L):
    # P, H, W, mask_in, mask_out, stream
    ok = [P, H, W, PTR, 2 * PTR, None]
    rows = SIZES + [("mask_in", {3: None}), ("mask_out", {4: None}), ("in place", {4: PTR})]
    _errors(L, L.olsr_mask_smooth, ok, rows, b"mask_smooth: ")


def test_query_eval_argument_errors(L):
    # P, H, W, mask, smoothed, score, gt_mask, boxes, box_offsets, result, mask_smoothed, scratch, stream
    off = (C.c_int32 * (P + 1))(0, 1, 1, 2)
    down = (C.c_int32 * (P + 1))(0, 2, 1, 2)
    negative = (C.c_int32 * (P + 1))(-1, 0, 1, 2)
    adr = lambda a: C.cast(a, C.c_void_p)   # noqa: E731
    ok = [P, H, W, PTR, PTR, PTR, PTR, PTR, adr(off), PTR, None, PTR, None]
    rows = SIZES + [("mask", {3: None}), ("smoothed", {4: None}), ("score", {5: None}), ("gt_mask", {6: None}),
                    ("box_offsets", {8: None}), ("decreasing box_offsets", {8: adr(down)}),
                    ("box_offsets below 0", {8: adr(negative)}), ("boxes, with boxes listed", {7: None}), ("result", {9: None}),
                    ("scratch", {11: None}), ("mask_smoothed = mask", {10: PTR})]
    _errors(L, L.olsr_query_eval, ok, rows, b"query_eval: ")


def test_image_psnr_argument_errors(L):
    # C, H, W, image, gt, out, scratch, stream
    ok = [3, H, W, PTR, PTR, PTR, PTR, None]
    rows = [("C = 0", {0: 0}), ("H = 0", {1: 0}), ("W < 0", {2: -1}), ("C H W above int32", {0: 1 << 11, 1: 1 << 10, 2: 1 << 10}),
            ("image", {3: None}), ("gt", {4: None}), ("out", {5: None}), ("scratch", {6: None})]
    _errors(L, L.olsr_image_psnr, ok, rows, b"image_psnr: ")


def test_host_layer_refuses_what_it_cannot_run():
    from online_lang_splatting_amd import QueryEvaluator, query_eval
    with pytest.raises(RuntimeError, match="GPU"):
        query_eval.smooth_masks(torch.zeros(H, W, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        query_eval.smooth_masks(np.zeros((H, W), np.uint8))
    with pytest.raises(RuntimeError, match="GPU"):
        query_eval.psnr(torch.zeros(3, H, W), torch.zeros(3, H, W))
    with pytest.raises(RuntimeError, match="GPU"):
        query_eval.frame_metrics(torch.zeros(3, H, W), torch.zeros(3, H, W))
    with pytest.raises(RuntimeError, match="LanguageQuery"):
        QueryEvaluator(object())
    # dtype and shape checks come before anything native: a meta tensor that claims to be on the GPU is enough
    for fn, args, match in (
            (query_eval.smooth_masks, (_Fake((H, W), torch.float32),), "uint8"),
            (query_eval.smooth_masks, (_Fake((P, 2, H, W), torch.uint8),), r"\(3, 2, 37, 71\)"),
            (query_eval.smooth_masks, (_Fake((H, 1), torch.uint8),), r"\(1, 37, 1\)"),
            (query_eval.psnr, (_Fake((3, H, W), torch.float64), _Fake((3, H, W), torch.float64)), "float32"),
            (query_eval.psnr, (_Fake((3, H, W), torch.float32), _Fake((3, H, W + 1), torch.float32)), r"\(3, 37, 72\)"),
            (query_eval.psnr, (_Fake((H, W), torch.float32), _Fake((H, W), torch.float32)), r"\(37, 71\)"),
            (query_eval.frame_metrics, (_Fake((1, H, W), torch.float32), _Fake((1, H, W), torch.float32)), r"\(1, 37, 71\)")):
        with pytest.raises(RuntimeError, match=match):
            fn(*args)


class _Fake(torch.Tensor):
    """A tensor without storage whose is_cuda is True: reaches the dtype and shape checks on a host without a GPU."""

    @staticmethod
    def __new__(cls, shape, dtype):
        return torch.Tensor._make_subclass(cls, torch.empty(shape, dtype=dtype, device="meta"))

    is_cuda = True
