"""Generates tests/golden/query_eval.npz: the reference's OWN `smooth` (eval/utils.py:47-56) and `psnr` / `mse`
(gaussian_splatting/utils/image_utils.py) on the cases of tests/query_eval_ref.py.  Runs ONLY where the reference checkout
exists (OLSR_REFERENCE names it); the committed .npz is data (arrays only).

What is executed from the reference: eval/utils.py is imported with mediapy, cv2 and colormaps stubbed (none of them is
installed; `smooth` uses numpy alone) and the eval package entered as a bare namespace, as make_golden_lang_query.py does;
`smooth` then runs its own double loop over every mask of query_eval_ref.make_masks at every size of SMOOTH_SIZES.
image_utils.py is loaded from its file; `psnr` and `mse` run on the evaluation's operands (utils/eval_utils.py:153, :171-173:
image = clamp(rendering, 0, 1), mask = gt_image > 0, psnr(image[mask].unsqueeze(0), gt_image[mask].unsqueeze(0))) in float64
("truth") and in float32 (the reference's own precision).

What is NOT executed: the IoU (:160-161 of eval/evaluate_onlinelangslam.py) and the box test (:203-223) sit inside
activate_stream and lerf_localization, which call cv2.filter2D and cv2.resize and write image files; cv2 is not installed.
Those statements are pinned by the numpy restatement tests/query_eval_ref.py (iou_counts, localise), not by this file.

Per size `smooth_{H}x{W}_in` / `_out` uint8 [7,H,W]; psnr_image, psnr_gt float32 [3,37,71], psnr_f64, psnr_f32, mse_f64,
mse_f32; psnr_empty_f32: the same call with an all-zero gt (NaN: the mean of nothing)."""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("OLSR_REFERENCE")
if not REF or not os.path.isdir(REF):
    raise SystemExit("set OLSR_REFERENCE to a checkout of the reference (rpng/online_lang_splatting)")
sys.path.insert(0, os.path.dirname(HERE))
import query_eval_ref as R  # noqa: E402

for name in ("mediapy", "cv2", "colormaps", "matplotlib", "matplotlib.patches", "matplotlib.pyplot"):
    if name not in sys.modules:
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
sys.modules["eval"] = types.ModuleType("eval")
sys.modules["eval"].__path__ = [os.path.join(REF, "eval")]
sys.path.insert(0, os.path.join(REF, "eval"))   # utils.py says `import colormaps`

from eval.utils import smooth  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_image_utils", os.path.join(REF, "gaussian_splatting", "utils", "image_utils.py"))
image_utils = importlib.util.module_from_spec(spec)
spec.loader.exec_module(image_utils)


def eval_psnr(rendering, gt_image):
    """utils/eval_utils.py:153, :171-173 -> (psnr, mse)"""
    image = torch.clamp(rendering, 0.0, 1.0)
    mask = gt_image > 0
    a, b = (image[mask]).unsqueeze(0), (gt_image[mask]).unsqueeze(0)
    return image_utils.psnr(a, b).item(), image_utils.mse(a, b).item()


def main():
    out = {}
    for h, w in R.SMOOTH_SIZES:
        masks = R.make_masks(h, w)
        sm = np.stack([smooth(m) for m in masks])
        assert sm.dtype == np.uint8 and set(np.unique(sm)) <= {0, 1}
        assert np.array_equal(sm, np.stack([R.smooth(m) for m in masks])), (h, w)
        out[f"smooth_{h}x{w}_in"], out[f"smooth_{h}x{w}_out"] = masks, sm
        print(f"{h} x {w}: ones in {masks.mean(axis=(1, 2)).round(3)} -> out {sm.mean(axis=(1, 2)).round(3)}")
    image, gt = R.make_psnr_case()
    out["psnr_image"], out["psnr_gt"] = image, gt
    p64, m64 = eval_psnr(torch.from_numpy(image).double(), torch.from_numpy(gt).double())
    p32, m32 = eval_psnr(torch.from_numpy(image), torch.from_numpy(gt))
    out["psnr_f64"], out["psnr_f32"], out["mse_f64"], out["mse_f32"] = (np.float64(v) for v in (p64, p32, m64, m32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out["psnr_empty_f32"] = np.float64(eval_psnr(torch.from_numpy(image), torch.zeros_like(torch.from_numpy(gt)))[0])
    assert np.isnan(out["psnr_empty_f32"])
    print(f"psnr {p64!r} (float32 run {p32!r}), mse {m64!r} ({m32!r}), tolerance {R.psnr_tolerance(m64, m32):.3e}")
    path = os.path.join(HERE, "query_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
