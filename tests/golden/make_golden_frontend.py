"""Generates tests/golden/frontend.npz by calling the REFERENCE's own front-end code on the CPU.  Runs ONLY where the reference
checkout exists (OLSR_REFERENCE names it); the committed .npz is data (arrays only).

  Camera.compute_grad_mask (utils/camera_utils.py:123-152) is called unbound on a stub, for both dataset types, and
  get_median_depth (utils/slam_utils.py:168-179) directly.  image_gradient / image_gradient_mask hard-code device="cuda";
  torch.tensor / torch.ones are wrapped for the duration of the call so that the keyword is dropped — the arithmetic is the
  reference's.
  FrontEnd.is_keyframe and FrontEnd.add_to_window (utils/slam_frontend.py:279-430) are taken out of the class by `ast` (the
  module imports a GUI and multiprocessing) and run on stub cameras.  The small-window rule and the single-thread rule are
  statements inside FrontEnd.run (:633-649), not a function; they are restated here on the same tensors.  dist and the ratios
  are recomputed with the reference's statements (is_keyframe returns only the boolean); the scores are what add_to_window hands
  to np.argmax, caught by giving it an `np` whose argmax records its argument.

Conditions on the inputs, asserted per case so that no discrete outcome hinges on rounding: every compared quantity is at least
1e-3 (relative) away from its threshold, the two best scores are at least 1e-3 apart, and the mask pixels whose float64
intensity lies within 2^-20 (relative) of the float64 threshold — |I - th| < 2^-20 |th|, strictly, so that I = th = 0 is no
near-tie: every precision answers 0 > 0 alike — are fewer than 0.1 % of the case.

Poses: the reference's getWorld2View2(R, T) inverts [R T] twice; the stored poses are [R T] itself, as the caller of
olsr_keyframe_decide holds it, so that rounding is part of the reference's own error against the float64 truth."""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if "OLSR_REFERENCE" not in os.environ:
    raise SystemExit("set OLSR_REFERENCE to the reference checkout")
REF = os.environ["OLSR_REFERENCE"]
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(HERE))
import frontend_ref as R  # noqa: E402
from gaussian_splatting.utils.graphics_utils import getWorld2View2  # noqa: E402
from utils.camera_utils import Camera  # noqa: E402
from utils.slam_utils import get_median_depth  # noqa: E402


class _on_cpu:
    """drops device="cuda" from torch.tensor / torch.ones while the reference runs"""

    def __enter__(self):
        self.saved = (torch.tensor, torch.ones)

        def strip(fn):
            def g(*a, **k):
                k.pop("device", None)
                return fn(*a, **k)
            return g
        torch.tensor, torch.ones = strip(torch.tensor), strip(torch.ones)

    def __exit__(self, *a):
        torch.tensor, torch.ones = self.saved


class _Stub:
    pass


def reference_mask(image, edge_threshold, dataset_type):
    cam = _Stub()
    cam.original_image = torch.from_numpy(image.copy())
    with _on_cpu():
        Camera.compute_grad_mask(cam, {"Training": {"edge_threshold": edge_threshold}, "Dataset": {"type": dataset_type}})
    return cam.grad_mask[0].to(torch.float32).numpy()


def make_image(seed, H, W, kind):
    g = np.random.default_rng(seed)
    img = (g.integers(0, 256, size=(3, H, W)).astype(np.float32) / np.float32(255)).astype(np.float32)
    if kind == "flat":
        img[:] = np.float32(0.5)
    if kind != "nodark" and kind != "flat":
        img[:, H // 3: H // 3 + max(H // 5, 2), W // 4: W // 4 + max(W // 5, 2)] = np.float32(0.002)   # dark: below 0.01
    if kind == "x8":
        img *= np.float32(8)
    return img


MASK_CASES = [("s32", 1, 32, 32, "nodark", 4.0), ("s64x96", 2, 64, 96, "dark", 4.0), ("s96x160", 3, 96, 160, "dark", 1.1),
              ("s85x131", 4, 85, 131, "dark", 4.0), ("s85x131b", 5, 85, 131, "dark", 1.1), ("flat", 6, 64, 96, "flat", 4.0),
              ("x8", 7, 96, 160, "x8", 4.0), ("s64x96b", 8, 64, 96, "dark", 1.1)]


def near_ties(I64, th64):
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(np.abs(I64 - th64) < 2.0 ** -20 * np.abs(th64)))


def mask_cases(out):
    names = []
    for name, seed, H, W, kind, thr in MASK_CASES:
        img = make_image(seed, H, W, kind)
        blocks, glob = reference_mask(img, thr, "replica"), reference_mask(img, thr, "tum")
        _, I64, th64 = R.grad_mask_blocks(img, thr, np.float64)
        _, _, tg64 = R.grad_mask_global(img, thr, np.float64)
        nb, ng = near_ties(I64, th64), near_ties(I64, tg64)
        assert nb <= 1e-3 * H * W and ng <= 1e-3 * H * W, (name, nb, ng)
        # the reference alone against the float64 truth outside the near-ties
        m64, _, _ = R.grad_mask_blocks(img, thr, np.float64)
        inblock = ~np.isnan(th64)
        far = inblock & ~(np.abs(I64 - th64) < 2.0 ** -20 * np.abs(th64))
        assert np.array_equal(blocks[far], m64[far].astype(np.float32)), name
        out[f"mask_{name}_image"], out[f"mask_{name}_thr"] = img, np.float64(thr)
        out[f"mask_{name}_blocks"], out[f"mask_{name}_global"] = blocks, glob
        names.append(name)
        print(f"mask {name}: {H}x{W} near-ties blocks {nb} global {ng}, ones {int((blocks == 1).sum())} / {int(glob.sum())}")
    out["mask_names"] = np.array(names)


def median_cases(out):
    g = np.random.default_rng(21)
    cases = {}
    d = g.integers(1, 6, size=40).astype(np.float32) * np.float32(0.5)            # ties
    cases["ties"] = (d, np.ones(40, np.float32), None)
    d = g.random(50).astype(np.float32) * 4
    d[::3] = 0
    o = g.random(50).astype(np.float32) * np.float32(0.1) + np.float32(0.93)
    cases["zeros"] = (d, o, None)
    d = g.random(9).astype(np.float32) + 1
    d[4] = np.inf
    cases["inf"] = (d, np.ones(9, np.float32), None)
    cases["one"] = (np.array([0, 2.5, 0], np.float32), np.ones(3, np.float32), None)
    cases["two"] = (np.array([3.5, 0, 1.25], np.float32), np.ones(3, np.float32), None)
    d = g.random(64).astype(np.float32) * 3 + np.float32(0.1)
    cases["even"] = (d, np.ones(64, np.float32), None)
    m = g.random(64) > 0.4
    cases["masked"] = (d, np.ones(64, np.float32), m)
    names = []
    for name, (d, o, m) in cases.items():
        med = get_median_depth(torch.from_numpy(d), torch.from_numpy(o), None if m is None else torch.from_numpy(m))
        valid = (d > 0) & (o > np.float32(0.95)) & (True if m is None else m)
        out[f"med_{name}_depth"], out[f"med_{name}_opacity"] = d, o
        out[f"med_{name}_mask"] = np.zeros(0, np.uint8) if m is None else m.astype(np.uint8)
        out[f"med_{name}_median"], out[f"med_{name}_count"] = np.float32(med.item()), np.int32(valid.sum())
        names.append(name)
    out["med_names"] = np.array(names)


def frontend_methods():
    path = os.path.join(REF, "utils", "slam_frontend.py")
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FrontEnd"][0]
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("is_keyframe", "add_to_window")]
    assert len(fns) == 2
    for fn in fns:
        fn.returns = None
        for a in fn.args.args:
            a.annotation = None

    class RecordingNp:
        def __init__(self):
            self.scores = None

        def argmax(self, x):
            self.scores = [float(v) for v in x]
            return np.argmax(x)
    rec = RecordingNp()
    scope = {"torch": torch, "np": rec, "getWorld2View2": getWorld2View2}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), scope)
    return scope["is_keyframe"], scope["add_to_window"], rec


def rot(g, angle):
    a = g.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose(g, centre, angle=0.2):
    Rm = rot(g, angle)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = Rm.astype(np.float32)
    T[:3, 3] = (-Rm @ np.asarray(centre)).astype(np.float32)
    return T


def away(x, th, what):
    assert np.isnan(x) or abs(float(x) - float(th)) >= 1e-3 * abs(float(th)), (what, x, th)


# name, K, window_size, check_time, single_thread, distance of cur from kf0, overlap of cur with kf0, kf spread, far keyframe
KF_CASES = [("k1_below_create", 1, 8, 1, 0, 0.02, 0.5, 0.3, None), ("k1_below_nocreate", 1, 8, 1, 0, 0.02, 0.98, 0.3, None),
            ("k1_below_notime", 1, 8, 0, 0, 0.02, 0.5, 0.3, None), ("k3_below_overlap", 3, 8, 1, 0, 0.02, 0.5, 0.3, None),
            ("k3_at_dist", 3, 3, 1, 0, 0.5, 0.98, 0.3, None), ("k3_at_overlap_min", 3, 3, 0, 0, 0.12, 0.5, 0.3, None),
            ("k3_at_neither", 3, 3, 1, 0, 0.02, 0.5, 0.3, None), ("k3_at_single_notime", 3, 3, 0, 1, 0.5, 0.98, 0.3, None),
            ("k10_at_both", 10, 10, 1, 0, 0.5, 0.5, 0.4, 7), ("k10_at_score", 10, 10, 1, 0, 0.5, 0.98, 0.4, None),
            ("k10_below_cut", 10, 12, 1, 0, 0.1, 0.5, 0.4, 4), ("k10_at_two_far", 10, 9, 1, 0, 0.5, 0.5, 0.4, 5)]
P = 1000
TRAIN = dict(kf_translation=0.08, kf_min_translation=0.05, kf_overlap=0.9, kf_cutoff=0.4)


def keyframe_cases(out):
    is_keyframe, add_to_window, rec = frontend_methods()
    names = []
    for ci, (name, K, wsize, check_time, single, d0, ov, spread, far) in enumerate(KF_CASES):
        g = np.random.default_rng(100 + ci)
        median = np.float32(2.0 + 0.37 * ci)
        centres = [np.array([0.0, 0.0, 0.0])] + [g.normal(size=3) * spread * float(median) for _ in range(K - 1)]
        kf = np.stack([pose(g, c) for c in centres])
        direction = g.normal(size=3)
        cur = pose(g, direction / np.linalg.norm(direction) * d0 * float(median), 0.05)
        base = g.random(P) < 0.6
        cur_vis = base.copy()
        flip = g.random(P) < (1 - ov) * 0.6
        cur_vis[flip] = ~cur_vis[flip]
        n_touched = (cur_vis * g.integers(1, 9, size=P)).astype(np.int32)
        vis = np.zeros((K, P), np.uint8)
        vis[0] = base
        for k in range(1, K):
            v = cur_vis.copy()
            f2 = g.random(P) < 0.25
            v[f2] = ~v[f2]
            vis[k] = v
        if far is not None:     # keyframes that share little with the tracked frame: candidates of the cut-off
            for k in ([far] if name != "k10_at_two_far" else [3, far]):
                vis[k] = (~cur_vis) & (g.random(P) < 0.8) | (cur_vis & (g.random(P) < 0.15))
        # the reference, on stub cameras
        fe = _Stub()
        fe.config = {"Training": dict(TRAIN, window_size=wsize)}
        fe.median_depth = torch.tensor(median)
        ids = [100 - 3 * k for k in range(K)]
        cur_id = 104
        fe.cameras = {}
        for i, T in zip(ids + [cur_id], list(kf) + [cur]):
            c = _Stub()
            c.R, c.T = torch.from_numpy(T[:3, :3].copy()), torch.from_numpy(T[:3, 3].copy())
            fe.cameras[i] = c
        curr_visibility = (torch.from_numpy(n_touched) > 0).long()
        occ = {i: torch.from_numpy(vis[k].astype(bool)) for k, i in enumerate(ids)}
        is_kf = bool(is_keyframe(fe, cur_id, ids[0], curr_visibility, occ))
        create = is_kf
        union = torch.logical_or(curr_visibility, occ[ids[0]]).count_nonzero()
        intersection = torch.logical_and(curr_visibility, occ[ids[0]]).count_nonzero()
        point_ratio = intersection / union
        if K < wsize:
            create = bool(check_time) and bool(point_ratio < TRAIN["kf_overlap"])
        if single:
            create = bool(check_time) and create
        rec.scores = None
        window, removed = add_to_window(fe, cur_id, curr_visibility, occ, list(ids))
        scores = rec.scores
        # dist and the cut-off ratios by the reference's statements
        pose_CW = getWorld2View2(fe.cameras[cur_id].R, fe.cameras[cur_id].T)
        last_WC = torch.linalg.inv(getWorld2View2(fe.cameras[ids[0]].R, fe.cameras[ids[0]].T))
        dist = torch.norm((pose_CW @ last_WC)[0:3, 3])
        cut = np.full(16, np.nan, np.float32)
        for k in range(1, K):
            inter = torch.logical_and(curr_visibility, occ[ids[k]]).count_nonzero()
            den = min(curr_visibility.count_nonzero(), occ[ids[k]].count_nonzero())
            cut[k] = (inter / den).item()
        # conditions on the inputs
        away(dist.item(), TRAIN["kf_translation"] * float(median), name + " dist")
        away(dist.item(), TRAIN["kf_min_translation"] * float(median), name + " dist min")
        away(point_ratio.item(), TRAIN["kf_overlap"], name + " overlap")
        for k in range(1, K):
            away(cut[k], TRAIN["kf_cutoff"], name + " cut")
        if scores is not None and len(scores) > 1:
            s = sorted(scores)
            assert s[-1] - s[-2] >= 1e-3 * s[-1], (name, s[-2:])
        keep = [ids.index(i) for i in window[1:]]
        removed_pos = [k for k in range(K) if k not in keep]
        out[f"kf_{name}_n_touched"], out[f"kf_{name}_vis"] = n_touched, vis
        out[f"kf_{name}_cur_pose"], out[f"kf_{name}_kf_poses"] = cur.reshape(16), kf.reshape(K, 16)
        out[f"kf_{name}_median"] = median
        out[f"kf_{name}_params"] = np.array([wsize, check_time, single], np.int32)
        out[f"kf_{name}_is_kf"], out[f"kf_{name}_create"] = np.int32(is_kf), np.int32(create)
        out[f"kf_{name}_keep"] = np.array(keep, np.int32)
        out[f"kf_{name}_removed"] = np.array(removed_pos, np.int32)
        out[f"kf_{name}_dist"], out[f"kf_{name}_ratio_u"] = np.float32(dist.item()), np.float32(point_ratio.item())
        out[f"kf_{name}_cut"] = cut
        # the scores of the window positions add_to_window scored, in its order (positions >= 2 of the window after the cut)
        out[f"kf_{name}_scores"] = np.array(scores if scores is not None else [], np.float64)
        names.append(name)
        print(f"kf {name}: is_kf {is_kf} create {create} removed {removed_pos} dist {dist.item():.4f} "
              f"(median {median:.2f}) ratio {point_ratio.item():.3f}")
    out["kf_names"] = np.array(names)
    out["kf_train"] = np.array([TRAIN["kf_translation"], TRAIN["kf_min_translation"], TRAIN["kf_overlap"], TRAIN["kf_cutoff"]])


def main():
    out = {}
    mask_cases(out)
    median_cases(out)
    keyframe_cases(out)
    np.savez_compressed(os.path.join(HERE, "frontend.npz"), **out)
    print("wrote frontend.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
