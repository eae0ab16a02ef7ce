"""The front end's frame step on the GPU (olsr_grad_mask, olsr_median_depth, olsr_covisibility, olsr_keyframe_decide and their
host layer online_lang_splatting_amd.frontend) against the float32 numpy restatement tests/frontend_ref.py, bit for bit; a NaN
equals a NaN.  Every helper below runs its entry twice and requires identical bytes.

Shapes.  Mask: the golden shapes (one-pixel blocks, even and odd block sizes, margins on both sides), 33 x 65 with a plane stride
of W H + 3 from an unaligned base, one 680 x 1200 frame (blocks of 21 x 37, 8 margin rows and 16 margin columns, 200 histogram
workgroups in global mode).  Median: one element, one wave +- 1, one workgroup's chunk + 1, a frame.  Covisibility: one element,
one wave +- 1, two workgroups, 49 workgroups; no, one and sixteen keyframes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import frontend_ref as R
from test_frontend_ref_golden import GOLD, KFS, MASKS, kf_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
TRAIN = dict(zip(("kf_translation", "kf_min_translation", "kf_overlap", "kf_cutoff"), (float(v) for v in GOLD["kf_train"])))


def same(a, b):
    """equal bits, or both NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert same(x, y), "two runs differ"
    return a


def frame_image(seed, H, W):
    g = np.random.default_rng(seed)
    img = (g.integers(0, 256, size=(3, H, W)).astype(np.float32) / np.float32(255)).astype(np.float32)
    img[:, H // 3: H // 3 + H // 5, W // 4: W // 4 + W // 5] = np.float32(0.002)   # dark: `ok` fails around it
    return img


@functools.lru_cache(maxsize=None)
def mask_case(name):
    if name == "frame":
        return frame_image(31, 680, 1200), 4.0
    if name == "strided":
        return frame_image(32, 33, 65), 1.1
    return GOLD[f"mask_{name}_image"], float(GOLD[f"mask_{name}_thr"])


@functools.lru_cache(maxsize=None)
def mask_ref(name, mode):
    img, thr = mask_case(name)
    return (R.grad_mask_blocks if mode == "blocks" else R.grad_mask_global)(img, thr, np.float32)[0]


def gpu_mask(img, thr, mode, strided=False):
    from online_lang_splatting_amd import tracking_mask
    _, H, W = img.shape
    if strided:   # planes W H + 3 floats apart, the first float 4 bytes past the allocation's start
        ps = W * H + 3
        buf = torch.full((1 + 3 * ps,), float("nan"), device=DEV)
        t = buf[1:].as_strided((3, H, W), (ps, W, 1))
        t.copy_(torch.from_numpy(img))
    else:
        t = torch.from_numpy(img).to(DEV)

    def run():
        out = tracking_mask(t, thr, mode)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (1, H, W)
        return (out[0].cpu().numpy(),)
    return twice(run)[0]


@pytest.mark.parametrize("mode", ["blocks", "global"])
@pytest.mark.parametrize("name", MASKS + ["strided", "frame"])
def test_mask(name, mode):
    img, thr = mask_case(name)
    if mode == "blocks" and name == "strided":   # 33 x 65: blocks of 1 x 2, one margin row and one margin column
        assert img.shape[1] // 32 == 1 and img.shape[2] // 32 == 2
    got, want = gpu_mask(img, thr, mode, strided=(name == "strided")), mask_ref(name, mode)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])


def test_mask_out_argument_and_errors():
    from online_lang_splatting_amd import tracking_mask
    img, thr = mask_case("s85x131")
    t = torch.from_numpy(img).to(DEV)
    out = torch.empty(85, 131, device=DEV)
    assert tracking_mask(t, thr, "blocks", out=out) is out
    assert same(out.cpu().numpy(), mask_ref("s85x131", "blocks"))
    with pytest.raises(ValueError):
        tracking_mask(t, thr, "replica")
    with pytest.raises(ValueError):
        tracking_mask(t[:, :, ::2], thr)


def test_mask_feeds_the_tracking_loss():
    from online_lang_splatting_amd import losses, tracking_mask
    img, thr = mask_case("s85x131b")
    g = torch.Generator().manual_seed(5)
    H, W = img.shape[1:]
    gt = torch.from_numpy(img).to(DEV)
    image, depth = torch.rand(3, H, W, generator=g).to(DEV), (torch.rand(1, H, W, generator=g) * 4).to(DEV)
    opacity, gt_depth = torch.rand(1, H, W, generator=g).to(DEV), (torch.rand(H, W, generator=g) * 4).to(DEV)
    a = losses.tracking_loss(image, depth, opacity, gt, gt_depth, grad_mask=tracking_mask(gt, thr, "blocks"))
    b = losses.tracking_loss(image, depth, opacity, gt, gt_depth, grad_mask=torch.from_numpy(mask_ref("s85x131b", "blocks")).to(DEV))
    for k in ("loss", "dL_dimage", "dL_ddepth"):
        assert torch.equal(a[k], b[k]), k
    assert float(a["loss"][1]) > 0


def depth_case(N, seed):
    g = np.random.default_rng(seed)
    d = (g.integers(-8, 320, size=N) / np.float32(64)).astype(np.float32)   # ties, zeros, negatives
    if N > 8:
        d[g.integers(0, N)] = np.inf
        d[g.integers(0, N)] = np.nan
    o = (0.9 + 0.1 * g.random(N)).astype(np.float32)
    o[0], d[0] = 1.0, max(d[0], np.float32(0.5)) if np.isfinite(d[0]) else np.float32(0.5)   # one valid pixel at least
    return d, o, (g.random(N) > 0.3)


def gpu_median(d, o, m):
    from online_lang_splatting_amd import median_depth
    td, to = torch.from_numpy(d).to(DEV), torch.from_numpy(o).to(DEV)
    tm = None if m is None else torch.from_numpy(m).to(DEV)

    def run():
        med, n = median_depth(td, to, tm)
        torch.cuda.synchronize()
        return med.cpu().numpy(), n.cpu().numpy()
    med, n = twice(run)
    return med[0], int(n[0])


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 4097, 680 * 1200])
def test_median_depth(N):
    d, o, m = depth_case(N, N)
    for mask in (None, m, m.astype(np.uint8)):
        want, n = R.median_depth(d, o, mask)
        got, gn = gpu_median(d, o, mask)
        assert gn == n and same(np.float32(got), np.float32(want)), (N, got, want, gn, n)
    # nothing valid: NaN and 0 (the reference raises)
    got, gn = gpu_median(d, np.full(N, 0.5, np.float32), None)
    assert gn == 0 and np.isnan(got)
    got, gn = gpu_median(d, o, np.zeros(N, bool))
    assert gn == 0 and np.isnan(got)


@pytest.mark.parametrize("name", [str(n) for n in GOLD["med_names"]])
def test_median_depth_golden(name):
    m = GOLD[f"med_{name}_mask"]
    got, n = gpu_median(GOLD[f"med_{name}_depth"], GOLD[f"med_{name}_opacity"], m if m.size else None)
    assert n == int(GOLD[f"med_{name}_count"]) and same(np.float32(got), np.float32(GOLD[f"med_{name}_median"]))


ONE, BELOW_ONE, TWO, BELOW_TWO, INF = 0x3F800000, 0x3F7FFFFF, 0x40000000, 0x3FFFFFFF, 0x7F800000


def last_digit_keys(N, at_zero=None):
    """0x3F800000 + k, k a seeded permutation of 0 ... 255 repeated up to N elements: the keys differ in the last 8-bit digit
    only.  at_zero: the permutation is rotated so that this k stands at the elements 0, 256, ..."""
    k = np.random.default_rng(256).permutation(256)
    if at_zero is not None:
        k = np.roll(k, -int(np.nonzero(k == at_zero)[0][0]))
    return (ONE + k[np.arange(N) % 256]).astype(np.uint32)


def split(lo, n_lo, hi, n_hi):
    return np.array([lo] * n_lo + [hi] * n_hi, dtype=np.uint32)


# name -> (key bits, mask or None, the median's bits where they can be stated without the model, else None)
SELECT_DIGIT_CASES = {
    "last_digit_256": (last_digit_keys(256), None, 0x3F80007F),
    "last_digit_257_one_repeated": (last_digit_keys(257), None, None),
    "all_equal_65": (np.full(65, 0x40490FDB, dtype=np.uint32), None, 0x40490FDB),
    "left_of_low_carry": (split(BELOW_ONE, 32, ONE, 32), None, BELOW_ONE),
    "right_of_low_carry": (split(BELOW_ONE, 31, ONE, 33), None, ONE),
    "left_of_top_carry": (split(BELOW_TWO, 32, TWO, 32), None, BELOW_TWO),
    "right_of_top_carry": (split(BELOW_TWO, 31, TWO, 33), None, TWO),
    "inf_is_the_median": (split(INF, 40, ONE, 25), None, INF),
    # FE_CHUNK = 4096: element 4096 is the only one of the second histogram workgroup, and it decides between the two
    # middle candidates 0x3F80007F and 0x3F800080 (asserted against the model below)
    "second_workgroup_4097": (last_digit_keys(4097, at_zero=128), None, 0x3F800080),
    "second_workgroup_4097_masked": (last_digit_keys(4097, at_zero=127), np.arange(4097) % 3 != 2, 0x3F80007F),
}


@pytest.mark.parametrize("name", list(SELECT_DIGIT_CASES))
def test_median_depth_every_digit(name):
    """Depths built from bit patterns (opacity 1) so that the select's later passes decide: test_median_depth's depths are
    small integers over 64, whose low 16 key bits are zero.  Keys that differ in the last digit only, a repeated value, equal
    keys, a rank on either side of a 255 -> 0 carry into the next digit (low digits and the top one), +inf as the median, and
    two histogram workgroups whose second holds one element that the median depends on — with and without elements that
    take no part lying between those that do."""
    bits, mask, stated = SELECT_DIGIT_CASES[name]
    d, o = bits.view(np.float32), np.ones(bits.size, np.float32)
    want, n = R.median_depth(d, o, mask)
    assert n == (bits.size if mask is None else int(mask.sum()))
    if stated is not None:
        assert int(np.float32(want).view(np.uint32)) == stated, hex(int(np.float32(want).view(np.uint32)))
    if bits.size == 4097:   # without element 4096 the model selects the other middle candidate
        other, _ = R.median_depth(d[:4096], o[:4096], None if mask is None else mask[:4096])
        assert {int(np.float32(v).view(np.uint32)) for v in (want, other)} == {0x3F80007F, 0x3F800080}
        assert mask is None or (bool(mask[4096]) and not mask[2::3].any() and int(mask.sum()) == 4097 - 1365)
    got, gn = gpu_median(d, o, mask)
    print(name, "median bits", hex(int(np.float32(got).view(np.uint32))), "count", gn)
    assert gn == n and same(np.float32(got), np.float32(want)), (name, got, want, gn, n)


def gpu_decide(params, n_touched, vis, median, cur_pose, kf_poses):
    """olsr_covisibility + olsr_keyframe_decide through the C ABI -> (cur uint8 [P], counts int64 [33], record int32[8], float32[40])"""
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd._lib import check, lib
    L, K, P = lib(), len(vis), len(n_touched)
    nt = torch.from_numpy(np.ascontiguousarray(n_touched, dtype=np.int32)).to(DEV)
    tv = [torch.from_numpy(np.ascontiguousarray(v, dtype=np.uint8)).to(DEV) for v in vis]
    views = _abi.OlsrCovisViews(K=K)
    for k, t in enumerate(tv):
        views.vis[k] = t.data_ptr()
    med = torch.tensor([median], dtype=torch.float32, device=DEV)
    cp = torch.from_numpy(np.ascontiguousarray(cur_pose, dtype=np.float32).reshape(16)).to(DEV)
    kp = torch.from_numpy(np.ascontiguousarray(kf_poses, dtype=np.float32).reshape(K, 16)).to(DEV) if K else None
    p = _abi.OlsrKeyframeDecideParams(window_len=K, **{k: (float(v) if k.startswith("kf_") else int(v)) for k, v in params.items()})

    def run():
        cur = torch.full((P,), 7, dtype=torch.uint8, device=DEV)
        counts = torch.full((_abi.COVIS_COUNTS,), -1, dtype=torch.int64, device=DEV)
        rec = torch.full((_abi.KEYFRAME_RECORD_BYTES // 4,), -1, dtype=torch.int32, device=DEV)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(L.olsr_covisibility(P, nt.data_ptr(), C.byref(views), cur.data_ptr(), counts.data_ptr(), st))
        check(L.olsr_keyframe_decide(C.byref(p), counts.data_ptr(), med.data_ptr(), cp.data_ptr(), kp.data_ptr() if K else None,
                                     rec.data_ptr(), st))
        torch.cuda.synchronize()
        raw = rec.cpu().numpy()
        return cur.cpu().numpy(), counts.cpu().numpy(), raw[:8].copy(), raw[8:].view(np.float32).copy()
    return twice(run)


def check_decide(params, n_touched, vis, median, cur_pose, kf_poses):
    cur, counts, ri, rf = gpu_decide(params, n_touched, vis, median, cur_pose, kf_poses)
    wcur, wcounts = R.covisibility(n_touched, vis)
    assert np.array_equal(cur, wcur) and np.array_equal(counts, wcounts), (counts, wcounts)
    res = R.decide(params, wcounts, median, cur_pose, kf_poses, np.float32)
    wi, wf = R.record(res, wcounts, np.float32(median))
    assert np.array_equal(ri, wi), (ri, wi)
    assert same(rf, wf), (rf, wf)
    return res


@pytest.mark.parametrize("name", KFS)
def test_decide_golden(name):
    params, n_touched, vis, cur_pose, kf_poses, median = kf_inputs(name)
    res = check_decide(params, n_touched, vis, median, cur_pose, kf_poses)
    assert res["create"] == bool(GOLD[f"kf_{name}_create"]) and res["keep"] == [int(v) for v in GOLD[f"kf_{name}_keep"]]


def random_pose(g, scale):
    a = g.normal(size=3)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    ang = g.uniform(0.05, 0.6)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = (np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx).astype(np.float32)
    T[:3, 3] = (g.normal(size=3) * scale).astype(np.float32)
    return T


@pytest.mark.parametrize("P", [1, 63, 64, 65, 4097, 100003])
def test_covisibility_and_decide_sizes(P):
    for K in (0, 1, 16):
        g = np.random.default_rng(1000 * K + P)
        n_touched = (g.integers(0, 5, size=P) * (g.random(P) < 0.7)).astype(np.int32)
        vis = [((g.random(P) < 0.5) * g.integers(1, 255, size=P)).astype(np.uint8) for _ in range(K)]   # any nonzero byte counts
        kf = [random_pose(g, 1.5) for _ in range(K)]
        params = dict(window_size=8, check_time=1, single_thread=0, **TRAIN)
        res = check_decide(params, n_touched, vis, np.float32(2.5), random_pose(g, 1.5), kf)
        if K == 16 and P > 1000:
            assert res["removed_b"] >= 1      # a window over its size loses the best-scored keyframe
        if K == 0:
            assert not res["create"] and np.isnan(res["dist"])


def test_union_of_zero_and_nan_median():
    P, g = 500, np.random.default_rng(9)
    kf = [random_pose(g, 1.0) for _ in range(3)]
    params = dict(window_size=8, check_time=1, single_thread=0, **TRAIN)
    res = check_decide(params, np.zeros(P, np.int32), [np.zeros(P, np.uint8)] * 3, np.float32(2.0), random_pose(g, 1.0), kf)
    assert np.isnan(res["ratio_u"]) and np.all(np.isnan(res["cut"][1:3])) and not res["create"] and res["removed_a"] == -1
    res = check_decide(dict(params, window_size=3), np.ones(P, np.int32), [np.ones(P, np.uint8)] * 3, np.float32(np.nan),
                       random_pose(g, 1.0), kf)
    assert not res["is_kf"] and not res["create"]


@pytest.mark.parametrize("name", KFS)
def test_selector_replays_the_golden_sequences(name):
    from online_lang_splatting_amd import KeyframeSelector
    params, n_touched, vis, cur_pose, kf_poses, median = kf_inputs(name)
    K = len(vis)
    ids, cur_id = [100 - 3 * k for k in range(K)], 104
    sel = KeyframeSelector(params["window_size"], 4 if params["check_time"] else 5, TRAIN["kf_translation"],
                           TRAIN["kf_min_translation"], TRAIN["kf_overlap"], TRAIN["kf_cutoff"], bool(params["single_thread"]))
    for k in reversed(range(K)):
        sel.add_keyframe(ids[k], torch.from_numpy(kf_poses[k].reshape(4, 4)).to(DEV), torch.from_numpy(vis[k].astype(bool)).to(DEV))
    assert sel.window == ids
    depth = torch.full((8, 8), float(median), device=DEV)
    depth[0, :3] = 0.0   # invalid pixels do not move the median
    create, new_window, removed, rec = sel.observe(cur_id, torch.from_numpy(n_touched).to(DEV),
                                                   torch.from_numpy(cur_pose.reshape(4, 4)).to(DEV), depth, torch.ones(8, 8, device=DEV))
    keep = [int(v) for v in GOLD[f"kf_{name}_keep"]]
    assert create == bool(GOLD[f"kf_{name}_create"]) and rec["is_kf"] == bool(GOLD[f"kf_{name}_is_kf"])
    assert new_window == [cur_id] + [ids[k] for k in keep]
    assert sorted(removed) == sorted(ids[int(k)] for k in GOLD[f"kf_{name}_removed"])
    assert float(rec["median_depth"].item()) == float(median) and int(rec["count"].item()) == 61
    assert np.float32(rec["ratio_u"]).tobytes() == np.float32(GOLD[f"kf_{name}_ratio_u"]).tobytes()
    if create:   # committed: the new keyframe leads the window with the tracked frame's visibility
        assert sel.window == new_window and all(r not in sel.visibility for r in removed)
        assert np.array_equal(sel.visibility[cur_id].cpu().numpy(), (n_touched > 0).astype(np.uint8))
        keep_mask = torch.from_numpy(np.arange(len(n_touched)) % 3 != 0).to(DEV)
        sel.prune(keep_mask)
        assert all(v.numel() == int(keep_mask.sum()) for v in sel.visibility.values())
    else:
        assert sel.window == ids and cur_id not in sel.visibility
