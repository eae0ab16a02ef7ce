"""numpy restatement of the front end's frame step (include/olsr.h, "front end: the frame step"; csrc/k_frontend.hip): the
tracking mask, the median depth, the covisibility counts and the keyframe decision with the window policy.

Every function takes `f`: np.float32 restates the contract operation for operation (numpy rounds every elementwise float32
operation once and fuses nothing), np.float64 is the truth the tolerances are measured against.  The ratios are float32 in both
(they are compared bit for bit), and the discrete outcomes come with whichever precision was asked for."""
import numpy as np

F32 = np.float32
EPS_OK = np.float32(0.01)
MAX_VIEWS = 16


def intensity(image, f=F32):
    """image [3,H,W] -> the Scharr gradient intensity I [H,W]."""
    img = np.asarray(image, dtype=F32).astype(f)
    gray = ((img[0] + img[1]) + img[2]) / f(3)
    H, W = gray.shape
    p = np.pad(gray, 1, mode="reflect")

    def s(dy, dx):
        return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]

    c3, c10, inv32 = f(3), f(10), f(0.03125)
    gv = inv32 * (((c3 * s(-1, -1) + c10 * s(-1, 0)) + c3 * s(-1, 1)) - ((c3 * s(1, -1) + c10 * s(1, 0)) + c3 * s(1, 1)))
    gh = inv32 * (((c3 * s(-1, -1) + c10 * s(0, -1)) + c3 * s(1, -1)) - ((c3 * s(-1, 1) + c10 * s(0, 1)) + c3 * s(1, 1)))
    ok = np.ones((H, W), dtype=bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ok &= np.abs(s(dy, dx)) > f(EPS_OK)
    return np.where(ok, np.sqrt(gv * gv + gh * gh), f(0)).astype(f)


def lower_median(a):
    """The element of rank (n - 1) / 2 in ascending order: torch.median."""
    a = np.sort(np.asarray(a).ravel())
    return a[(a.size - 1) // 2]


def grad_mask_blocks(image, edge_threshold, f=F32):
    """-> (mask [H,W], I [H,W], th [H,W]): th is the threshold of a pixel's block, NaN on the margins (raw intensity there)."""
    I = intensity(image, f)
    H, W = I.shape
    bh, bw = H // 32, W // 32
    out, th = I.copy(), np.full((H, W), np.nan, dtype=f)
    et = f(F32(edge_threshold))
    for r in range(32):
        for c in range(32):
            sl = (slice(r * bh, (r + 1) * bh), slice(c * bw, (c + 1) * bw))
            t = f(lower_median(I[sl]) * et)
            th[sl] = t
            out[sl] = ((I[sl] > t) & (not (f(1) <= t))).astype(f)
    return out, I, th


def grad_mask_global(image, edge_threshold, f=F32):
    """-> (mask [H,W], I, th scalar)."""
    I = intensity(image, f)
    t = f(lower_median(I) * f(F32(edge_threshold)))
    return (I > t).astype(f), I, t


def median_depth(depth, opacity, mask=None):
    """-> (float32 lower median of the valid depths, or NaN; their count)."""
    d, o = np.asarray(depth, dtype=F32).ravel(), np.asarray(opacity, dtype=F32).ravel()
    valid = (d > 0) & (o > F32(0.95))
    if mask is not None:
        valid &= np.asarray(mask).ravel() != 0
    n = int(valid.sum())
    return (F32(lower_median(d[valid])) if n else F32(np.nan)), n


def covisibility(n_touched, vis):
    """-> (cur uint8 [P], counts int64 [33]): |cur|, then {|cur & vis_k|, |vis_k|} per k."""
    cur = np.asarray(n_touched) > 0
    counts = np.zeros(1 + 2 * MAX_VIEWS, dtype=np.int64)
    counts[0] = cur.sum()
    for k, v in enumerate(vis):
        v = np.asarray(v) != 0
        counts[1 + 2 * k] = (cur & v).sum()
        counts[2 + 2 * k] = v.sum()
    return cur.astype(np.uint8), counts


def _centre(T):
    """c = -(R^-1 t) in double from the float32 entries, R^-1 by cofactors (the operation order of the kernel)."""
    T = [[float(F32(v)) for v in row] for row in np.asarray(T).reshape(4, 4)]
    (r00, r01, r02, t0), (r10, r11, r12, t1), (r20, r21, r22, t2) = T[0], T[1], T[2]
    c00, c01, c02 = r11 * r22 - r12 * r21, r12 * r20 - r10 * r22, r10 * r21 - r11 * r20
    det = (r00 * c00 + r01 * c01) + r02 * c02
    i = 1.0 / det
    i00, i01, i02 = c00 * i, (r02 * r21 - r01 * r22) * i, (r01 * r12 - r02 * r11) * i
    i10, i11, i12 = c01 * i, (r00 * r22 - r02 * r20) * i, (r02 * r10 - r00 * r12) * i
    i20, i21, i22 = c02 * i, (r01 * r20 - r00 * r21) * i, (r00 * r11 - r01 * r10) * i
    return (-((i00 * t0 + i01 * t1) + i02 * t2), -((i10 * t0 + i11 * t1) + i12 * t2), -((i20 * t0 + i21 * t1) + i22 * t2))


def _rel_dist(A, cB, f):
    """|translation of A B^-1| = |R_A c_B + t_A|: the vector in double, narrowed to f once, the norm in f."""
    A = np.asarray(A).reshape(4, 4)
    tv = [f(((float(A[r, 0]) * cB[0] + float(A[r, 1]) * cB[1]) + float(A[r, 2]) * cB[2]) + float(A[r, 3])) for r in range(3)]
    return np.sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2])


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return F32(F32(num) / F32(den))


def decide(params, counts, median, cur_pose, kf_poses, f=F32):
    """params: window_size, check_time, single_thread, kf_translation, kf_min_translation, kf_overlap, kf_cutoff; the window
    length is len(kf_poses).  -> dict(create, is_kf, removed_a, removed_b, removals, dist, ratio_u, cut [16], score [16]
    (float64), keep: the window positions that stay, in order)."""
    K = len(kf_poses)
    counts = np.asarray(counts, dtype=np.int64)
    n_cur, median = int(counts[0]), F32(median)
    centres = [_centre(T) for T in kf_poses]
    c_cur = _centre(cur_pose)
    cut = np.full(MAX_VIEWS, np.nan, dtype=F32)
    score = np.full(MAX_VIEWS, np.nan, dtype=np.float64)
    removed_a = -1
    for k in range(1, K):
        cut[k] = _ratio(counts[1 + 2 * k], min(n_cur, int(counts[2 + 2 * k])))
        if cut[k] <= F32(params["kf_cutoff"]):
            removed_a = k
    left = [k for k in range(1, K) if k != removed_a]
    for i in left:
        k0 = float(np.sqrt(_rel_dist(kf_poses[i], c_cur, f)))
        total = 0.0
        for j in left:
            if j != i:
                total = total + 1.0 / float(_rel_dist(kf_poses[i], centres[j], f) + f(1e-6))
        score[i] = k0 * total
    dist, ratio_u = f(np.nan), F32(np.nan)
    if K > 0:
        dist = _rel_dist(cur_pose, centres[0], f)
        ratio_u = _ratio(counts[1], n_cur + int(counts[2]) - int(counts[1]))
    overlap = F32(params["kf_overlap"])
    is_kf = bool((ratio_u < overlap and dist > F32(params["kf_min_translation"]) * median)
                 or dist > F32(params["kf_translation"]) * median)
    create = is_kf
    if K < params["window_size"]:
        create = bool(params["check_time"]) and bool(ratio_u < overlap)
    if params["single_thread"]:
        create = bool(params["check_time"]) and create
    removed_b = -1
    if K + 1 - (removed_a >= 0) > params["window_size"] and left:
        removed_b = left[int(np.argmax([score[i] for i in left]))]
    keep = [k for k in range(K) if k not in (removed_a, removed_b)]
    return dict(create=create, is_kf=is_kf, removed_a=removed_a, removed_b=removed_b,
                removals=int(removed_a >= 0) + int(removed_b >= 0), dist=dist, ratio_u=ratio_u, cut=cut, score=score, keep=keep)


def record(res, counts, median):
    """The record olsr_keyframe_decide writes: (int32[8], float32[40])."""
    ri = np.array([res["create"], res["removals"], res["removed_a"], res["removed_b"], res["is_kf"], counts[0], counts[1], counts[2]],
                  dtype=np.int32)
    rf = np.zeros(40, dtype=F32)
    rf[0], rf[1], rf[2] = res["dist"], median, res["ratio_u"]
    rf[4:20], rf[20:36] = res["cut"], res["score"].astype(F32)
    return ri, rf
