"""Keyframe seeding on the GPU (olsr_keyframe_seed_plan / _finish, keyframe_seed.seed_rows, GaussianMap.extend_from_rgbd)
against the numpy restatement tests/keyframe_seed_ref.py.

Inputs that make the comparison unambiguous: image values are multiples of 1/256 (the three-term sum is exact in any order);
under an exposure every c * 255 has a fractional part in [0.05, 0.95] (no byte flips on an ulp); depths lie in 0.3 .. 6 m.
Shapes: 40 x 24 (one partial workgroup), 67 x 45 (odd pixel count, rows no multiple of 64), 64 x 48 (even count),
200 x 150 (several workgroups in every kernel — eight histogram blocks, 118 emit blocks —, all radix passes live)."""
import os

import numpy as np
import pytest
import torch

import keyframe_seed_ref as R

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyframe_seed.npz"))
# a non-identity pose, as getWorld2View2 returns it (torch.linalg.inv leaves it column-major: the values, row-major)
W2C = np.ascontiguousarray(GOLD["pose1_w2c"], dtype=np.float32)
SHAPES = [(40, 24), (67, 45), (64, 48), (200, 150)]
EXPOSURE = np.array([0.1, 0.02], dtype=np.float32)
ROW_KEYS = ("means3D", "shs", "opacities", "scales", "rotations")


def _expf():
    from oracle import oracle_C
    return oracle_C.expf


def _intrinsics(W, H):
    return (W * 0.5 + 3.0, W * 0.5 - 2.0, W * 0.5 - 4.25, H * 0.5 + 2.5)   # cx, cy off-centre


def make_frame(W, H, seed, exposure=None, lo=0.3, hi=6.0):
    rng = np.random.default_rng(seed)
    k = np.arange(13, 244)
    if exposure is not None:
        c = R.f32(_expf()(float(exposure[0]))) * (k / 256.0).astype(np.float32) + exposure[1]
        frac = np.modf(np.clip(c, 0, 1).astype(np.float64) * 255.0)[0]
        k = k[(frac >= 0.05) & (frac <= 0.95)]
        assert k.size > 100
    image = (rng.choice(k, size=(3, H, W)) / 256.0).astype(np.float32)
    depth = rng.uniform(lo, hi, size=(H, W)).astype(np.float32)
    return image, depth


def run(image, depth, w2c, intr, dev="cuda", **kw):
    from online_lang_splatting_amd import seed_rows
    ex = kw.pop("exposure", None)
    out = seed_rows(torch.from_numpy(image).to(dev), torch.from_numpy(depth).to(dev), torch.from_numpy(w2c).to(dev), intr,
                    exposure=None if ex is None else torch.from_numpy(ex).to(dev), **kw)
    torch.cuda.synchronize()
    return out


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, ref, what):
    g, r = bits(got), bits(np.asarray(ref))
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), (what, int((g != r).sum()), g.size)


def check_plan(out, ref, M):
    assert int(out["n_valid"]) == ref["n_valid"]
    assert out["n_keep"] == ref["n_keep"]
    same_bits(out["median_depth"], np.float32(ref["median_depth"]), "median")
    same_bits(out["point_size"], np.float32(ref["point_size"]), "point_size")
    n = ref["n_keep"] if ref["n_keep"] >= 4 else 0
    assert out["means3D"].shape[0] == n
    if n:
        same_bits(out["pix_index"], ref["pix_index"], "pix_index")
        same_bits(out["means3D"], ref["means3D"], "means3D")
        same_bits(out["shs"], ref["shs"], "shs")
        assert tuple(out["shs"].shape) == (n, M, 3) and not out["shs"][:, 1:].any()
        same_bits(out["rotations"], ref["rotations"], "rotations")
        same_bits(out["opacities"], ref["opacities"], "opacities")


def check_scales(out, ref):
    """d2 and max(d2, 1e-7) ps are exact, so only logf can differ: the kernel stays within E_ref + 4 ulp (float32, at the
    value) of the float64 value, E_ref = what torch's CPU float32 log(sqrt(x)) misses it by on these points; 4 ulp = OpenCL's
    3 ulp for log plus the half ulp of the correctly rounded sqrt carried through.  Prints the worst error in ulp and returns it."""
    got = out["scales"].cpu().numpy()
    assert np.array_equal(got[:, 0].view(np.uint32), got[:, 1].view(np.uint32))
    assert np.array_equal(got[:, 0].view(np.uint32), got[:, 2].view(np.uint32))
    s64 = ref["scales64"]
    e_ref = float(np.abs(torch.log(torch.sqrt(torch.from_numpy(ref["scale_arg"]))).numpy().astype(np.float64) - s64).max())
    ulp = np.spacing(np.abs(s64.astype(np.float32))).astype(np.float64)
    err = np.abs(got[:, 0].astype(np.float64) - s64)
    print(f"scales: n = {got.shape[0]}, max error {float((err / ulp).max()):.3f} ulp, E_ref {e_ref:.3e}")
    assert np.all(err <= e_ref + 4.0 * ulp), float((err / ulp).max())
    return float((err / ulp).max())


_REF = {}


def reference(W, H, M, exposed):
    key = (W, H, M, exposed)
    if key not in _REF:
        ex = EXPOSURE if exposed else None
        image, depth = make_frame(W, H, 100 + W, ex)
        kw = dict(downsample=8, seed=7, exposure=ex, M=M)
        _REF[key] = (image, depth, kw, R.seed_rows_ref(image, depth, W2C, _intrinsics(W, H), expf=_expf(), **kw))
    return _REF[key]


@pytest.mark.parametrize("M,exposed", [(1, False), (16, True)])
@pytest.mark.parametrize("W,H", SHAPES)
def test_bit_exact_against_the_restatement(hip, W, H, M, exposed):
    image, depth, kw, ref = reference(W, H, M, exposed)
    out = run(image, depth, W2C, _intrinsics(W, H), **kw)
    assert ref["n_valid"] == W * H and ref["n_keep"] == W * H // 8
    check_plan(out, ref, M)
    check_scales(out, ref)


def test_identity_pose_and_centred_principal_point(hip):
    W, H = 67, 45
    image, depth = make_frame(W, H, 5)
    eye, intr = np.eye(4, dtype=np.float32), (W / 2.0, W / 2.0, (W - 1) / 2.0, (H - 1) / 2.0)
    kw = dict(downsample=8, seed=2)
    ref = R.seed_rows_ref(image, depth, eye, intr, **kw)
    out = run(image, depth, eye, intr, **kw)
    check_plan(out, ref, 1)
    check_scales(out, ref)


def test_image_with_a_plane_stride(hip):
    """The image is taken as it lies: three planes of a wider allocation."""
    W, H = 40, 24
    image, depth, kw, ref = reference(W, H, 1, False)
    big = torch.full((3, H + 5, W), float("nan"), device="cuda")
    big[:, :H] = torch.from_numpy(image).cuda()
    from online_lang_splatting_amd import seed_rows
    out = seed_rows(big[:, :H], torch.from_numpy(depth).cuda(), torch.from_numpy(W2C).cuda(), _intrinsics(W, H), **kw)
    check_plan(out, ref, 1)


@pytest.mark.parametrize("W,H", [(67, 45), (64, 48)])
def test_masks(hip, W, H):
    """A black border (rgb invalid), depth 0, depth exactly depth_trunc and the largest float below it, NaN, +inf and
    negative depth: none of the invalid pixels is kept, and the median counts them as 0 — for an odd and an even count."""
    image, depth = make_frame(W, H, 11)
    image[:, :3, :] = 0.0
    image[:, :, -2:] = 0.0
    image[:, 10, 10] = np.float32(1.0 / 256.0) * np.array([1, 1, 0], dtype=np.float32)   # sum 2/256 <= 0.01: invalid
    image[:, 10, 11] = np.float32(1.0 / 256.0) * np.array([1, 1, 1], dtype=np.float32)   # sum 3/256 > 0.01: valid
    below = np.nextafter(np.float32(100.0), np.float32(0.0))
    special = {(5, 5): 0.0, (5, 6): 100.0, (5, 7): below, (6, 5): np.nan, (6, 6): np.inf, (6, 7): -1.5, (6, 8): -np.inf,
               (7, 5): -0.0, (7, 6): 250.0}
    depth[np.random.default_rng(1).random((H, W)) < 0.1] = 0.0
    for (v, u), d in special.items():
        depth[v, u] = d
    depth[10, 10:12] = 2.0
    kw = dict(downsample=2, seed=3)
    ref = R.seed_rows_ref(image, depth, W2C, _intrinsics(W, H), **kw)
    out = run(image, depth, W2C, _intrinsics(W, H), **kw)
    check_plan(out, ref, 1)
    # the expectation, stated without the restatement
    rgb_ok = image.sum(axis=0) > 0.01
    with np.errstate(invalid="ignore"):
        valid = rgb_ok & (depth > 0) & (depth < 100.0)
    assert valid[5, 7] and valid[10, 11] and not valid[10, 10]
    for (v, u) in special:
        if (v, u) != (5, 7):
            assert not valid[v, u]
    assert int(out["n_valid"]) == int(valid.sum())
    pix = out["pix_index"].cpu().numpy()
    assert valid.ravel()[pix].all()
    with np.errstate(invalid="ignore"):
        d0 = np.where(rgb_ok & np.isfinite(depth) & (depth > 0), depth, np.float32(0.0)).astype(np.float32)
    assert d0[7, 6] == 250.0   # a finite depth past depth_trunc is invalid, but the median sees it as it is
    srt = np.sort(d0.ravel())
    N = W * H
    med = srt[N // 2] if N % 2 else np.float32(np.float32(srt[N // 2 - 1] + srt[N // 2]) / np.float32(2))
    same_bits(out["median_depth"], np.float32(med), "median")


def _sentinel_staging(cap, M=1):
    f = lambda *s: torch.full(s, 12345.0, device="cuda")   # noqa: E731
    return dict(means3D=f(cap, 3), shs=f(cap, M, 3), opacities=f(cap, 1), scales=f(cap, 3), rotations=f(cap, 4),
                pix_index=torch.full((cap,), -7, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("n_valid,factor,n_keep", [(960, 1, 960), (10, 64, 0), (8, 8, 1), (24, 8, 3), (32, 8, 4), (37, 1, 37)])
def test_count_edges(hip, n_valid, factor, n_keep):
    """Factor 1 keeps every valid pixel in pixel order; a factor larger than n_valid keeps none; n_keep of 1 and 3 append
    nothing (finish writes nothing); n_keep = 4 appends four rows.  Nothing is written past the rows in use."""
    W, H = 40, 24
    image, depth = make_frame(W, H, 21)
    rng = np.random.default_rng(n_valid)
    off = rng.permutation(W * H)[n_valid:]
    depth.ravel()[off] = 0.0
    cap = W * H // factor + 3
    st = _sentinel_staging(cap)
    kw = dict(downsample=factor, seed=9, adaptive_pointsize=False)   # (most depths are 0 here: the median is, too)
    ref = R.seed_rows_ref(image, depth, W2C, _intrinsics(W, H), **kw)
    out = run(image, depth, W2C, _intrinsics(W, H), staging=st, **kw)
    assert ref["n_valid"] == n_valid and ref["n_keep"] == n_keep
    check_plan(out, ref, 1)
    n_rows = n_keep if n_keep >= 4 else 0
    assert out["means3D"].shape[0] == n_rows
    if factor == 1:
        assert np.array_equal(out["pix_index"].cpu().numpy(), np.nonzero(depth.ravel() > 0)[0])
    # the plan wrote rows [0, n_keep) and nothing else; finish wrote scales [0, n_rows) and nothing else
    for k in ("means3D", "shs", "opacities", "rotations"):
        assert bool((st[k][n_keep:] == 12345.0).all()), k
        assert not bool((st[k][:n_keep] == 12345.0).any()), k
    assert bool((st["pix_index"][n_keep:] == -7).all())
    same_bits(st["pix_index"][:n_keep], ref["pix_index"], "pix_index of the plan")
    assert bool((st["scales"][n_rows:] == 12345.0).all())
    if n_rows:
        check_scales(out, ref)


@pytest.mark.parametrize("seed,key5,downsample,n_keep,kept", [(1015369654, 0xFFFFFFFF, 1, 64, True), (1015369654, 0xFFFFFFFF, 2, 32, False),
                                                             (1702866605, 0, 64, 1, True), (1702866605, 0, 16, 4, True)])
def test_extreme_sampling_keys(hip, seed, key5, downsample, n_keep, kept):
    """The sampling key is fmix32(i ^ seed * 0x9E3779B9), a bijection of the 32-bit words, so 0xFFFFFFFF and 0 are the keys of
    one pixel index each per seed, and both are keys like any other: the all-ones word must be counted by the select.  The
    seeds come from inverting the function for pixel 5: seed = (fmix32^-1(key) ^ 5) * 0x9E3779B9^-1 mod 2^32 (fmix32's steps
    are xor-shifts and odd multipliers, each invertible).  With 1015369654 pixel 5 has the largest key of the frame, 0xFFFFFFFF:
    kept when every valid pixel is, dropped at half; with 1702866605 it has the smallest, 0: the one pixel kept of 64, and
    one of four.  As in test_count_edges nothing is appended when n_keep < 4; pix_index is read from the staging buffer."""
    W, H = 8, 8
    image, depth = make_frame(W, H, 41)
    keys = R.sample_keys(W * H, seed)
    assert int(keys[5]) == key5 and int(keys.argmax() if key5 else keys.argmin()) == 5
    kw = dict(downsample=downsample, seed=seed)
    ref = R.seed_rows_ref(image, depth, W2C, _intrinsics(W, H), **kw)
    assert ref["n_valid"] == W * H and ref["n_keep"] == n_keep and (5 in ref["pix_index"]) == kept
    if n_keep == 1:
        assert ref["pix_index"].tolist() == [5]
    cap = W * H // downsample + 3
    runs = []
    for _ in range(2):
        st = _sentinel_staging(cap)
        out = run(image, depth, W2C, _intrinsics(W, H), staging=st, **kw)
        check_plan(out, ref, 1)
        same_bits(st["pix_index"][:n_keep], ref["pix_index"], "pix_index of the plan")
        assert bool((st["pix_index"][n_keep:] == -7).all())
        assert out["means3D"].shape[0] == (n_keep if n_keep >= 4 else 0)
        runs.append({k: bits(v).copy() for k, v in list(st.items()) + [(k, out[k]) for k in ("n_valid", "median_depth", "point_size")]})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), ("two runs differ", k)


def test_point_size(hip):
    W, H = 40, 24
    intr = _intrinsics(W, H)

    def one(lo, hi, zero_fraction=0.0, **kw):
        image, depth = make_frame(W, H, 31, lo=lo, hi=hi)
        if zero_fraction:
            depth.ravel()[np.random.default_rng(2).permutation(W * H)[:int(zero_fraction * W * H)]] = 0.0
        kw = dict(dict(downsample=8, seed=1), **kw)
        ref = R.seed_rows_ref(image, depth, W2C, intr, **kw)
        out = run(image, depth, W2C, intr, **kw)
        check_plan(out, ref, 1)
        return out, ref

    # adaptive, median < 1 m: ps = (float)(0.05 * median) < 0.05
    out, ref = one(0.3, 0.9)
    assert float(out["median_depth"]) < 1.0
    same_bits(out["point_size"], np.float32(0.05 * float(ref["median_depth"])), "ps")
    assert float(out["point_size"]) < np.float32(0.05)
    check_scales(out, ref)
    # adaptive, median >= 1 m: exactly 0.05f
    out, ref = one(1.5, 6.0)
    same_bits(out["point_size"], np.float32(0.05), "ps")
    check_scales(out, ref)
    # a point size that is not a float32 number times a median: the product is taken in double and narrowed once
    out, ref = one(0.3, 0.9, point_size=0.037)
    same_bits(out["point_size"], np.float32(0.037 * float(ref["median_depth"])), "ps")
    # more than half the depths invalid: median 0, ps = 0, max(d2, 1e-7) * 0 = 0 and every scale is log(0) = -inf, as in the
    # reference (the clamp keeps d2 positive; it cannot keep the product from vanishing)
    out, ref = one(0.3, 6.0, zero_fraction=0.6)
    assert float(out["median_depth"]) == 0.0 and float(out["point_size"]) == 0.0
    assert out["scales"].shape[0] == ref["n_keep"] >= 4 and bool(torch.isneginf(out["scales"]).all())
    # adaptive off: the configured size, narrowed
    out, ref = one(0.3, 0.9, adaptive_pointsize=False, point_size=0.037)
    same_bits(out["point_size"], np.float32(0.037), "ps")
    check_scales(out, ref)


def test_determinism(hip):
    W, H = 200, 150
    image, depth, kw, _ = reference(W, H, 1, False)
    keys = ROW_KEYS + ("pix_index", "n_valid", "median_depth", "point_size")
    a = run(image, depth, W2C, _intrinsics(W, H), **kw)
    b = run(image, depth, W2C, _intrinsics(W, H), **kw)
    for k in keys:
        same_bits(a[k], b[k].cpu().numpy(), k)
    c = run(image, depth, W2C, _intrinsics(W, H), **dict(kw, seed=8))
    assert c["n_keep"] == a["n_keep"]
    assert not np.array_equal(c["pix_index"].cpu().numpy(), a["pix_index"].cpu().numpy())


def test_default_staging_is_fully_written(hip):
    """seed_rows builds its rows in torch.empty buffers (so that OLSR_TEST_POISON=1 means something); here the same with
    the poison written by hand: every word of the returned rows is the restatement's."""
    W, H = 67, 45
    image, depth, kw, ref = reference(W, H, 16, True)
    cap = W * H // 8
    st = dict(means3D=torch.full((cap, 3), float("nan"), device="cuda"), shs=torch.full((cap, 16, 3), float("nan"), device="cuda"),
              opacities=torch.full((cap, 1), float("nan"), device="cuda"), scales=torch.full((cap, 3), float("nan"), device="cuda"),
              rotations=torch.full((cap, 4), float("nan"), device="cuda"),
              pix_index=torch.full((cap,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"))
    out = run(image, depth, W2C, _intrinsics(W, H), staging=st, **kw)
    check_plan(out, ref, 16)
    check_scales(out, ref)
    for k in ROW_KEYS:
        assert not bool(torch.isnan(out[k]).any()), k


LRS = dict(xyz=1.6e-4, sh_dc=2.5e-3, sh_rest=1.25e-4, opacity=0.05, scale=1e-3, rotation=1e-3, language=2.5e-3)


def _map(P=500, M=4, F=15):
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    g = torch.Generator().manual_seed(4)
    r = lambda *s: torch.randn(*s, generator=g).cuda()   # noqa: E731
    m = GaussianMap(r(P, 3), r(P, M, 3), r(P, 1), r(P, 3), r(P, 4), r(P, F), LRS, kf_id=torch.arange(P, dtype=torch.int32).cuda() % 5,
                    n_obs=torch.ones(P, dtype=torch.int32).cuda(), device="cuda")
    m.adam.exp_avg.copy_(r(P, m.layout.width))
    m.adam.exp_avg_sq.copy_(r(P, m.layout.width).abs())
    m.stats.copy_(r(P, 2).abs())
    m.max_radii.fill_(3)
    return m


def test_extend_from_rgbd(hip, monkeypatch):
    from online_lang_splatting_amd import seed_rows
    W, H, P, M, F = 200, 150, 500, 4, 15
    image, depth, _, _ = reference(W, H, 1, False)
    dev = dict(image=torch.from_numpy(image).cuda(), depth=torch.from_numpy(depth).cuda(), w2c=torch.from_numpy(W2C).cuda())
    intr = _intrinsics(W, H)
    for init, factor in ((True, 32), (False, 64)):
        m = _map(P, M, F)
        before = {k: v.clone() for k, v in m.state().items()}
        rows = seed_rows(dev["image"], dev["depth"], dev["w2c"], intr, downsample=factor, seed=11, M=M)
        n = rows["n_keep"]
        assert n == int(W * H * (1.0 / factor)) and rows["means3D"].shape[0] == n
        torch.cuda.synchronize()
        # one host synchronisation: count the .item() reads (and the other ways a tensor reaches the host)
        reads = []
        for name in ("item", "cpu", "tolist", "numpy"):
            orig = getattr(torch.Tensor, name)
            monkeypatch.setattr(torch.Tensor, name, (lambda o, nm: lambda self, *a, **k: (reads.append(nm), o(self, *a, **k))[1])(orig, name))
        src_index = m.extend_from_rgbd(dev["image"], dev["depth"], dev["w2c"], intr, 11, init=init)
        monkeypatch.undo()
        assert reads == ["item"], reads
        assert m.P == P + n
        after = m.state()
        for k in ROW_KEYS:   # the new rows equal seed_rows' bit for bit, the old rows are untouched
            same_bits(after[k][P:].reshape(n, -1), rows[k].reshape(n, -1).cpu().numpy(), k)
            same_bits(after[k][:P], before[k].cpu().numpy(), k)
        same_bits(after["language"][:P], before["language"].cpu().numpy(), "language")
        assert not after["language"][P:].any()
        assert bool((after["kf_id"][P:] == 11).all()) and torch.equal(after["kf_id"][:P], before["kf_id"])
        assert not after["n_obs"][P:].any() and torch.equal(after["n_obs"][:P], before["n_obs"])
        assert not after["exp_avg"][P:].any() and not after["exp_avg_sq"][P:].any()
        same_bits(after["exp_avg"][:P], before["exp_avg"].cpu().numpy(), "exp_avg")
        same_bits(after["exp_avg_sq"][:P], before["exp_avg_sq"].cpu().numpy(), "exp_avg_sq")
        assert not after["stats"].any() and not after["max_radii"].any()   # the accumulators of EVERY row are zeroed
        expect = torch.cat([torch.arange(P), -(torch.arange(n) + 1)]).to(torch.int32)
        assert torch.equal(src_index.cpu(), expect)
    # seed defaults to kf_id; an explicit downsample and seed are honoured
    m = _map(P, M, F)
    m.extend_from_rgbd(dev["image"], dev["depth"], dev["w2c"], intr, 3, downsample=8, seed=7)
    ref = reference(W, H, 1, False)[3]
    same_bits(m.params["means3D"][P:], ref["means3D"], "means3D")
    # fewer than four rows: nothing is appended, the map is left as it is
    m = _map(P, M, F)
    edits = m.edits
    few = dev["depth"].clone()
    few.view(-1)[200:] = 0.0
    src_index = m.extend_from_rgbd(dev["image"], few, dev["w2c"], intr, 3)   # 200 valid / 64 -> 3
    assert m.P == P and m.edits == edits and torch.equal(src_index.cpu(), torch.arange(P, dtype=torch.int32))
