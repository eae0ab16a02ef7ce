"""olsr_tsdf_* (HIP) and tsdf.TSDFVolume on the GPU.

Yardstick: tests/tsdf_ref.py, the float32 numpy restatement of the kernels' statements (pinned to the reference's own CPU path
by tests/test_tsdf_ref_golden.py).  The kernels evaluate the same float32 expressions in the same order, without FMA
contraction and with IEEE division, so every comparison here is torch.equal: the tsdf, the weights, every feature channel,
the surface points, their features and their order.  The one exception is label_points, whose similarities come from the
matrix-core decoder of lang_query and carry that module's tolerance (tests/test_gpu_lang_query.py): a label may differ from
the float64 evaluation's only where the best and second-best similarity are closer than that tolerance.
"""
import functools
import math

import numpy as np
import pytest
import torch

import tsdf_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = 0.04
DIMS = [(1, 1, 1), (5, 3, 70), (64, 1, 65), (42, 34, 38)]
IMAGES = [(64, 48), (61, 45)]          # (W, H)
FEATURES = [0, 3, 15, 32, "rgb"]
ORIGIN = np.array([-0.37, 0.21, 0.55])


def _bnds(dim):
    """Bounds that the constructor's ceil turns into `dim` voxels of VOXEL."""
    return np.stack([ORIGIN, ORIGIN + (np.array(dim) - 0.5) * VOXEL], axis=1)


def _rot_y(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])


@functools.lru_cache(maxsize=None)
def _views(dim, W, H, feature, seed=0):
    """Five views of the volume `dim`: (0) in front of it, (1) from the side with obs_weight 0.5, (2) facing away: every
    voxel is behind the camera, (3) with the camera centre ON a voxel inside the volume and no rotation: one voxel plane has
    cam_z == 0 exactly and the planes before it cam_z < 0, (4) with an opacity mask.  Every depth image has noise and zeros."""
    rng = np.random.default_rng(1000 * seed + 7 * W + dim[0])
    dimv, origin, voxel, _ = R.volume_geometry(_bnds(dim), VOXEL)
    assert tuple(dimv) == dim
    extent = np.array(dim) * VOXEL
    centre = origin.astype(np.float64) + 0.5 * extent
    back = 0.5 * extent[2] + 0.6
    K = np.array([[0.7 * W, 0.0, (W - 1) / 2.0], [0.0, 0.7 * W, (H - 1) / 2.0], [0.0, 0.0, 1.0]])

    def pose(Rm, t):
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = Rm, t
        return P
    # (3): the float32 position of voxel (X//2, Y//2, Z//2), computed as the kernel computes it
    mid = np.array([origin[k] + np.float32(dim[k] // 2) * np.float32(voxel) for k in range(3)], dtype=np.float32)
    poses = [pose(np.eye(3), centre - [0.0, 0.0, back]),
             pose(_rot_y(25.0), centre - _rot_y(25.0) @ [0.0, 0.0, back] + [0.02, -0.01, 0.0]),
             pose(_rot_y(180.0), centre - [0.0, 0.0, back]),
             pose(np.eye(3), mid.astype(np.float64)),
             pose(_rot_y(-12.0), centre - _rot_y(-12.0) @ [0.0, 0.0, back] + [-0.03, 0.02, 0.01])]
    base = [back, back, back, 0.25 * extent[2] + 0.05, back]
    out = []
    for k, P in enumerate(poses):
        depth = (base[k] + 0.08 * rng.normal(size=(H, W))).astype(np.float32)
        depth[rng.random((H, W)) < 0.07] = 0.0
        if feature == "rgb":
            colour = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        else:
            colour = rng.normal(size=(H, W, feature)).astype(np.float32)
        v = dict(color_im=colour, depth_im=depth, cam_intr=K, cam_pose=P, obs_weight=0.5 if k == 1 else 1.0)
        if k == 4:
            v.update(opacity=rng.random((H, W)).astype(np.float32), min_opacity=0.5)
        out.append(v)
    return tuple(out)


def _ref_integrate(ref, v, voxels=None):
    return ref.integrate(v["color_im"], v["depth_im"], v["cam_intr"], v["cam_pose"], v["obs_weight"], v.get("opacity"),
                         v.get("min_opacity", 0.0), voxels=voxels)


@functools.lru_cache(maxsize=None)
def _reference(dim, W, H, feature, n_views=5):
    """The restatement after the first n_views views (cycled beyond five), and per view the voxels it updated."""
    dimv, origin, voxel, _ = R.volume_geometry(_bnds(dim), VOXEL)
    ref = R.Volume(dimv, origin, voxel, feature)
    views = _views(dim, W, H, feature)
    hit = [_ref_integrate(ref, views[k % 5]) for k in range(n_views)]
    return ref, hit


def _volume(dim, feature):
    from online_lang_splatting_amd.tsdf import TSDFVolume
    vol = TSDFVolume(_bnds(dim), VOXEL, feature_dim=feature, device=DEV)
    assert vol.vol_dim == dim and np.array_equal(vol.vol_origin, R.volume_geometry(_bnds(dim), VOXEL)[1])
    return vol


def _device_view(v, layout="rows"):
    """The view with device tensors; layout "channels": the features as [F,H,W]."""
    d = dict(v)
    d["depth_im"] = torch.from_numpy(v["depth_im"]).to(DEV)
    c = torch.from_numpy(v["color_im"]).to(DEV)
    if layout == "channels" and c.dtype == torch.float32:   # (an "rgb" volume takes its uint8 colour as [H,W,3] only)
        c = c.permute(2, 0, 1).contiguous()
    d["color_im"] = c
    if "opacity" in v:
        d["opacity"] = torch.from_numpy(v["opacity"]).to(DEV)
    if c.dtype == torch.float32 and c.dim() == 3 and c.shape[-1] > 0:
        d["layout"] = layout
    return d


def _assert_equals_reference(vol, ref, label):
    t, w, f = ref.arrays()
    tsdf, feat = vol.get_volume()
    torch.cuda.synchronize()
    assert torch.equal(vol.weight.cpu(), torch.from_numpy(w)), f"{label}: weight"
    assert torch.equal(tsdf.cpu(), torch.from_numpy(t)), f"{label}: tsdf"
    if ref.F > 0:
        got = feat.cpu()
        assert got.shape == f.shape
        if ref.packed:
            assert torch.equal(got, torch.from_numpy(f)), f"{label}: packed colour"
        else:
            for c in range(ref.F):
                assert torch.equal(got[c], torch.from_numpy(f[c])), f"{label}: feature channel {c}"
    else:
        assert feat is None


@pytest.mark.parametrize("feature", FEATURES)
@pytest.mark.parametrize("image", IMAGES)
@pytest.mark.parametrize("dim", DIMS)
def test_integrate_equals_the_restatement(hip, dim, image, feature):
    W, H = image
    views = _views(dim, W, H, feature)
    ref, hit = _reference(dim, W, H, feature)
    n = int(np.prod(dim))
    print(f"{dim} {W}x{H} F={feature}: voxels updated per view {[len(h) for h in hit]} of {n}")
    assert len(hit[2]) == 0                                   # the view that faces away touches nothing
    if n > 1000:
        assert all(len(hit[k]) > 0.02 * n for k in (0, 1, 3, 4)) and len(hit[3]) < n
        assert int((ref.weight == 0).sum()) > 0 and len(np.unique(ref.weight)) > 4
    # numpy arrays as the reference's callers pass them ([H,W,F]), one call per view
    vol = _volume(dim, feature)
    for v in views:
        vol.integrate(**v)
    _assert_equals_reference(vol, ref, "numpy [H,W,F]")
    # device tensors in both layouts
    layouts = ("rows", "channels") if feature not in (0, "rgb") else ("rows",)
    for layout in layouts:
        vol = _volume(dim, feature)
        for v in views:
            vol.integrate(**_device_view(v, layout))
        _assert_equals_reference(vol, ref, f"device {layout}")


def test_camera_plane_and_voxels_behind_it_are_skipped(hip):
    """View 3's camera sits on voxel (X//2, Y//2, Z//2) with no rotation: the plane z = Z//2 has cam_z == 0 exactly (the
    reference kernel would divide by it and convert the result to int), the planes below it cam_z < 0."""
    dim, (W, H) = (42, 34, 38), IMAGES[1]
    dimv, origin, voxel, _ = R.volume_geometry(_bnds(dim), VOXEL)
    ref = R.Volume(dimv, origin, voxel, 3)
    v = _views(dim, W, H, 3)[3]
    hit = _ref_integrate(ref, v)
    z = hit % dim[2]
    assert len(hit) > 100 and dim[2] // 2 < int(z.min()) <= dim[2] // 2 + 2
    vol = _volume(dim, 3)
    vol.integrate(**v)
    _assert_equals_reference(vol, ref, "camera inside")
    assert float(vol.weight[:, :, :dim[2] // 2 + 1].abs().sum()) == 0.0


@pytest.mark.parametrize("feature", [15, "rgb"])
def test_a_batch_equals_single_calls_bit_for_bit(hip, feature):
    dim, (W, H) = (42, 34, 38), IMAGES[1]
    views = [_device_view(v, "channels") for v in _views(dim, W, H, feature)]
    single, batch = _volume(dim, feature), _volume(dim, feature)
    for v in views:
        single.integrate(**v)
    batch.integrate_views(views)
    torch.cuda.synchronize()
    for a, b in zip((single.weight,) + single.get_volume(), (batch.weight,) + batch.get_volume()):
        assert torch.equal(a, b)
    _assert_equals_reference(batch, _reference(dim, W, H, feature)[0], "batch of 5")


def test_seventeen_views_are_chunked(hip):
    """integrate_views with more views than one launch takes (OLSR_TSDF_MAX_VIEWS = 16), as tuples."""
    from online_lang_splatting_amd import _abi
    assert _abi.TSDF_MAX_VIEWS == 16
    dim, (W, H), F = (5, 3, 70), IMAGES[0], 3
    views = _views(dim, W, H, F)
    ref, _ = _reference(dim, W, H, F, 17)
    frames = [(views[k % 5]["color_im"], views[k % 5]["depth_im"], views[k % 5]["cam_intr"], views[k % 5]["cam_pose"],
               views[k % 5]["obs_weight"], views[k % 5].get("opacity"), views[k % 5].get("min_opacity", 0.0)) for k in range(17)]
    vol, single = _volume(dim, F), _volume(dim, F)
    vol.integrate_views(frames)
    for f in frames:
        single.integrate(*f)
    _assert_equals_reference(vol, ref, "17 views")
    _assert_equals_reference(single, ref, "17 single calls")


@pytest.mark.parametrize("feature", [15, "rgb"])
def test_voxels_no_view_reaches_are_not_written(hip, feature):
    dim, (W, H) = (42, 34, 38), IMAGES[0]
    ref, _ = _reference(dim, W, H, feature)
    t, w, f = ref.arrays()
    untouched = torch.from_numpy(w == 0).to(DEV)
    assert 0 < int(untouched.sum()) < untouched.numel()
    vol = _volume(dim, feature)
    tsdf, feat = vol.get_volume()
    canary = float("nan")
    tsdf[untouched], vol.weight[untouched] = canary, canary
    if feature == "rgb":
        feat[untouched] = canary
    else:
        feat[:, untouched] = canary
    vol.integrate_views([_device_view(v) for v in _views(dim, W, H, feature)])
    torch.cuda.synchronize()
    planes = feat.reshape(-1, *dim)
    assert bool(tsdf[untouched].isnan().all()) and bool(vol.weight[untouched].isnan().all())
    assert bool(planes[:, untouched].isnan().all())
    touched = ~untouched
    assert torch.equal(tsdf[touched].cpu(), torch.from_numpy(t)[touched.cpu()])
    fr = torch.from_numpy(f).reshape(-1, *dim)
    assert torch.equal(planes[:, touched].cpu(), fr[:, touched.cpu()])


def test_a_volume_beyond_2_to_the_31_feature_elements(hip):
    """72 M voxels of 32 channels: linear voxel indices above 2^24 (where the reference kernel's (float)voxel_idx loses the
    coordinates) and feature offsets c * N + idx above 2^31.  One narrow view near the far corner reaches a few hundred voxels
    inside a 20^3 box; the restatement runs on that box, and nothing outside it may have been touched."""
    from online_lang_splatting_amd.tsdf import TSDFVolume
    dim, voxel, F = (300, 300, 800), 0.01, 32
    n = int(np.prod(dim))
    assert n > 1 << 26 and (F - 1) * n > 1 << 31
    origin = np.array([-1.0, -1.0, 0.5])
    bnds = np.stack([origin, origin + (np.array(dim) - 0.5) * voxel], axis=1)
    rng = np.random.default_rng(11)
    W, H = 61, 45
    K = np.array([[100.0, 0.0, 30.0], [0.0, 100.0, 22.0], [0.0, 0.0, 1.0]])
    pose = np.eye(4)
    pose[:3, :3] = _rot_y(90.0)                                  # the camera looks along +x
    pose[:3, 3] = origin + (np.array([282, 150, 400]) + 0.3) * voxel
    depth = (0.08 + 0.01 * rng.normal(size=(H, W))).astype(np.float32)
    depth[rng.random((H, W)) < 0.05] = 0.0
    lang = rng.normal(size=(F, H, W)).astype(np.float32)
    box = np.stack(np.meshgrid(np.arange(280, 300), np.arange(140, 160), np.arange(390, 410), indexing="ij"), axis=-1).reshape(-1, 3)
    voxels = (box[:, 0] * dim[1] + box[:, 1]) * dim[2] + box[:, 2]
    dimv, o32, vs, _ = R.volume_geometry(bnds, voxel)
    assert tuple(dimv) == dim
    # the restatement on the box only (its arrays are indexed by the global voxel index: keep them sparse)
    ref = R.Volume((1, 1, 1), o32, vs, F)
    ref.dim = dim
    ref.tsdf, ref.weight, ref.feat = (_Sparse(1.0), _Sparse(0.0), _SparseRows(F))
    hit = ref.integrate(lang, depth, K, pose, 1.0, layout="channels", voxels=voxels)
    x, y, z = hit // (dim[1] * dim[2]), (hit // dim[2]) % dim[1], hit % dim[2]
    print(f"large volume: {len(hit)} voxels updated, x {x.min()}..{x.max()}, y {y.min()}..{y.max()}, z {z.min()}..{z.max()}")
    assert len(hit) > 100 and int(hit.min()) > 1 << 26
    # the frustum stays clear of the box's faces (x = 299 is the volume's last plane), so the box holds every touched voxel
    assert x.min() > 280 and 140 < y.min() and y.max() < 159 and 390 < z.min() and z.max() < 409
    vol = TSDFVolume(bnds, voxel, feature_dim=F, device=DEV)
    vol.integrate(torch.from_numpy(lang).to(DEV), torch.from_numpy(depth).to(DEV), K, pose, layout="channels")
    tsdf, feat = vol.get_volume()
    torch.cuda.synchronize()
    assert int((vol.weight != 0).sum()) == len(hit) and int((tsdf != 1).sum()) <= len(hit)
    assert int((feat != 0).sum()) == F * len(hit)
    idx = torch.from_numpy(hit).to(DEV)
    assert torch.equal(vol.weight.reshape(-1)[idx].cpu(), torch.from_numpy(ref.weight[hit]))
    assert torch.equal(tsdf.reshape(-1)[idx].cpu(), torch.from_numpy(ref.tsdf[hit]))
    assert torch.equal(feat.reshape(F, -1)[:, idx].cpu(), torch.from_numpy(ref.feat[:, hit]))


class _Sparse:
    """A float32 array over every voxel index that stores only what was written (the rest holds `fill`)."""

    def __init__(self, fill):
        self.fill, self.d, self.dtype = np.float32(fill), {}, np.dtype(np.float32)

    def __getitem__(self, idx):
        return np.array([self.d.get(int(i), self.fill) for i in idx], np.float32)

    def __setitem__(self, idx, val):
        for i, v in zip(idx, np.asarray(val, np.float32)):
            self.d[int(i)] = v


class _SparseRows:
    def __init__(self, F):
        self.rows, self.dtype = [_Sparse(0.0) for _ in range(F)], np.dtype(np.float32)

    def __getitem__(self, key):
        c, idx = key
        if isinstance(c, slice):
            return np.stack([r[idx] for r in self.rows])
        return self.rows[c][idx]

    def __setitem__(self, key, val):
        c, idx = key
        self.rows[c][idx] = val


# ---- the surface point cloud -------------------------------------------------------------------------------------------------
def _assert_surface(vol, arrays, packed, min_weight, label):
    t, w, f = arrays
    want = R.surface(t, w, f, vol.vol_origin, VOXEL, min_weight, packed)
    points, feats, index = vol.surface_points(min_weight)
    torch.cuda.synchronize()
    print(f"{label}: {len(want[2])} surface points (min_weight {min_weight})")
    assert points.shape[0] == len(want[2]) and index.dtype == torch.int32
    assert torch.equal(index.cpu(), torch.from_numpy(want[2])), f"{label}: order"
    assert torch.equal(points.cpu(), torch.from_numpy(want[0])), f"{label}: points"
    if want[1].shape[1]:
        assert torch.equal(feats.cpu(), torch.from_numpy(want[1])), f"{label}: feats"
    else:
        assert feats is None
    cloud = vol.get_point_cloud(min_weight)
    assert tuple(cloud.shape) == (len(want[2]), 3 + want[1].shape[1])
    assert torch.equal(cloud[:, :3], points) and (feats is None or torch.equal(cloud[:, 3:], feats))
    return want


@pytest.mark.parametrize("min_weight", [0.0, 1.0])
@pytest.mark.parametrize("feature", [0, 15, "rgb"])
def test_surface_of_a_fused_volume(hip, feature, min_weight):
    dim, (W, H) = (42, 34, 38), IMAGES[0]
    ref, _ = _reference(dim, W, H, feature)
    vol = _volume(dim, feature)
    vol.integrate_views([_device_view(v) for v in _views(dim, W, H, feature)])
    want = _assert_surface(vol, ref.arrays(), feature == "rgb", min_weight, f"fused F={feature}")
    assert len(want[2]) > 500
    if min_weight == 0.0:   # edges to unobserved voxels (tsdf 1, weight 0) count only without a weight bound
        assert len(want[2]) > len(R.surface(*ref.arrays(), vol.vol_origin, VOXEL, 1.0, feature == "rgb")[2])


# (65, 64, 65): 1057 blocks of 256 voxels, more than the 1024 block counts one round of the surface prefix handles
@pytest.mark.parametrize("dim", [(1, 1, 1), (5, 3, 70), (64, 1, 65), (65, 64, 65)])
@pytest.mark.parametrize("feature", [3, "rgb"])
def test_surface_of_a_random_volume_reaches_the_last_planes(hip, dim, feature):
    """Random signs: crossings on every kind of edge, those that end on the last plane of each axis included, over several
    blocks of a size that is no multiple of the block."""
    rng = np.random.default_rng(5)
    t = rng.uniform(-1, 1, dim).astype(np.float32)
    w = rng.integers(0, 3, dim).astype(np.float32)
    f = (rng.integers(0, 1 << 24, dim).astype(np.float32) if feature == "rgb" else rng.normal(size=(3,) + dim).astype(np.float32))
    vol = _volume(dim, feature)
    tsdf, feat = vol.get_volume()
    tsdf.copy_(torch.from_numpy(t))
    vol.weight.copy_(torch.from_numpy(w))
    feat.copy_(torch.from_numpy(f))
    for mw in (0.0, 1.0):
        want = _assert_surface(vol, (t, w, f), feature == "rgb", mw, f"random {dim}")
    pts, _, own = R.surface(t, w, f, vol.vol_origin, VOXEL, 0.0, feature == "rgb")
    if dim == (1, 1, 1):
        assert len(own) == 0
        return
    X, Y, Z = dim
    x, y, z = own // (Y * Z), (own % (Y * Z)) // Z, own % Z
    # an owner on the last-but-one plane of an axis whose point moved along that axis ends on the last plane
    grid = (pts - vol.vol_origin) / np.float32(VOXEL)
    for axis, (c, n) in enumerate(((x, X), (y, Y), (z, Z))):
        if n > 1:
            assert bool(((c == n - 2) & (grid[:, axis] > n - 2 + 1e-3)).any()), axis
        assert not bool((grid[:, axis] > n - 1 + 1e-3).any())


def test_surface_of_an_empty_volume(hip):
    vol = _volume((5, 3, 70), 15)
    points, feats, index = vol.surface_points()
    assert tuple(points.shape) == (0, 3) and tuple(feats.shape) == (0, 15) and tuple(index.shape) == (0,)
    assert tuple(vol.get_point_cloud(1.0).shape) == (0, 18)


# ---- labels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_label_points(hip, n):
    import lang_codec_ref as RC
    import lang_query_ref as Q
    from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec
    from online_lang_splatting_amd.lang_query import LanguageDecoder, LanguageQuery
    from online_lang_splatting_amd.tsdf import TSDFVolume, label_points
    from test_lang_query_ref_golden import golden_case
    case, _, _ = golden_case(Q.golden(), "direct")            # the decoder fixtures of tests/test_gpu_lang_query.py
    codec = OnlineLanguageCodec(DEV, seed=0)
    codec.load_state_dict(RC.unflatten(case["online"]))
    q = LanguageQuery(LanguageDecoder(DEV, case["dec_state"]), codec)
    q.set_phrases(case["pos"].to(DEV), case["neg"].to(DEV))
    q.set_labels(case["labels"].to(DEV))
    n_pos, n_lab = case["pos"].shape[0], case["labels"].shape[0]
    feats = case["codes"].reshape(15, -1)[:, 500:500 + n].t().contiguous()   # [n,15] rows, as surface_points returns them
    assert tuple(feats.shape) == (n, 15)
    got = label_points(q, feats.to(DEV))
    assert got.dtype == torch.int64 and tuple(got.shape) == (n,)
    assert torch.equal(got, TSDFVolume.label_points(q, feats.to(DEV)))
    # torch ops: decode, products with the label rows, argmax (the softmax of get_semantic_map_pc is monotone)
    sims = {dt: Q.similarities(feats.t().reshape(15, 1, n), case["online"], case["dec_state"], case["labels"], dt)[:, 0, :]
            for dt in (torch.float64, torch.float32)}
    want = torch.argmax(torch.softmax(10 * sims[torch.float64].T, dim=-1), dim=-1)
    top = sims[torch.float64].T.topk(2, dim=-1).values
    margin = top[:, 0] - top[:, 1]
    tol = Q.tolerance(sims[torch.float64], sims[torch.float32])
    differs = got.cpu() != want
    print(f"label_points n={n}: {int(differs.sum())} labels differ from the float64 argmax; tolerance {tol:.3e}, smallest margin "
          f"{float(margin.min()):.3e}; labels used {sorted(set(want.tolist()))}")
    assert int((differs & (margin > tol)).sum()) == 0
    assert int((margin <= tol).sum()) <= max(1, n // 100)
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        label_points(q, feats)
    with pytest.raises(RuntimeError, match=r"expected \[N,15\]"):
        label_points(q, feats[:, :14].contiguous().to(DEV))
    q.set_labels(None)
    with pytest.raises(RuntimeError, match="set_labels first"):
        label_points(q, feats.to(DEV))


# ---- rendered maps -----------------------------------------------------------------------------------------------------------
def test_integrate_render_on_a_room_scene(hip):
    """Two keyframes of a small room: the rasteriser's language, depth and opacity maps go into the volume as they are."""
    from types import SimpleNamespace

    from online_lang_splatting_amd import render
    from online_lang_splatting_amd.scene import make_room_scene, world2view2
    from online_lang_splatting_amd.tsdf import TSDFVolume, get_view_frustum
    from test_gpu_api import _Model, _view
    dev = torch.device(DEV)
    W, H, F = 160, 96, 15
    rs = make_room_scene(20_000, W, H, F, views=2, seed=4)
    pipe = SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False)
    pkgs, Ks, w2cs = [], [], []
    bnds = np.zeros((3, 2))
    for k in range(2):
        sc = rs.view(k)
        cam = sc.camera
        pkg = render(_view(sc, dev), _Model(sc, dev), pipe, sc.bg.to(dev))
        assert tuple(pkg["language"].shape) == (F, H, W) and tuple(pkg["depth"].shape) == (1, H, W)
        K = np.array([[cam.fx, 0.0, cam.cx], [0.0, cam.fy, cam.cy], [0.0, 0.0, 1.0]])
        w2c = world2view2(cam.R, cam.T).numpy()
        fr = get_view_frustum(pkg["depth"][0].detach(), K, np.linalg.inv(w2c))   # dim15_recon.py:46-48
        bnds[:, 0] = np.minimum(bnds[:, 0], fr.min(axis=1))
        bnds[:, 1] = np.maximum(bnds[:, 1], fr.max(axis=1))
        pkgs.append(pkg), Ks.append(K), w2cs.append(w2c)
    a = TSDFVolume(bnds, 0.1, feature_dim=F, device=DEV)
    b = TSDFVolume(bnds, 0.1, feature_dim=F, device=DEV)
    assert int(np.prod(a.vol_dim)) < 2_000_000
    for k in range(2):
        a.integrate_render(pkgs[k], Ks[k], w2cs[k], min_opacity=0.5)
    b.integrate_views([dict(color_im=pkgs[k]["language"].detach(), depth_im=pkgs[k]["depth"].detach()[0], cam_intr=Ks[k],
                            cam_pose=np.linalg.inv(w2cs[k]), opacity=pkgs[k]["opacity"].detach()[0], min_opacity=0.5,
                            layout="channels") for k in range(2)])
    torch.cuda.synchronize()
    for x, y in zip((a.weight,) + a.get_volume(), (b.weight,) + b.get_volume()):
        assert torch.equal(x, y)
    assert float(a.weight.max()) == 2.0                      # some voxels are seen from both keyframes
    cloud = a.get_point_cloud()
    print(f"room scene: volume {a.vol_dim}, {cloud.shape[0]} surface points")
    assert cloud.shape[0] > 100 and cloud.shape[1] == 3 + F and bool(torch.isfinite(cloud).all())
    lo, hi = torch.from_numpy(a.vol_bnds[:, 0]).to(dev), torch.from_numpy(a.vol_bnds[:, 1]).to(dev)
    assert bool(((cloud[:, :3] >= lo - 1e-4) & (cloud[:, :3] <= hi + 1e-4)).all())
    # sensor depth in place of the rendered one (what the reference fuses)
    c = TSDFVolume(bnds, 0.1, feature_dim=F, device=DEV)
    c.integrate_render(pkgs[0], Ks[0], w2cs[0], depth=rs.targets[0][1].to(dev), min_opacity=0.0)
    assert float(c.weight.sum()) > 0.0


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_errors_are_raised_with_the_offending_name(hip):
    from online_lang_splatting_amd.tsdf import TSDFVolume
    dim, (W, H) = (5, 3, 70), IMAGES[0]
    v = _views(dim, W, H, 15)[0]
    d = _device_view(v)
    with pytest.raises(RuntimeError, match="GPU device is required"):
        TSDFVolume(_bnds(dim), VOXEL, device="cpu")
    with pytest.raises(RuntimeError, match=r"vol_bnds has shape \(2, 3\)"):
        TSDFVolume(np.zeros((2, 3)), VOXEL, device=DEV)
    with pytest.raises(RuntimeError, match="feature_dim must be"):
        TSDFVolume(_bnds(dim), VOXEL, feature_dim=7, device=DEV)
    with pytest.raises(RuntimeError, match="voxel_size must be positive"):
        TSDFVolume(_bnds(dim), 0.0, device=DEV)
    vol = _volume(dim, 15)
    with pytest.raises(RuntimeError, match="integrate: depth_im must be a float32 tensor on the GPU"):
        vol.integrate(**dict(d, depth_im=torch.from_numpy(v["depth_im"])))           # a CPU tensor
    with pytest.raises(RuntimeError, match="integrate: color_im must be a float32 tensor on the GPU"):
        vol.integrate(**dict(d, color_im=d["color_im"].double()))                    # the wrong dtype
    with pytest.raises(RuntimeError, match=r"integrate: color_im has shape \(48, 64, 14\)"):
        vol.integrate(**dict(d, color_im=d["color_im"][..., :14]))                   # the wrong shape
    with pytest.raises(RuntimeError, match=r"integrate: opacity has shape \(47, 64\)"):
        vol.integrate(**dict(d, opacity=torch.ones(47, 64, device=DEV)))
    with pytest.raises(RuntimeError, match=r"integrate: cam_pose has shape \(3, 4\)"):
        vol.integrate(**dict(d, cam_pose=np.eye(4)[:3]))
    with pytest.raises(RuntimeError, match=r"integrate: cam_intr has shape \(4, 4\)"):
        vol.integrate(**dict(d, cam_intr=np.eye(4)))
    with pytest.raises(RuntimeError, match="color_im is required"):
        vol.integrate(**dict(d, color_im=None))
    with pytest.raises(RuntimeError, match=r"integrate_views\[1\]: depth_im must be an \[H,W\] image"):
        vol.integrate_views([d, dict(d, depth_im=d["depth_im"][0])])
    with pytest.raises(RuntimeError, match=r"integrate_views\[0\]: a tuple"):
        vol.integrate_views([42])
    with pytest.raises(RuntimeError, match="the dict render"):
        vol.integrate_render({"language": d["color_im"]}, v["cam_intr"], np.eye(4))
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="depth_im is on cuda:1"):
            vol.integrate(**dict(d, depth_im=d["depth_im"].to("cuda:1")))
    # nothing above reached the volume
    assert float(vol.weight.abs().sum()) == 0.0 and float((vol.get_volume()[0] - 1).abs().sum()) == 0.0
    # the C-ABI's own checks
    import ctypes as C

    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd._lib import lib
    L = lib()
    bad = _abi.OlsrTsdfVolume(X=4, Y=4, Z=4, F=7, voxel_size=0.1, trunc_margin=0.5, tsdf=0x1000, weight=0x1000, feat=0x1000)
    assert L.olsr_tsdf_init(C.byref(bad), None) == _abi.OLSR_ERR_ARG and b"F must be one of" in L.olsr_last_error()
    assert L.olsr_tsdf_integrate(C.byref(vol._vol), 17, (_abi.OlsrTsdfView * 17)(), None) == _abi.OLSR_ERR_ARG
    assert b"between 1 and 16 views" in L.olsr_last_error()
    assert L.olsr_tsdf_integrate(C.byref(vol._vol), 1, (_abi.OlsrTsdfView * 1)(), None) == _abi.OLSR_ERR_ARG
    assert b"H, W must be >= 1" in L.olsr_last_error()
    assert L.olsr_tsdf_surface_plan(C.byref(vol._vol), 0.0, None, None, None) == _abi.OLSR_ERR_ARG
    assert b"scratch and status are required" in L.olsr_last_error()
