"""olsr_tsdf_mesh_* (HIP) and TSDFVolume.get_mesh / meshwrite on the GPU.

Yardstick: tests/tsdf_mesh_ref.py, the float32 numpy restatement (vertices: tests/tsdf_ref.py's surface; faces: the generated
table of scripts/gen_mc_table.py; normals: the statements of include/olsr.h).  Every comparison with it is exact: the faces as
integers, the vertices, colours and normals bit for bit (a NaN where the restatement has a NaN), and the vertices, colours and
voxel indices also against surface_points of the same volume on the device.  The smooth shapes are held to properties of the
mesh itself: closed, the right Euler characteristic, outward winding, the enclosed volume, normals along the faces'.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import tsdf_mesh_ref as M
from test_gpu_tsdf import DEV, IMAGES, VOXEL, _device_view, _reference, _views, _volume

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    """Two device tensors of 32-bit elements hold the same bits (NaNs included)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _equals_restatement(got, want):
    """float32: the same bits wherever the restatement has a number, a NaN wherever it has a NaN."""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan])


def _fill(vol, t, w, f):
    tsdf, feat = vol.get_volume()          # the volume itself
    tsdf.copy_(torch.from_numpy(t))
    vol.weight.copy_(torch.from_numpy(w))
    if f is not None:
        feat.copy_(torch.from_numpy(f))


def _assert_mesh(vol, arrays, packed, min_weight, label):
    """get_mesh against the restatement and against surface_points; -> (the restatement's mesh, the device's)."""
    t, w, f = arrays
    want = M.mesh(t, w, f, vol.vol_origin, VOXEL, min_weight, packed)
    verts, faces, norms, colors, index = vol._mesh(min_weight)
    points, feats, own = vol.surface_points(min_weight)
    torch.cuda.synchronize()
    print(f"{label}: {len(want[0])} vertices, {len(want[1])} faces (min_weight {min_weight})")
    assert faces.dtype == torch.int32 and tuple(faces.shape) == want[1].shape and tuple(verts.shape) == want[0].shape
    assert torch.equal(faces.cpu(), torch.from_numpy(want[1])), f"{label}: faces"
    assert _bits_equal(verts, points) and torch.equal(index, own), f"{label}: vertices against surface_points"
    assert _equals_restatement(verts, want[0]), f"{label}: vertices"
    if want[3].shape[1]:
        assert _bits_equal(colors, feats) and _equals_restatement(colors, want[3]), f"{label}: colours"
    else:
        assert colors is None and feats is None
    assert _equals_restatement(norms, want[2]), f"{label}: normals"
    again = vol.get_mesh(min_weight)
    assert len(again) == 4 and torch.equal(again[1], faces) and _bits_equal(again[0], verts) and _bits_equal(again[2], norms)
    assert (colors is None and again[3] is None) or _bits_equal(again[3], colors)
    return want, (verts, faces, norms, colors, index)


@functools.lru_cache(maxsize=None)
def _random_arrays(dim, feature):
    """Random distances with exact zeros and, where there is room, one NaN, one +inf and one -inf; weights 0, 1, 2."""
    rng = np.random.default_rng(5 + dim[0])
    n = int(np.prod(dim))
    t = rng.uniform(-1, 1, dim).astype(np.float32)
    t[rng.random(dim) < 0.05] = 0.0
    if n >= 8:
        where = rng.choice(n, 3, replace=False)
        t.reshape(-1)[where] = [np.nan, np.inf, -np.inf]
    w = rng.integers(0, 3, dim).astype(np.float32)
    f = (rng.integers(0, 1 << 24, dim).astype(np.float32) if feature == "rgb" else rng.normal(size=(3,) + dim).astype(np.float32))
    return t, w, f


# (64, 1, 65): vertices but no cube; (65, 64, 65): 1057 blocks of 256 voxels, more than one round of the prefix
@pytest.mark.parametrize("dim", [(1, 1, 1), (2, 2, 2), (5, 3, 70), (64, 1, 65), (9, 7, 6), (65, 64, 65)])
@pytest.mark.parametrize("feature", [3, "rgb"])
def test_mesh_of_a_random_volume_equals_the_restatement(hip, dim, feature):
    t, w, f = _random_arrays(dim, feature)
    vol = _volume(dim, feature)
    _fill(vol, t, w, f)
    for mw in (0.0, 1.0):
        want, _ = _assert_mesh(vol, (t, w, f), feature == "rgb", mw, f"random {dim} F={feature}")
        if min(dim) < 2:
            assert len(want[1]) == 0
    full = M.mesh(t, w, f, vol.vol_origin, VOXEL, 0.0, feature == "rgb")
    if dim == (64, 1, 65):
        assert len(full[0]) > 1000
    if int(np.prod(dim)) >= 100:
        assert np.isnan(full[0]).any() and np.isnan(full[2]).any() and (len(full[1]) > 0) == (min(dim) > 1)


def test_all_256_configurations(hip):
    """(512, 2, 2): the cube at x = 2 c has configuration c, every one of the 256 occurs."""
    dim = (512, 2, 2)
    rng = np.random.default_rng(3)
    t = rng.uniform(0.1, 1.0, dim).astype(np.float32)
    for c in range(256):
        for corner in range(8):
            if (c >> corner) & 1:
                t[2 * c + (corner & 1), (corner >> 1) & 1, corner >> 2] *= -1
    w = np.ones(dim, np.float32)
    f = rng.normal(size=(3,) + dim).astype(np.float32)
    vol = _volume(dim, 3)
    _fill(vol, t, w, f)
    want, _ = _assert_mesh(vol, (t, w, f), False, 0.0, "all configurations")
    n_tris = [len(x) for x in M.table()]
    assert len(want[1]) > sum(n_tris) == 820                  # (the cubes at odd x add theirs)
    # the faces of the cubes at even x, found through their first vertex's owner, are the table's
    neg = t < 0
    config = sum(neg[c & 1:511 + (c & 1), (c >> 1) & 1, c >> 2].astype(int) << c for c in range(8))
    assert np.array_equal(config[0::2], np.arange(256))
    per_cube = np.array([n_tris[c] for c in config])
    start = np.concatenate([[0], np.cumsum(per_cube)])
    cross, _, _ = M.crossings(t, w)
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(dim + (3,))
    for c in (1, 0x5a, 0x69, 0x96, 0xfe):                      # spot checks: edge ids to vertex ids by hand
        tri = M.table()[c][0]
        ids = []
        for e in tri:
            axis, k = e >> 2, e & 3
            p = [2 * c, 0, 0]
            others = [d for d in range(3) if d != axis]
            p[others[0]] += k & 1
            p[others[1]] += k >> 1
            ids.append(vid[p[0], p[1], p[2], axis])
        assert want[1][start[2 * c]].tolist() == ids, c


def test_the_device_mesh_of_a_random_volume_is_closed_away_from_the_boundary(hip):
    dim = (65, 64, 65)
    rng = np.random.default_rng(17)
    t = rng.uniform(-1, 1, dim).astype(np.float32)
    w = np.ones(dim, np.float32)
    vol = _volume(dim, 0)
    _fill(vol, t, w, None)
    verts, faces, norms, colors, index = vol._mesh(0.0)
    torch.cuda.synchronize()
    assert colors is None and faces.shape[0] > 500_000
    axes = M.vertex_axes(t, w)
    assert len(axes) == verts.shape[0]
    faces, index = faces.cpu().numpy(), index.cpu().numpy()
    assert len(np.unique(faces)) == len(index)               # every vertex is referenced
    assert M.unmatched_sides(faces, len(index), M.on_boundary_face(index, axes, dim)) == 0
    assert M.unmatched_sides(faces, len(index)) > 0          # (the boundary's sides have no partner: the check can fail)


# What the restatement gives for these shapes (tests/test_tsdf_mesh_cpu.py runs it): sphere 1036 faces, 520 vertices, volume
# ratio 0.979, smallest face-normal . vertex-normal 0.986; torus 1012 faces, 506 vertices, ratio 0.942, smallest dot 0.810.
# The inscribed mesh of a convex (sphere) or mostly convex (torus) body encloses less than the body: the windows below.
@pytest.mark.parametrize("shape,chi,lo", [("sphere", 2, 0.96), ("torus", 0, 0.92)])
def test_smooth_shapes(hip, shape, chi, lo):
    t = getattr(M, shape)()
    dim = t.shape
    exact = 4.0 / 3.0 * math.pi * 5.3 ** 3 if shape == "sphere" else 2.0 * math.pi ** 2 * 4.6 * 1.9 ** 2
    w = np.ones(dim, np.float32)
    vol = _volume(dim, 0)
    _fill(vol, t, w, None)
    want, (verts, faces, norms, _, index) = _assert_mesh(vol, (t, w, np.zeros((0,) + dim, np.float32)), False, 0.0, shape)
    faces = faces.cpu().numpy()
    grid = (verts.cpu().numpy().astype(np.float64) - vol.vol_origin.astype(np.float64)) / VOXEL      # in voxel units
    n = len(grid)
    assert len(np.unique(faces)) == n                          # every vertex is referenced
    assert M.unmatched_sides(faces, n) == 0                    # every side is matched once in the opposite direction
    assert M.euler_characteristic(faces, n) == chi
    volume = M.signed_volume(grid, faces)
    a, b, c = grid[faces[:, 0]], grid[faces[:, 1]], grid[faces[:, 2]]
    fn = np.cross(b - a, c - a)
    area = np.linalg.norm(fn, axis=1)
    keep = area > 0
    fn = fn[keep] / area[keep, None]
    vn = norms.cpu().numpy().astype(np.float64)
    dots = np.stack([(fn * vn[faces[keep, k]]).sum(axis=1) for k in range(3)])
    print(f"{shape}: {len(faces)} faces, {n} vertices, volume ratio {volume / exact:.4f}, smallest dot {dots.min():.4f}, "
          f"{int((~keep).sum())} faces of no area")
    assert volume > 0
    assert lo <= volume / exact <= 1.0
    assert float(dots.min()) > 0.5


@pytest.mark.parametrize("min_weight", [0.0, 1.0])
@pytest.mark.parametrize("feature", [0, 15, "rgb"])
def test_mesh_of_a_fused_volume(hip, feature, min_weight):
    dim, (W, H) = (42, 34, 38), IMAGES[0]
    ref, _ = _reference(dim, W, H, feature)
    vol = _volume(dim, feature)
    vol.integrate_views([_device_view(v) for v in _views(dim, W, H, feature)])
    t, w, f = ref.arrays()
    want, (verts, faces, norms, colors, index) = _assert_mesh(vol, (t, w, f), feature == "rgb", min_weight, f"fused F={feature}")
    assert len(want[1]) > 500
    if min_weight == 0.0:
        assert len(want[1]) > len(M.faces(t, w, 1.0))
        return
    # no face touches a cube with an unobserved corner.  A face's three vertices lie on three edges of its cube that do not
    # all lie in one face of it, so the least of their owners' coordinates, axis by axis, is the cube's lowest voxel
    own = index.cpu().numpy().astype(np.int64)[faces.cpu().numpy()]                    # [M,3]
    X, Y, Z = dim
    base = np.stack([(own // (Y * Z)).min(axis=1), ((own % (Y * Z)) // Z).min(axis=1), (own % Z).min(axis=1)], axis=1)
    assert (base.max(axis=0) < np.array(dim) - 1).all()
    seen = w >= 1.0
    for c in range(8):
        assert seen[base[:, 0] + (c & 1), base[:, 1] + ((c >> 1) & 1), base[:, 2] + (c >> 2)].all(), c


def test_capacities_one_short_write_nothing_past_them(hip):
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd._lib import check, lib
    dim, feature = (9, 7, 6), 3
    t, w, f = _random_arrays(dim, feature)
    vol = _volume(dim, feature)
    _fill(vol, t, w, f)
    verts, faces, norms, colors, index = vol._mesh(0.0)
    n, m = verts.shape[0], faces.shape[0]
    assert n > 100 and m > 100
    L = lib()
    GUARD, canary = 64, -7.0
    scratch = torch.empty(L.olsr_tsdf_mesh_scratch_bytes(*dim), dtype=torch.uint8, device=DEV)
    status = torch.zeros(4, dtype=torch.int32, device=DEV)
    check(L.olsr_tsdf_mesh_plan(C.byref(vol._vol), 0.0, scratch.data_ptr(), status.data_ptr(), None))
    assert status.tolist() == [n, m, 0, 0]
    for nv, nf in ((n - 1, m - 1), (n, m - 1), (n - 1, m), (0, m), (n, 0)):
        p = torch.full((n + GUARD, 3), canary, device=DEV)
        q = torch.full((n + GUARD, 3), canary, device=DEV)
        c = torch.full((n + GUARD, 3), canary, device=DEV)
        i = torch.full((n + GUARD,), -7, dtype=torch.int32, device=DEV)
        fa = torch.full((m + GUARD, 3), -7, dtype=torch.int32, device=DEV)
        check(L.olsr_tsdf_mesh_emit(C.byref(vol._vol), 0.0, scratch.data_ptr(), nv, nf, p.data_ptr(), q.data_ptr(), c.data_ptr(),
                                    i.data_ptr(), fa.data_ptr(), None))
        torch.cuda.synchronize()
        assert bool((p[nv:] == canary).all()) and bool((q[nv:] == canary).all()) and bool((c[nv:] == canary).all())
        assert bool((i[nv:] == -7).all()) and bool((fa[nf:] == -7).all())
        assert _bits_equal(p[:nv], verts[:nv]) and _bits_equal(q[:nv], norms[:nv]) and _bits_equal(c[:nv], colors[:nv])
        assert torch.equal(i[:nv], index[:nv]) and torch.equal(fa[:nf], faces[:nf])
    assert L.olsr_tsdf_mesh_emit(C.byref(vol._vol), 0.0, scratch.data_ptr(), n, m, None, None, None, None, None, None) == _abi.OLSR_ERR_ARG
    assert b"points, normals and (F > 0) feats are required" in L.olsr_last_error()


def test_mesh_of_an_empty_volume(hip):
    vol = _volume((5, 3, 70), 15)
    verts, faces, norms, colors = vol.get_mesh()
    assert tuple(verts.shape) == (0, 3) and tuple(norms.shape) == (0, 3) and tuple(colors.shape) == (0, 15)
    assert tuple(faces.shape) == (0, 3) and faces.dtype == torch.int32
    assert tuple(vol.get_mesh(1.0)[1].shape) == (0, 3)


def test_meshwrite_round_trip(hip, tmp_path):
    from online_lang_splatting_amd.tsdf import meshwrite, meshwrite_color, pcwrite
    dim, (W, H) = (42, 34, 38), IMAGES[0]
    vol = _volume(dim, 15)
    vol.integrate_views([_device_view(v) for v in _views(dim, W, H, 15)])
    verts, faces, norms, colors = vol.get_mesh(1.0)
    n, m = verts.shape[0], faces.shape[0]
    assert n > 100 and m > 100
    path = str(tmp_path / "semantic_mesh.ply")
    meshwrite(path, verts, faces, norms, colors)
    head = open(path).read().split("end_header")[0]
    assert f"element vertex {n}\n" in head and f"element face {m}\n" in head
    got_n, got_f = M.mesh_parser(path)
    assert got_n.shape == (n, 3) and np.array_equal(got_f, faces.cpu().numpy())
    assert np.allclose(got_n, norms.cpu().numpy(), atol=1e-6)
    meshwrite_color(path, verts, faces, norms, (colors[:, :3].clamp(-1, 1) + 1) * 127.5)
    got_n, got_f = M.mesh_parser(path)
    assert got_n.shape == (n, 3) and np.array_equal(got_f, faces.cpu().numpy())
    cloud = vol.get_point_cloud(1.0)
    pcwrite(path, cloud)
    pts, feats = M.pc15_parser(path)
    assert pts.shape == (n, 3) and feats.shape == (n, 15) and np.allclose(pts, verts.cpu().numpy(), atol=1e-6)
