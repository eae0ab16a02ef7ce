"""The TSDF mesh extraction, the part that needs no GPU: the generated triangle table and its rule, the numpy restatement's
meshes (tests/tsdf_mesh_ref.py), the C-ABI's argument checks and the PLY writers against what the reference's own writers
wrote (tests/golden/mesh_ply.npz)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import tsdf_mesh_ref as M
import tsdf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000   # a made-up address: every call below returns before anything could follow it


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import build
    build.build()
    from online_lang_splatting_amd import _lib
    return _lib.lib()


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_the_committed_header_is_what_the_generator_emits():
    G = M.generator()
    assert open(G.HEADER).read() == G.header_text()
    from online_lang_splatting_amd import build
    assert "olsr_mc_table.h" in build.HEADERS
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{16})ull", open(G.HEADER).read())]
    assert len(words) == 256 and [G.unpack(w) for w in words] == [[tuple(t) for t in tris] for tris in G.table()]


# the cube's geometry, stated here on its own from the numbering the header documents
def _edge_ends(e):
    axis, k = e >> 2, e & 3
    others = [d for d in range(3) if d != axis]
    p = np.zeros(3, int)
    p[others[0]], p[others[1]] = k & 1, k >> 1
    q = p.copy()
    q[axis] = 1
    return p, q


def _cube_faces():
    """(outward normal, the edges in the face, its corners in cyclic order)."""
    out = []
    for axis, side in itertools.product(range(3), (0, 1)):
        edges = [e for e in range(12) if all(p[axis] == side for p in _edge_ends(e))]
        u, v = [d for d in range(3) if d != axis]
        ring = []
        for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
            p = np.zeros(3, int)
            p[axis], p[u], p[v] = side, du, dv
            ring.append(p)
        normal = np.zeros(3)
        normal[axis] = 2 * side - 1
        assert len(edges) == 4
        out.append((normal, edges, ring))
    return out


def _edge_between(p, q):
    return next(e for e in range(12) if {tuple(x) for x in _edge_ends(e)} == {tuple(p), tuple(q)})


def _marching_squares(config, ring):
    """The undirected segments of a face, as frozensets of edge ids, with the negative corner each has on one side."""
    neg = [bool(config >> (int(p[0]) | int(p[1]) << 1 | int(p[2]) << 2) & 1) for p in ring]
    edge = [_edge_between(ring[k], ring[(k + 1) % 4]) for k in range(4)]
    crossed = [k for k in range(4) if neg[k] != neg[(k + 1) % 4]]
    if len(crossed) == 2:
        return {frozenset((edge[crossed[0]], edge[crossed[1]])): ring[neg.index(True)]}
    if len(crossed) == 4:   # the two negative corners are cut off separately
        return {frozenset((edge[(k - 1) % 4], edge[k])): ring[k] for k in range(4) if neg[k]}
    assert not crossed
    return {}


def test_every_configuration_follows_the_rule():
    T = M.table()
    faces = _cube_faces()
    assert sum(len(t) for t in T) == 820 and max(len(t) for t in T) == 5
    mid = {e: sum(_edge_ends(e)) / 2.0 for e in range(12)}
    for config, tris in enumerate(T):
        neg = [(config >> c) & 1 for c in range(8)]
        crossed = {e for e in range(12)
                   if neg[int(_edge_ends(e)[0] @ [1, 2, 4])] != neg[int(_edge_ends(e)[1] @ [1, 2, 4])]}
        assert {e for t in tris for e in t} == crossed, config                       # corners are crossed edges, all are used
        assert all(len(set(t)) == 3 for t in tris), config
        sides = [(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)]
        in_a_face = set()
        for normal, edges, ring in faces:
            want = _marching_squares(config, ring)
            got = [s for s in sides if s[0] in edges and s[1] in edges]
            assert len(got) == len(want) and {frozenset(s) for s in got} == set(want), (config, got, want)
            for a, b in got:   # seen from outside the cube the negative corner lies to the right: the normal points to free space
                n = want[frozenset((a, b))]
                assert np.dot(np.cross(normal, mid[b] - mid[a]), n - mid[a]) < 0, (config, a, b)
            in_a_face.update(got)
        inner = [s for s in sides if s not in in_a_face]
        assert len(inner) == len(set(inner)) and all((b, a) in inner for a, b in inner), config   # once in each direction


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def _random_volume(dim, seed):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, dim).astype(np.float32)
    w = rng.integers(0, 3, dim).astype(np.float32)
    f = rng.normal(size=(3,) + dim).astype(np.float32)
    return t, w, f


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_random_volume_is_closed_away_from_the_boundary(seed):
    dim = (9, 7, 6)
    t, w, f = _random_volume(dim, seed)
    origin = np.array([-0.37, 0.21, 0.55], np.float32)
    verts, faces, norms, colors, index = M.mesh(t, w, f, origin, 0.04)
    points, feats, own = R.surface(t, w, f, origin, 0.04)
    assert np.array_equal(verts, points) and np.array_equal(colors, feats) and np.array_equal(index, own)
    assert norms.shape == verts.shape and faces.dtype == np.int32 and len(faces) > 500
    assert int(faces.min()) >= 0 and int(faces.max()) < len(verts) and len(np.unique(faces)) == len(verts)
    edge = M.on_boundary_face(index, M.vertex_axes(t, w), dim)
    assert 0 < int(edge.sum()) < len(verts)
    assert M.unmatched_sides(faces, len(verts), edge) == 0
    assert M.unmatched_sides(faces, len(verts)) > 0            # (the sides in the boundary faces have no partner)
    # min_weight: only cubes whose eight corners were observed, so fewer faces, each a face of the full mesh's cube
    part = M.faces(t, w, 1.0)
    assert 0 < len(part) < len(faces)


@pytest.mark.parametrize("shape,chi", [("sphere", 2), ("torus", 0)])
def test_smooth_shapes_have_the_right_topology(shape, chi):
    t = getattr(M, shape)()
    w = np.ones(t.shape, np.float32)
    verts, faces, norms, _, _ = M.mesh(t, w, np.zeros((0,) + t.shape, np.float32), np.zeros(3), 1.0)
    assert len(np.unique(faces)) == len(verts) and M.unmatched_sides(faces, len(verts)) == 0
    assert M.euler_characteristic(faces, len(verts)) == chi
    assert M.signed_volume(verts, faces) > 0
    length = np.linalg.norm(norms.astype(np.float64), axis=1)
    assert np.allclose(length, 1.0, atol=1e-6)


def test_gradient_on_the_border_and_zero_normals():
    t = np.arange(24, dtype=np.float32).reshape(2, 3, 4) ** 2
    g = M.gradient(t)
    assert g[0, 0, 0, 2] == t[0, 0, 1] - t[0, 0, 0] and g[0, 0, 3, 2] == t[0, 0, 3] - t[0, 0, 2]
    assert g[0, 1, 1, 2] == np.float32(0.5) * (t[0, 1, 2] - t[0, 1, 0]) and g[1, 1, 1, 0] == t[1, 1, 1] - t[0, 1, 1]
    assert not M.gradient(np.ones((1, 1, 5), np.float32))[..., :2].any()
    # signs that alternate along z only: the gradients at both ends of an edge in the middle are zero, the border's are one-sided
    t = np.where(np.arange(8) % 2 == 0, -1.0, 1.0).astype(np.float32).reshape(1, 1, 8)
    n = M.normals(t, np.ones_like(t))
    assert n.shape == (7, 3) and not n[1:-1].any() and n[0, 2] == 1.0 and n[-1, 2] == 1.0


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------
def test_prototypes_match_the_header(L):
    from online_lang_splatting_amd import _lib
    src = open(os.path.join(ROOT, "include", "olsr.h")).read()
    for name, n_args, restype in (("olsr_tsdf_mesh_scratch_bytes", 3, C.c_size_t), ("olsr_tsdf_mesh_plan", 5, C.c_int),
                                  ("olsr_tsdf_mesh_emit", 11, C.c_int)):
        m = re.search(r"(size_t|int) " + name + r"\(([^;]*)\);", src)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(2))
        assert len(args.split(",")) == n_args == len(getattr(L, name).argtypes) and name in _lib.EXPORTS
        assert getattr(L, name).restype is restype and (m.group(1) == "size_t") == (restype is C.c_size_t)
    assert L.olsr_tsdf_mesh_emit.argtypes[3:5] == [C.c_int32, C.c_int32] and L.olsr_tsdf_mesh_plan.argtypes[1] is C.c_float


def _volume(**kw):
    from online_lang_splatting_amd import _abi
    a = dict(X=4, Y=5, Z=6, F=15, feat_mode=_abi.TSDF_FEAT_FLOAT, voxel_size=0.02, trunc_margin=0.1, tsdf=X, weight=X, feat=X)
    a.update(kw)
    return _abi.OlsrTsdfVolume(**a)


def test_entries_validate_their_arguments(L):
    from online_lang_splatting_amd import _abi
    ok = _volume()

    def emit(vol=ok, scratch=X, nv=10, nf=10, points=X, normals=X, feats=X, index=X, faces=X):
        return L.olsr_tsdf_mesh_emit(None if vol is None else C.byref(vol), 0.0, scratch, nv, nf, points, normals, feats, index, faces, None)
    need = "tsdf_mesh_emit: points, normals and (F > 0) feats are required"
    rows = [
        ("plan no volume", lambda: L.olsr_tsdf_mesh_plan(None, 0.0, X, X, None), "tsdf_mesh_plan: volume is required"),
        ("plan empty", lambda: L.olsr_tsdf_mesh_plan(C.byref(_volume(Z=0)), 0.0, X, X, None),
         "tsdf_mesh_plan: volume: X, Y, Z must be >= 1"),
        ("plan size", lambda: L.olsr_tsdf_mesh_plan(C.byref(_volume(X=1024, Y=1024, Z=1024)), 0.0, X, X, None),
         "tsdf_mesh_plan: volume: 3 X Y Z must be below 2^31"),
        ("plan F", lambda: L.olsr_tsdf_mesh_plan(C.byref(_volume(F=7)), 0.0, X, X, None),
         "tsdf_mesh_plan: volume: F must be one of 0, 3, 15, 16, 32"),
        ("plan tsdf", lambda: L.olsr_tsdf_mesh_plan(C.byref(_volume(tsdf=None)), 0.0, X, X, None),
         "tsdf_mesh_plan: volume: tsdf, weight and (F > 0) feat are required"),
        ("plan scratch", lambda: L.olsr_tsdf_mesh_plan(C.byref(ok), 0.0, None, X, None), "tsdf_mesh_plan: scratch and status are required"),
        ("plan status", lambda: L.olsr_tsdf_mesh_plan(C.byref(ok), 0.0, X, None, None), "tsdf_mesh_plan: scratch and status are required"),
        ("emit no volume", lambda: emit(vol=None), "tsdf_mesh_emit: volume is required"),
        ("emit empty", lambda: emit(vol=_volume(X=0)), "tsdf_mesh_emit: volume: X, Y, Z must be >= 1"),
        ("emit size", lambda: emit(vol=_volume(X=1024, Y=1024, Z=1024)), "tsdf_mesh_emit: volume: 3 X Y Z must be below 2^31"),
        ("emit scratch", lambda: emit(scratch=None),
         "tsdf_mesh_emit: scratch, vert_capacity >= 0 and face_capacity >= 0 are required"),
        ("emit vert capacity", lambda: emit(nv=-1), "tsdf_mesh_emit: scratch, vert_capacity >= 0 and face_capacity >= 0 are required"),
        ("emit face capacity", lambda: emit(nf=-1), "tsdf_mesh_emit: scratch, vert_capacity >= 0 and face_capacity >= 0 are required"),
        ("emit 3 faces", lambda: emit(nf=(2 ** 31 - 1) // 3 + 1), "tsdf_mesh_emit: 3 face_capacity must be below 2^31"),
        ("emit points", lambda: emit(points=None), need),
        ("emit normals", lambda: emit(normals=None), need),
        ("emit feats", lambda: emit(feats=None), need),
        ("emit faces", lambda: emit(faces=None), "tsdf_mesh_emit: faces is required"),
    ]
    wrong = []
    for label, call, message in rows:
        rc = call()
        got = L.olsr_last_error().decode()
        if rc != _abi.OLSR_ERR_ARG or got != message:
            wrong.append((label, rc, got))
    assert not wrong, wrong
    # nothing to emit is not an error, whatever the pointers
    assert emit(nv=0, nf=0, points=None, normals=None, feats=None, index=None, faces=None) == _abi.OLSR_OK


def test_mesh_scratch_size(L):
    # four 32-bit words per block of 256 voxels and one per voxel, in five carved sub-arrays: each may be padded to 256 bytes,
    # and the base takes up to 256 more (tests/test_extents_cpu.py checks the layout itself)
    slack = 256 * (5 + 1)
    n = 400 * 250 * 150
    for dim, payload in (((1, 1, 1), 4 * (4 + 1)), ((400, 250, 150), 4 * (4 * -(-n // 256) + n)), ((0, 5, 5), 0)):
        assert payload <= L.olsr_tsdf_mesh_scratch_bytes(*dim) <= payload + slack, dim


# ---- the writers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_tensor", [False, True])
def test_writers_reproduce_the_reference_files(tmp_path, as_tensor):
    import torch

    from online_lang_splatting_amd import tsdf as T
    g = np.load(os.path.join(ROOT, "tests", "golden", "mesh_ply.npz"))
    conv = torch.from_numpy if as_tensor else (lambda a: a)
    verts, faces, norms, feats, colors = (conv(g[k]) for k in ("verts", "faces", "norms", "feats", "colors"))
    assert tuple(verts.shape) == (5, 3) and tuple(faces.shape) == (3, 3) and tuple(feats.shape) == (5, 15)
    path = str(tmp_path / "a.ply")
    T.meshwrite(path, verts, faces, norms, feats)
    assert open(path, "rb").read() == g["meshwrite"].tobytes()
    n, f = M.mesh_parser(path)
    assert np.allclose(n, g["norms"], atol=1e-6) and np.array_equal(f, g["faces"])
    T.meshwrite_color(path, verts, faces, norms, colors)
    assert open(path, "rb").read() == g["meshwrite_color"].tobytes()
    n, f = M.mesh_parser(path)
    assert np.allclose(n, g["norms"], atol=1e-6) and np.array_equal(f, g["faces"])
    cloud = np.concatenate([g["verts"], g["feats"]], axis=1)
    T.pcwrite(path, conv(cloud))
    assert open(path, "rb").read() == g["pcwrite"].tobytes()
    p, c = M.pc15_parser(path)
    assert p.shape == (5, 3) and c.shape == (5, 15) and np.allclose(c, g["feats"], atol=1e-6)
    with pytest.raises(RuntimeError, match=r"meshwrite: colors has shape \(5, 3\), expected \[N,15\]"):
        T.meshwrite(path, verts, faces, norms, colors)
    with pytest.raises(RuntimeError, match=r"pcwrite: xyzfeat has shape \(5, 3\), expected \[N,18\]"):
        T.pcwrite(path, verts)
