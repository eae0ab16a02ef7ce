"""Float32 numpy restatement of the TSDF mesh extraction (include/olsr.h, olsr_tsdf_mesh_plan / olsr_tsdf_mesh_emit): the
vertices are those of tests/tsdf_ref.py's `surface`, the faces come from the generated triangle table
(scripts/gen_mc_table.py), the normals from the statements of include/olsr.h one numpy operation each, every operand float32
(no FMA, IEEE division and square root).  The GPU tests hold the kernels to this bit for bit; the functions at the end state
the mesh properties (closedness, Euler characteristic, signed volume) both suites check.
"""
import importlib.util
import os

import numpy as np

import tsdf_ref as R

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def generator():
    """scripts/gen_mc_table.py as a module."""
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "scripts", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TABLE = None


def table():
    """[256] lists of (edge, edge, edge)."""
    global _TABLE
    if _TABLE is None:
        _TABLE = generator().table()
    return _TABLE


def crossings(tsdf, weight, min_weight=0.0):
    """bool [X,Y,Z,3]: the edge from a voxel along axis a is owned by it and crosses zero (tsdf_ref.surface's rule)."""
    X, Y, Z = tsdf.shape
    neg = tsdf < 0
    seen = (weight >= f32(min_weight)) if min_weight > 0 else np.ones_like(neg)
    cross = np.zeros((X, Y, Z, 3), bool)
    cross[:-1, :, :, 0] = (neg[:-1] != neg[1:]) & seen[:-1] & seen[1:]
    cross[:, :-1, :, 1] = (neg[:, :-1] != neg[:, 1:]) & seen[:, :-1] & seen[:, 1:]
    cross[:, :, :-1, 2] = (neg[:, :, :-1] != neg[:, :, 1:]) & seen[:, :, :-1] & seen[:, :, 1:]
    return cross, neg, seen


def faces(tsdf, weight, min_weight=0.0):
    """int32 [M,3] vertex ids, in cube linear order (z fastest), then table order."""
    X, Y, Z = tsdf.shape
    cross, neg, seen = crossings(tsdf, weight, min_weight)
    if min(X, Y, Z) < 2:
        return np.zeros((0, 3), np.int32)
    vid = (np.cumsum(cross.reshape(-1)) - 1).reshape(X, Y, Z, 3)        # the id of an owned edge's vertex
    config = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    ok = np.ones((X - 1, Y - 1, Z - 1), bool)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        config |= neg[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << c
        ok &= seen[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz]
    config[~ok] = 0
    T = table()
    n_tris = np.array([len(t) for t in T])
    edges = np.zeros((256, 5, 3), np.int64)
    for c, tris in enumerate(T):
        if tris:
            edges[c, :len(tris)] = tris
    cubes = np.nonzero(n_tris[config.reshape(-1)])[0]                     # row-major: cube linear order
    cfg = config.reshape(-1)[cubes]
    x, y, z = np.unravel_index(cubes, config.shape)
    e = edges[cfg]                                                       # [C,5,3] edge ids
    axis, lo, hi = e >> 2, e & 1, (e >> 1) & 1
    # edge 4 * axis + k is owned by the corner whose two other coordinates, in ascending axis order, are (k & 1, k >> 1)
    px = x[:, None, None] + np.where(axis == 0, 0, lo)
    py = y[:, None, None] + np.where(axis == 0, lo, np.where(axis == 1, 0, hi))
    pz = z[:, None, None] + np.where(axis == 2, 0, hi)
    keep = np.arange(5)[None, :] < n_tris[cfg][:, None]                  # [C,5]: then table order
    assert cross[px, py, pz, axis][keep].all()
    return vid[px, py, pz, axis][keep].astype(np.int32).reshape(-1, 3)


def gradient(tsdf):
    """float32 [X,Y,Z,3]: central differences 0.5f * (t[+1] - t[-1]), one-sided t[+1] - t[0] / t[0] - t[-1] on the grid's
    border, 0 along an axis of one voxel."""
    g = np.zeros(tsdf.shape + (3,), np.float32)
    with np.errstate(all="ignore"):
        for a in range(3):
            n = tsdf.shape[a]
            if n < 2:
                continue
            t = np.moveaxis(tsdf, a, 0)
            ga = np.moveaxis(g[..., a], a, 0)
            ga[1:-1] = f32(0.5) * (t[2:] - t[:-2])
            ga[0] = t[1] - t[0]
            ga[-1] = t[-1] - t[-2]
    assert g.dtype == np.float32
    return g


def normals(tsdf, weight, min_weight=0.0):
    """float32 [N,3] per vertex, in the vertices' order."""
    X, Y, Z = tsdf.shape
    cross, _, _ = crossings(tsdf, weight, min_weight)
    v, axis = np.nonzero(cross.reshape(-1, 3))
    stride = np.array([Y * Z, Z, 1], dtype=np.int64)[axis]
    flat, g = tsdf.reshape(-1), gradient(tsdf).reshape(-1, 3)
    t0, t1 = flat[v], flat[v + stride]
    with np.errstate(all="ignore"):
        mu = (t0 / (t0 - t1))[:, None]
        g0, g1 = g[v], g[v + stride]
        n = g0 + (g1 - g0) * mu
        length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        out = np.where((length == 0)[:, None], f32(0), n / length[:, None])
    assert out.dtype == np.float32
    return out


def mesh(tsdf, weight, feat, origin, voxel_size, min_weight=0.0, packed=False):
    """-> (verts [N,3], faces int32 [M,3], norms [N,3], colors [N,F], voxel_index int32 [N])."""
    points, feats, index = R.surface(tsdf, weight, feat, origin, voxel_size, min_weight, packed)
    return points, faces(tsdf, weight, min_weight), normals(tsdf, weight, min_weight), feats, index


# ---- properties of a mesh ----------------------------------------------------------------------------------------------------
def directed_sides(faces):
    """int64 [3M,2]: the sides (i, j), (j, k), (k, i) of every face."""
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def unmatched_sides(faces, n_verts, skip=None):
    """The number of directed sides that are not matched exactly once in the opposite direction (each undirected side must
    occur once as (a, b) and once as (b, a)).  skip: bool [n_verts], sides with BOTH ends marked are left out."""
    s = directed_sides(faces)
    if skip is not None:
        s = s[~(skip[s[:, 0]] & skip[s[:, 1]])]
    fwd = s[:, 0] * n_verts + s[:, 1]
    rev = s[:, 1] * n_verts + s[:, 0]
    keys, counts = np.unique(fwd, return_counts=True)
    bad = int((counts != 1).sum())
    pos = np.searchsorted(keys, rev)
    pos[pos == len(keys)] = 0
    return bad + int((keys[pos] != rev).sum()) if len(keys) else 0


def on_boundary_face(voxel_index, axis, dim):
    """bool [N]: the vertex lies in one of the volume's six boundary faces (its edge runs inside that face)."""
    X, Y, Z = dim
    v = np.asarray(voxel_index, np.int64)
    c = [v // (Y * Z), (v % (Y * Z)) // Z, v % Z]
    out = np.zeros(len(v), bool)
    for d, n in enumerate(dim):
        out |= (axis != d) & ((c[d] == 0) | (c[d] == n - 1))
    return out


def vertex_axes(tsdf, weight, min_weight=0.0):
    cross, _, _ = crossings(tsdf, weight, min_weight)
    return np.nonzero(cross.reshape(-1, 3))[1]


def euler_characteristic(faces, n_verts):
    s = np.sort(directed_sides(faces), axis=1)
    return n_verts - len(np.unique(s[:, 0] * n_verts + s[:, 1])) + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def sphere(dim=(16, 16, 16), centre=(7.4, 7.6, 7.3), r=5.3):
    """An exact signed distance (negative inside), float32 [X,Y,Z], in voxel units."""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dim], indexing="ij"), axis=-1) - np.asarray(centre)
    return (np.sqrt((g * g).sum(-1)) - r).astype(np.float32)


def torus(dim=(16, 16, 16), centre=(7.4, 7.6, 7.3), R_=4.6, r=1.9):
    """The torus round the z axis through `centre`."""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dim], indexing="ij"), axis=-1) - np.asarray(centre)
    q = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - R_
    return (np.sqrt(q * q + g[..., 2] ** 2) - r).astype(np.float32)


# ---- the reference's readers of the PLY files ------------------------------------------------------------------------------
def mesh_parser(path):
    """What the evaluation's mesh_parser does with a file (3d_evaluation_and_visualize_langslam_dim15.py:276-293), restated:
    lines whose first token is a number; four tokens make a face, anything else a vertex whose tokens 3 ... 5 are the normal."""
    normals, faces = [], []
    for line in open(path).readlines():
        ele = line.split(" ")
        try:
            float(ele[0])
        except ValueError:
            continue
        if len(ele) != 4:
            normals.append([float(v) for v in ele[3:6]])
        else:
            faces.append([float(v) for v in ele[1:4]])
    return np.asarray(normals), np.asarray(faces)


def pc15_parser(path):
    pts, feats = [], []
    for line in open(path).readlines():
        ele = line.split(" ")
        try:
            float(ele[0])
        except ValueError:
            continue
        pts.append([float(v) for v in ele[:3]])
        feats.append([float(v) for v in ele[3:18]])
    return np.asarray(pts), np.asarray(feats)
