"""The numpy restatement of the reference's point_cloud.ply record (GaussianModel.save_ply / load_ply /
construct_list_of_attributes, gaussian_splatting/scene/gaussian_model.py:478-689), the reference of tests/test_map_io_cpu.py
and tests/test_gpu_map_io.py, with a minimal PLY writer and reader of its own (no line of map_io.py is used here).

Arrays are handled as float32 whose BITS matter: np.concatenate, transpose and reshape copy words, so a record built here
carries every NaN payload, signed zero, infinity and denormal of its inputs."""
import numpy as np


def attribute_names(xyz, f_dc, f_rest, language, scaling, rotation):
    """construct_list_of_attributes (:478-507) on the reference's shapes: f_dc [P,1,3], f_rest [P,M-1,3], language [P,F] or
    None (is_language False)."""
    names = ["x", "y", "z", "nx", "ny", "nz"]
    for i in range(f_dc.shape[1] * f_dc.shape[2]):
        names.append(f"f_dc_{i}")
    for i in range(f_rest.shape[1] * f_rest.shape[2]):
        names.append(f"f_rest_{i}")
    if language is not None:
        for i in range(language.shape[1]):
            names.append(f"f_language_{i}")
    names.append("opacity")
    for i in range(scaling.shape[1]):
        names.append(f"scale_{i}")
    for i in range(rotation.shape[1]):
        names.append(f"rot_{i}")
    return names


def names_for(M, F):
    """attribute_names for empty arrays of the shapes a map with shs [P,M,3] and language [P,F] has."""
    z = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    return attribute_names(z(0, 3), z(0, 1, 3), z(0, M - 1, 3), z(0, F) if F else None, z(0, 3), z(0, 4))


def record(means3D, shs, opacities, scales, rotations, language):
    """save_ply's `attributes` (:519-558): [P, 14 + 3 M + F] float32.  shs [P,M,3] = cat(f_dc, f_rest); language None or
    [P,0]: no language columns."""
    xyz = np.asarray(means3D, dtype=np.float32).reshape(-1, 3)
    P = xyz.shape[0]
    shs = np.asarray(shs, dtype=np.float32).reshape(P, -1, 3)
    normals = np.zeros_like(xyz)
    f_dc = np.ascontiguousarray(np.transpose(shs[:, :1], (0, 2, 1))).reshape(P, -1)      # .transpose(1, 2).flatten(start_dim=1)
    f_rest = np.ascontiguousarray(np.transpose(shs[:, 1:], (0, 2, 1))).reshape(P, -1)
    parts = [xyz, normals, f_dc, f_rest]
    if language is not None and np.asarray(language).reshape(P, -1).shape[1] > 0:
        parts.append(np.asarray(language, dtype=np.float32).reshape(P, -1))
    parts += [np.asarray(opacities, dtype=np.float32).reshape(P, 1), np.asarray(scales, dtype=np.float32).reshape(P, 3),
              np.asarray(rotations, dtype=np.float32).reshape(P, 4)]
    return np.concatenate(parts, axis=1)


def lookup(names, columns, F=0):
    """load_ply's lookup by name (:605-657) on a file's property names and its [P, n] body -> means3D, shs [P,M,3],
    opacities [P,1], scales, rotations, language [P,F] (the stated deviation: the reference reads no f_language_*;
    a missing channel is zero)."""
    at = {n: i for i, n in enumerate(names)}
    col = lambda n: columns[:, at[n]]  # noqa: E731
    P = columns.shape[0]
    xyz = np.stack((col("x"), col("y"), col("z")), axis=1)
    opac = col("opacity")[..., np.newaxis]
    dc = np.zeros((P, 3, 1), dtype=np.float32)
    for c in range(3):
        dc[:, c, 0] = col(f"f_dc_{c}")
    extra = sorted([n for n in names if n.startswith("f_rest_")], key=lambda x: int(x.split("_")[-1]))
    rest = np.zeros((P, len(extra)), dtype=np.float32)
    for i, n in enumerate(extra):
        rest[:, i] = col(n)
    rest = rest.reshape(P, 3, len(extra) // 3)
    shs = np.concatenate([np.transpose(dc, (0, 2, 1)), np.transpose(rest, (0, 2, 1))], axis=1)
    sn = sorted([n for n in names if n.startswith("scale_")], key=lambda x: int(x.split("_")[-1]))
    rn = sorted([n for n in names if n.startswith("rot")], key=lambda x: int(x.split("_")[-1]))
    scales = np.stack([col(n) for n in sn], axis=1)
    rots = np.stack([col(n) for n in rn], axis=1)
    lang = np.zeros((P, F), dtype=np.float32)
    for i in range(F):
        if f"f_language_{i}" in at:
            lang[:, i] = col(f"f_language_{i}")
    return dict(means3D=xyz, shs=np.ascontiguousarray(shs), opacities=opac, scales=scales, rotations=rots, language=lang)


# ---- a minimal PLY writer and reader of the tests' own -------------------------------------------------------------------
def write_ply(path, names, columns, comments=()):
    """A binary little-endian PLY with one float property per name and `columns` [P, len(names)] as its body."""
    columns = np.ascontiguousarray(columns, dtype="<f4")
    assert columns.ndim == 2 and columns.shape[1] == len(names)
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\n")
        for c in comments:
            f.write(("comment " + c + "\n").encode())
        f.write(f"element vertex {columns.shape[0]}\n".encode())
        for n in names:
            f.write(f"property float {n}\n".encode())
        f.write(b"end_header\n")
        f.write(columns.tobytes())


def read_ply(path):
    """-> (property names, body [P, n] float32) of a binary little-endian all-float PLY with one element."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    P, names = None, []
    for ln in lines[2:]:
        w = ln.split()
        if not w or w[0] in ("comment", "obj_info", "end_header"):
            continue
        if w[0] == "element":
            assert P is None and w[1] == "vertex", ln
            P = int(w[2])
        else:
            assert w[0] == "property" and w[1] in ("float", "float32") and len(w) == 3, ln
            names.append(w[2])
    body = np.frombuffer(data, dtype="<f4", offset=end)
    assert body.size == P * len(names), (body.size, P, len(names))
    return names, body.reshape(P, len(names)).copy()


# ---- inputs whose bits matter ---------------------------------------------------------------------------------------------
SPECIALS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7FA5A5A5, 0xFF812345,   # NaNs, quiet and signalling
                     0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                           # +-0, +-inf
                     0x00000001, 0x807FFFFF, 0x00400000, 0x80000123], dtype=np.uint32)         # denormals
SENTINEL = 0x7FDEAD5E   # a NaN no generator below produces: what rows >= P hold


def random_bits(shape, seed):
    """float32 array of `shape` holding random 32-bit patterns with SPECIALS planted (every one at least once when the array
    has room); never SENTINEL."""
    g = np.random.default_rng(seed)
    n = int(np.prod(shape))
    bits = g.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    bits[bits == SENTINEL] = 0
    if n:
        where = g.permutation(n)[: min(n, 4 * SPECIALS.size)]
        bits[where] = SPECIALS[np.arange(where.size) % SPECIALS.size]
    return bits.view(np.float32).reshape(shape)


def random_map(P, M, F, seed):
    """The six parameter arrays of a map, random bits."""
    return dict(means3D=random_bits((P, 3), seed), shs=random_bits((P, M, 3), seed + 1), opacities=random_bits((P, 1), seed + 2),
                scales=random_bits((P, 3), seed + 3), rotations=random_bits((P, 4), seed + 4),
                language=random_bits((P, F), seed + 5))


def bits(a):
    """The int32 view all value comparisons are made on."""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)
