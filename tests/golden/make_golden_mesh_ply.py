"""Generates tests/golden/mesh_ply.npz: what the reference's OWN meshwrite, meshwrite_color and pcwrite
(tsdf-fusion/fusion3.py:607-773) write for a fixed mesh of 5 vertices and 3 faces with 15 features.  Runs ONLY where the
reference checkout exists (OLSR_REFERENCE names it); the committed .npz is data: the input arrays and the three files' bytes.

fusion3.py is imported unmodified.  numba and skimage are not installed where this file is made: `numba.njit` is stubbed as
the identity and `prange` as range, `skimage.measure` as an empty module (none of them is reached by the writers); pycuda's
absence is handled by fusion3.py itself (its import sits in a try block).

The mesh: a fan of three triangles over five vertices; positions, normals and features with negative values, values that "%f"
rounds in the sixth decimal, an exact zero and a value above 1e6; colours in 0 ... 255 with fractional parts (meshwrite_color
truncates them to uint8)."""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if "OLSR_REFERENCE" not in os.environ:
    raise SystemExit("set OLSR_REFERENCE to the reference checkout")
sys.path.insert(0, os.path.join(os.environ["OLSR_REFERENCE"], "tsdf-fusion"))

numba = types.ModuleType("numba")
numba.njit = lambda *a, **k: (a[0] if a and callable(a[0]) else (lambda f: f))
numba.prange = range
skimage = types.ModuleType("skimage")
skimage.measure = types.ModuleType("skimage.measure")
sys.modules.update({"numba": numba, "skimage": skimage, "skimage.measure": skimage.measure})

import fusion3  # noqa: E402


def make_mesh(seed=0):
    rng = np.random.default_rng(seed)
    verts = rng.normal(size=(5, 3)).astype(np.float32)
    verts[0] = [0.0, -1.2345675, 1234567.875]
    norms = rng.normal(size=(5, 3)).astype(np.float32)
    norms /= np.linalg.norm(norms, axis=1, keepdims=True)
    norms[4] = 0.0
    feats = rng.normal(size=(5, 15)).astype(np.float32)
    feats[1, 0] = 0.0000004
    colors = rng.uniform(0.0, 255.99, size=(5, 3)).astype(np.float32)
    colors[2] = [0.0, 255.0, 127.5]
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4]], dtype=np.int32)
    return verts, faces, norms, feats, colors


def main():
    verts, faces, norms, feats, colors = make_mesh()
    out = dict(verts=verts, faces=faces, norms=norms, feats=feats, colors=colors)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "a.ply")
        fusion3.meshwrite(path, verts, faces, norms, feats)
        out["meshwrite"] = np.frombuffer(open(path, "rb").read(), np.uint8)
        fusion3.meshwrite_color(path, verts, faces, norms, colors)
        out["meshwrite_color"] = np.frombuffer(open(path, "rb").read(), np.uint8)
        # pcwrite never closes its file: run it where the file object dies with the call, so that its buffer is flushed
        (lambda: fusion3.pcwrite(path, np.concatenate([verts, feats], axis=1)))()
        import gc
        gc.collect()
        out["pcwrite"] = np.frombuffer(open(path, "rb").read(), np.uint8)
    for k in ("meshwrite", "meshwrite_color", "pcwrite"):
        text = out[k].tobytes().decode()
        assert text.startswith("ply\n") and text.endswith("\n"), k
        print(f"{k}: {len(out[k])} bytes, {text.count(chr(10))} lines")
    np.savez_compressed(os.path.join(HERE, "mesh_ply.npz"), **out)


if __name__ == "__main__":
    main()
