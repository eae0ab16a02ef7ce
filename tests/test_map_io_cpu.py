"""The map's PLY record and the session's output files without a GPU: the header text, the header reader, the three symbols
of include/olsr_map_io.h and their argument errors, _abi's mirror of the header's constants, and save_trajectory's JSON."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import map_io_ref as R
from online_lang_splatting_amd import _abi, map_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "olsr_map_io.h")
SIZES = [(1, 0), (1, 15), (4, 3), (16, 32)]


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


# ---- the header text ------------------------------------------------------------------------------------------------------
LITERAL = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\n"
           b"property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
           b"property float f_dc_0\nproperty float f_dc_1\nproperty float f_dc_2\n"
           b"property float f_language_0\nproperty float f_language_1\nproperty float f_language_2\nproperty float f_language_3\n"
           b"property float f_language_4\nproperty float f_language_5\nproperty float f_language_6\nproperty float f_language_7\n"
           b"property float f_language_8\nproperty float f_language_9\nproperty float f_language_10\n"
           b"property float f_language_11\nproperty float f_language_12\nproperty float f_language_13\n"
           b"property float f_language_14\n"
           b"property float opacity\nproperty float scale_0\nproperty float scale_1\nproperty float scale_2\n"
           b"property float rot_0\nproperty float rot_1\nproperty float rot_2\nproperty float rot_3\nend_header\n")


def test_header_literal():
    assert map_io.ply_header(2, 1, 15) == LITERAL
    assert b"\r" not in LITERAL and b"comment" not in LITERAL


@pytest.mark.parametrize("M,F", SIZES)
def test_names_and_order(M, F):
    want = R.names_for(M, F)
    assert map_io.attribute_names(M, F) == want and len(want) == 14 + 3 * M + F
    lines = map_io.ply_header(7, M, F).decode("ascii").split("\n")
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 7"] and lines[-2:] == ["end_header", ""]
    assert lines[3:-2] == [f"property float {n}" for n in want]


@pytest.mark.parametrize("M,F", SIZES)
def test_header_round_trip(M, F):
    P = 3
    head = map_io.ply_header(P, M, F)
    width = 14 + 3 * M + F
    got_P, props, offset = map_io.read_ply_header(io.BytesIO(head + bytes(4 * P * width)))
    assert got_P == P and offset == len(head)
    assert props == [(n, "float") for n in R.names_for(M, F)]


def _file(lines, body=b""):
    return io.BytesIO(("\n".join(lines) + "\n").encode("ascii") + body)


GOOD = ["ply", "format binary_little_endian 1.0", "element vertex 2", "property float x", "property float32 y", "end_header"]


def test_reader_skips_comments_and_obj_info():
    lines = ["ply", "comment made by a test", "format binary_little_endian 1.0", "obj_info anything at all",
             "element vertex 2", "comment between", "property float x", "obj_info more", "property float32 y", "end_header"]
    f = _file(lines, bytes(16) + b"tail")
    P, props, offset = map_io.read_ply_header(f)
    assert (P, props) == (2, [("x", "float"), ("y", "float32")])
    assert offset == len(("\n".join(lines) + "\n").encode()) and f.tell() == offset
    # a second element's properties are not the vertex's
    P, props, _ = map_io.read_ply_header(_file(GOOD[:-1] + ["element face 0", "property list uchar int vertex_indices",
                                                               "end_header"], bytes(16)))
    assert (P, len(props)) == (2, 2)


BAD = {
    "ascii": ["ply", "format ascii 1.0"] + GOOD[2:],
    "big-endian": ["ply", "format binary_big_endian 1.0"] + GOOD[2:],
    "a double property": GOOD[:4] + ["property double y", "end_header"],
    "a list property": GOOD[:4] + ["property list uchar float y", "end_header"],
    "a first element that is not vertex": ["ply", "format binary_little_endian 1.0", "element face 2"] + GOOD[3:],
    "a missing end_header": GOOD[:-1],
    "not a ply": ["plx"] + GOOD[1:],
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_reader_rejects(what):
    with pytest.raises(ValueError):
        map_io.read_ply_header(_file(BAD[what], bytes(16)))


def test_reader_rejects_a_truncated_body():
    assert map_io.read_ply_header(_file(GOOD, bytes(16)))[0] == 2
    with pytest.raises(ValueError, match="body"):
        map_io.read_ply_header(_file(GOOD, bytes(15)))
    with pytest.raises(ValueError):
        map_io.read_ply_header(_file(GOOD))


def test_vertex_zero_parses():
    for M, F in SIZES:
        P, props, offset = map_io.read_ply_header(io.BytesIO(map_io.ply_header(0, M, F)))
        assert P == 0 and len(props) == 14 + 3 * M + F and offset == len(map_io.ply_header(0, M, F))
    assert map_io.read_ply_header(_file(["ply", "format binary_little_endian 1.0", "element vertex 0", "end_header"]))[:2] == (0, [])


def test_column_table():
    names = R.names_for(4, 3)
    order = list(np.random.default_rng(3).permutation(len(names)))
    props = [(names[i], "float") for i in order] + [("extra", "float")]
    M, F, col = map_io.column_table(props)
    assert (M, F) == (4, 3) and [order[c] for c in col] == list(range(len(names)))
    # F = 0 drops the channels, another count is refused, a file without channels gives -1
    assert map_io.column_table(props, F=0)[:2] == (4, 0)
    with pytest.raises(ValueError, match="language"):
        map_io.column_table(props, F=15)
    M, F, col = map_io.column_table([(n, "float") for n in R.names_for(1, 0)], F=15)
    assert (M, F) == (1, 15) and col[9:24] == [-1] * 15 and -1 not in col[:9] + col[24:]
    # normals may be missing; anything else may not; f_rest must give a square M
    no_normals = [(n, "float") for n in R.names_for(1, 0) if n not in ("nx", "ny", "nz")]
    assert map_io.column_table(no_normals)[2][3:6] == [-1, -1, -1]
    with pytest.raises(ValueError, match="rot_3"):
        map_io.column_table([(n, "float") for n in R.names_for(1, 0) if n != "rot_3"])
    with pytest.raises(ValueError, match="f_rest"):
        map_io.column_table([(n, "float") for n in R.names_for(4, 0)] + [("f_rest_9", "float"), ("f_rest_10", "float"),
                                                                       ("f_rest_11", "float")])


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(olsr_[a-z0-9_]+)\s*\(", src)))


def test_symbols_and_abi(L):
    from online_lang_splatting_amd import _lib
    assert _declared() == sorted(_lib.EXPORTS_MAP_IO) == ["olsr_map_ply_pack", "olsr_map_ply_unpack", "olsr_map_ply_width"]
    assert not set(_lib.EXPORTS_MAP_IO) & set(_lib.EXPORTS + _lib.EXPORTS_SINGLE_STAGE + _lib.EXPORTS_FRAME_INGEST)
    for name in _lib.EXPORTS_MAP_IO:
        assert hasattr(L, name), name
    header = open(HEADER).read()
    assert '#include "olsr.h"' in header
    for name, value in (("MAX_M", 16), ("MAX_F", 32), ("MAX_WIDTH", 94), ("BLOCK_ROWS", 64), ("MAX_COLS", 6016)):
        assert int(re.search(rf"#define OLSR_MAP_PLY_{name} (\d+)", header).group(1)) == getattr(_abi, f"MAP_PLY_{name}") == value
    assert _abi.MAP_PLY_MAX_WIDTH == 14 + 3 * _abi.MAP_PLY_MAX_M + _abi.MAP_PLY_MAX_F
    assert _abi.MAP_PLY_BLOCK_ROWS * _abi.MAP_PLY_MAX_WIDTH <= _abi.MAP_PLY_MAX_COLS    # one block's image at the widest record
    for deviation in ("language channels", "restated", "little-endian"):
        assert deviation in header, deviation
    # olsr.h's own declarations are untouched: none of the three is declared there
    olsr_h = open(os.path.join(ROOT, "include", "olsr.h")).read()
    assert "olsr_map_ply" not in olsr_h
    from online_lang_splatting_amd import build
    assert any(u[0] == "k_map_io.hip" for u in build.UNITS) and any(h.endswith("olsr_map_io.h") for h in build.HEADERS)
    import online_lang_splatting_amd as pkg
    assert pkg.map_io is map_io and "map_io" in pkg.__all__


def test_every_declared_function_has_an_extents_row():
    import test_gpu_map_io_extents as T
    assert sorted(T.COVERED + ("olsr_map_ply_width",)) == _declared()   # (the width is a host function: it stores nothing)


def test_width(L):
    for M in (1, 4, 9, 16):
        for F in (0, 1, 3, 15, 16, 32):
            assert L.olsr_map_ply_width(M, F) == 14 + 3 * M + F == map_io.ply_width(M, F)
    for M, F in ((0, 0), (2, 0), (3, 15), (25, 0), (17, 0), (-1, 0), (1, -1), (1, 33)):
        assert L.olsr_map_ply_width(M, F) == _abi.OLSR_ERR_ARG, (M, F)
        assert L.olsr_last_error()
        with pytest.raises(ValueError):
            map_io.ply_width(M, F)


# Addresses that are never dereferenced: every row below must be rejected before a launch.
PTR = 0x1000


def _buffers(**kw):
    b = _abi.OlsrMapBuffers(**{k: PTR for k in ("means3D", "shs", "opacities", "scales", "rotations", "language")})
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def test_pack_argument_errors(L):
    # P, M, F, src, rows, stream
    ok = [100, 1, 15, _buffers(), PTR, None]
    rows = [("src", {3: None}), ("rows", {4: None}), ("P < 0", {0: -1}), ("M = 0", {1: 0}), ("M = 2", {1: 2}), ("M = 17", {1: 17}),
            ("M = 25", {1: 25}), ("F < 0", {2: -1}), ("F = 33", {2: 33}), ("rows alignment", {4: PTR + 2})]
    rows += [(f"src.{k}", {3: _buffers(**{k: None})}) for k in ("means3D", "shs", "opacities", "scales", "rotations", "language")]
    for what, change in rows:
        a = list(ok)
        for k, v in change.items():
            a[k] = v
        src = None if a[3] is None else C.byref(a[3])
        assert L.olsr_map_ply_pack(a[0], a[1], a[2], src, a[4], a[5]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error()
    # language is not needed at F = 0; P = 0 succeeds and launches nothing, whatever the pointers
    assert L.olsr_map_ply_pack(0, 1, 0, None, None, None) == 0
    assert L.olsr_map_ply_pack(0, 16, 32, C.byref(_buffers()), PTR, None) == 0
    assert L.olsr_map_ply_pack(0, 2, 0, None, None, None) == _abi.OLSR_ERR_ARG


def _table(M, F, **changes):
    t = list(range(14 + 3 * M + F))
    for j, v in changes.items():
        t[int(j)] = v
    return (C.c_int32 * len(t))(*t)


def test_unpack_argument_errors(L):
    M, F = 1, 15
    width = 14 + 3 * M + F
    # P, M, F, n_cols, col, rows, dst, stream
    ok = [100, M, F, width, _table(M, F), PTR, _buffers(), None]
    rows = [("col", {4: None}), ("rows", {5: None}), ("dst", {6: None}), ("P < 0", {0: -1}), ("M = 0", {1: 0}), ("M = 3", {1: 3}),
            ("M = 17", {1: 17}), ("F < 0", {2: -1}), ("F = 33", {2: 33}), ("n_cols = 0", {3: 0}), ("n_cols < 0", {3: -4}),
            ("n_cols beyond the limit", {3: _abi.MAP_PLY_MAX_COLS + 1}), ("col[j] >= n_cols", {4: _table(M, F, **{"0": width})}),
            ("col[j] >= n_cols", {3: width - 1}), ("col[j] < -1", {4: _table(M, F, **{"7": -2})}),
            ("rows alignment", {5: PTR + 1})]
    # -1 anywhere but on a normal or a language channel
    rows += [(f"col[{j}] = -1", {4: _table(M, F, **{str(j): -1})}) for j in (0, 1, 2, 6, 7, 8, 24, 25, 27, 28, 31)]
    rows += [(f"dst.{k}", {6: _buffers(**{k: None})}) for k in ("means3D", "shs", "opacities", "scales", "rotations", "language")]
    for what, change in rows:
        a = list(ok)
        for k, v in change.items():
            a[k] = v
        dst = None if a[6] is None else C.byref(a[6])
        assert L.olsr_map_ply_unpack(a[0], a[1], a[2], a[3], a[4], a[5], dst, a[7]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error()
    # P = 0 succeeds and launches nothing: with -1 on the normals and on language channels, and with extra file columns
    absent = _table(M, F, **{str(j): -1 for j in (3, 4, 5, 9, 23)})
    assert L.olsr_map_ply_unpack(0, M, F, width, absent, None, None, None) == 0
    assert L.olsr_map_ply_unpack(0, M, F, width + 40, absent, None, None, None) == 0
    assert L.olsr_map_ply_unpack(0, M, F, width, _table(M, F, **{"0": -1}), None, None, None) == _abi.OLSR_ERR_ARG
    assert L.olsr_map_ply_unpack(0, 16, 32, 94, _table(16, 32), None, None, None) == 0


def test_a_gpu_is_required():
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    with pytest.raises(RuntimeError, match="GPU"):
        GaussianMap.load_ply("nowhere.ply", {}, "cpu")
    for name in ("save_ply", "load_ply", "save_state", "load_state", "blank"):
        assert callable(getattr(GaussianMap, name))


# ---- the session's trajectory files ----------------------------------------------------------------------------------------
def _rigid(angle, axis, t):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def test_save_trajectory(tmp_path):
    from online_lang_splatting_amd.slam import OnlineSlam, ate_rmse, ate_statistics
    # three ground-truth camera-to-world poses; the estimate is the same trajectory in a world moved by one rigid offset
    gt_c2w = [_rigid(0.1 * k, (0.2, 1.0, 0.1), (0.3 * k, 0.05 * k * k, 0.1 * k)) for k in range(3)]
    offset = _rigid(0.4, (1.0, 0.3, -0.5), (0.7, -0.2, 1.1))
    ids = [0, 4, 9]
    gt_w2c = {i: torch.from_numpy(np.linalg.inv(T)).float() for i, T in zip(ids, gt_c2w)}
    gt_w2c[5] = torch.eye(4)                                   # a frame that is no keyframe is not looked at
    slam = OnlineSlam.__new__(OnlineSlam)                      # host only: keyframes and poses are all save_trajectory reads
    slam.keyframes = list(ids)
    slam.poses = {i: torch.from_numpy(np.linalg.inv(offset @ T)).float() for i, T in zip(ids, gt_c2w)}
    slam.poses[5] = torch.eye(4)
    rmse = slam.save_trajectory(str(tmp_path), gt_w2c, iterations=37)
    rmse_final = slam.save_trajectory(str(tmp_path), gt_w2c, final=True)
    assert sorted(os.listdir(tmp_path / "plot")) == ["stats_0037.json", "stats_final.json", "trj_0037.json", "trj_final.json"]
    trj = json.load(open(tmp_path / "plot" / "trj_0037.json"))
    assert sorted(trj) == ["trj_est", "trj_gt", "trj_id"] and trj["trj_id"] == ids
    assert trj == json.load(open(tmp_path / "plot" / "trj_final.json"))
    for key, w2c in (("trj_est", slam.poses), ("trj_gt", gt_w2c)):
        got = np.array(trj[key])
        assert got.shape == (3, 4, 4) and got.dtype == np.float64
        for k, i in enumerate(ids):
            want = np.linalg.inv(w2c[i].numpy().astype(np.float64))     # the float64 inverse of the float32 pose
            assert np.array_equal(got[k], want), (key, i)
    stats = json.load(open(tmp_path / "plot" / "stats_0037.json"))
    assert sorted(stats) == ["max", "mean", "median", "min", "rmse", "sse", "std"]
    est = torch.stack([slam.poses[i] for i in ids])
    gt = torch.stack([gt_w2c[i] for i in ids])
    assert stats == ate_statistics(est, gt) and stats["rmse"] == rmse == rmse_final == ate_rmse(est, gt)
    # a rigid offset aligns away: what is left is float32 rounding of the poses (entries of order 1: 2^-24 each)
    assert 0.0 <= rmse < 1e-6 and stats["max"] < 1e-6 and stats["min"] <= stats["median"] <= stats["max"]
    assert abs(stats["sse"] - 3 * rmse * rmse) <= 1e-12 * max(stats["sse"], 1e-30) + 1e-30
    with pytest.raises(ValueError):
        slam.save_trajectory(str(tmp_path), gt_w2c)
    assert not [n for n in os.listdir(tmp_path / "plot") if n.endswith(".tmp")]
