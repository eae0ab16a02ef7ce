"""The Gaussian map on disk: the reference's point_cloud.ply, and the resumable state as one .npz.

GaussianModel.save_ply (gaussian_splatting/scene/gaussian_model.py:478-563) copies seven arrays to the host, concatenates
them and builds one Python tuple per row; GaussianModel.load_ply (:585-689) looks every property up by name.  Here the record
array [P, 14 + 3 M + F] is packed on the device in the file's column order (olsr_map_ply_pack, include/olsr_map_io.h;
csrc/k_map_io.hip), leaves it in pinned chunks that are written while the next one is copied, and a file's body goes to the
device as it lies, where olsr_map_ply_unpack fills the map's own buffers.  The host handles nothing per row.

Per row, float32 (construct_list_of_attributes):
    x y z | nx ny nz (zeros) | f_dc_0..2 | f_rest_0..3(M-1)-1 | f_language_0..F-1 | opacity | scale_0..2 | rot_0..3
with f_dc_c = shs[p, 0, c] and f_rest_{c (M - 1) + k} = shs[p, 1 + k, c]; the parameters are the raw ones the map holds.

Stated deviations from the reference.  (1) load_ply reads the f_language_* channels (F=None: as many as the file has, F=0
drops them as the reference does).  (2) The header is restated from the PLY format and from what plyfile is known to write for
such a dtype — `plyfile` was not available to record it from.  (3) Only binary little-endian files whose vertex properties
are all float32 are read.

`save_state` / `load_state` write and read GaussianMap.state() — parameters, both Adam moments, kf_id, n_obs, stats,
max_radii, group_steps and the groups that skip the next step — as one .npz: the form a mapping job resumes from.  Both
writers go through `path + ".tmp"` and os.replace, so a periodic save never leaves half a file."""
import ctypes as C
import io
import os
from typing import BinaryIO, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _abi
from ._host import stream_ptr
from ._lib import check, lib

FLOAT_TYPES = ("float", "float32")
CHUNK_BYTES = 32 << 20        # the size of one pinned staging buffer of save_ply
MAX_HEADER_LINES = 1 << 16


def ply_width(M: int, F: int) -> int:
    """olsr_map_ply_width: 14 + 3 M + F (M a perfect square in 1 ... 16, F in 0 ... 32)."""
    w = int(lib().olsr_map_ply_width(int(M), int(F)))
    if w < 0:
        raise ValueError(f"a PLY record needs M in (1, 4, 9, 16) and F in 0 ... 32, not M = {M}, F = {F}")
    return w


def attribute_names(M: int, F: int) -> List[str]:
    """construct_list_of_attributes for shs [P,M,3] and language [P,F]: the record's columns in order."""
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * (M - 1))]
            + [f"f_language_{i}" for i in range(F)] + ["opacity"] + [f"scale_{i}" for i in range(3)]
            + [f"rot_{i}" for i in range(4)])


def ply_header(P: int, M: int, F: int) -> bytes:
    """The header of point_cloud.ply for P rows: what plyfile's PlyData([PlyElement.describe(elements, "vertex")]).write
    emits for an all-"f4" dtype — restated from the PLY format and plyfile's known output, not recorded from it."""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(P)}"]
    lines += [f"property float {n}" for n in attribute_names(M, F)]
    lines.append("end_header")
    return ("\n".join(lines) + "\n").encode("ascii")


def read_ply_header(f: BinaryIO) -> Tuple[int, List[Tuple[str, str]], int]:
    """The header of a binary little-endian PLY whose first element is `vertex` with float32 properties only.
    -> (P, [(property name, type as written)], the body's offset in bytes).  `comment` and `obj_info` lines are skipped,
    elements after the first are ignored.  ValueError: not a PLY, an ascii or big-endian body, a first element that is not
    `vertex`, a list property or one that is not float / float32, no end_header, a body shorter than P n_cols 4 bytes."""
    f.seek(0)
    if f.readline().strip() != b"ply":
        raise ValueError("not a PLY file (the first line is not 'ply')")
    fmt, P, props, elements, ended = None, None, [], 0, False
    for _ in range(MAX_HEADER_LINES):
        raw = f.readline()
        if not raw:
            break
        try:
            words = raw.decode("ascii").split()
        except UnicodeDecodeError:
            raise ValueError("the PLY header is not ASCII (no end_header before the body?)") from None
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            ended = True
            break
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else ""
        elif words[0] == "element":
            elements += 1
            if elements == 1:
                if len(words) != 3 or words[1] != "vertex":
                    raise ValueError(f"the first element of the PLY must be 'vertex', not {' '.join(words[1:2])!r}")
                P = int(words[2])
                if P < 0:
                    raise ValueError("element vertex: a negative count")
        elif words[0] == "property":
            if elements == 0:
                raise ValueError("a property ahead of the first element")
            if elements > 1:
                continue
            if len(words) > 1 and words[1] == "list":
                raise ValueError(f"list property {words[-1]!r}: only float32 scalars are read")
            if len(words) != 3 or words[1] not in FLOAT_TYPES:
                raise ValueError(f"property {' '.join(words[1:])!r}: only float / float32 properties are read")
            props.append((words[2], words[1]))
        else:
            raise ValueError(f"unknown PLY header line {' '.join(words)!r}")
    if not ended:
        raise ValueError("the PLY header has no end_header")
    if fmt != "binary_little_endian":
        raise ValueError(f"PLY format {fmt!r}: only binary_little_endian is read")
    if P is None:
        raise ValueError("the PLY has no vertex element")
    if P > 0 and not props:
        raise ValueError("the vertex element has no property")
    offset = f.tell()
    size = f.seek(0, io.SEEK_END)
    if size - offset < P * len(props) * 4:
        raise ValueError(f"the PLY body holds {size - offset} bytes, {P} rows of {len(props)} floats need {P * len(props) * 4}")
    f.seek(offset)
    return P, props, offset


def _numbered(names: Dict[str, int], prefix: str) -> List[int]:
    """The file columns of prefix0, prefix1, ... (every index present exactly once)."""
    found = {n: c for n, c in names.items() if n.startswith(prefix) and n[len(prefix):].isdigit()}
    cols = []
    for i in range(len(found)):
        if f"{prefix}{i}" not in found:
            raise ValueError(f"the PLY's {prefix}* properties are not numbered 0 ... {len(found) - 1}")
        cols.append(found[f"{prefix}{i}"])
    return cols


def column_table(props, F: Optional[int] = None) -> Tuple[int, int, List[int]]:
    """load_ply's lookup by name: -> (M, F, col) with col[j] the file column that feeds record column j of
    attribute_names(M, F), -1 for the normals when the file has none and for language channels it lacks.  Unknown
    properties are ignored.  F=None: the file's language channels; 0: none; else the file's count must be F or 0 (zeros)."""
    names = {}
    for c, (n, _) in enumerate(props):
        if n in names:
            raise ValueError(f"the PLY names property {n!r} twice")
        names[n] = c
    rest, lang = _numbered(names, "f_rest_"), _numbered(names, "f_language_")
    M = 1 + len(rest) // 3
    if len(rest) % 3 or M not in (1, 4, 9, 16):
        raise ValueError(f"{len(rest)} f_rest_* properties: 3 (M - 1) with M a perfect square <= 16 is expected")
    if F is None:
        F = len(lang)
    elif F != 0 and len(lang) not in (0, F):
        raise ValueError(f"the PLY has {len(lang)} language channels, F = {F} was asked for")
    if not 0 <= F <= _abi.MAP_PLY_MAX_F:
        raise ValueError(f"F = {F}: 0 ... {_abi.MAP_PLY_MAX_F} language channels")
    col = []
    for j, n in enumerate(attribute_names(M, F)):
        optional = 3 <= j < 6 or n.startswith("f_language_")
        if n not in names and not optional:
            raise ValueError(f"the PLY lacks property {n!r}")
        col.append(names.get(n, -1))
    return M, F, col


def _need_gpu(device, what):
    if torch.device(device).type != "cuda":
        raise RuntimeError(f"{what} packs the record on the GPU: the map must live on one (no CPU path)")


def pack_rows(gmap) -> torch.Tensor:
    """The record array [P, 14 + 3 M + F] of a GaussianMap, on its device (one launch on the current stream)."""
    _need_gpu(gmap.device, "save_ply")
    if gmap.M == 0:
        raise ValueError("a map without spherical harmonics (M = 0) has no PLY record: the reference always has f_dc")
    width = ply_width(gmap.M, gmap.F)
    rows = torch.empty(gmap.P, width, dtype=torch.float32, device=gmap.device)
    src = gmap._struct(gmap._bufs[gmap._front])
    check(lib().olsr_map_ply_pack(gmap.P, gmap.M, gmap.F, C.byref(src), rows.data_ptr() if gmap.P else None, stream_ptr(gmap.device)))
    return rows


def _replace_with(path: str, write):
    """write(file) into path + ".tmp", then os.replace: the file at `path` is always a whole one."""
    path = os.fspath(path)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)   # mkdir_p
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            write(f)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def save_ply(gmap, path: str):
    """GaussianModel.save_ply: the map as point_cloud.ply.  The record leaves the device in chunks of CHUNK_BYTES through two
    pinned buffers; a chunk is written while the next one is copied."""
    rows = pack_rows(gmap)
    P, width = rows.shape
    chunk = max(1, CHUNK_BYTES // (4 * width))
    starts = list(range(0, P, chunk))
    stage = [torch.empty(min(chunk, P), width, dtype=torch.float32, pin_memory=True) for _ in range(min(2, len(starts)))]
    done = [torch.cuda.Event() for _ in stage]
    stream = torch.cuda.current_stream(gmap.device)

    def fetch(k):
        n = min(chunk, P - starts[k])
        stage[k % 2][:n].copy_(rows[starts[k]:starts[k] + n], non_blocking=True)
        done[k % 2].record(stream)
        return n

    def write(f):
        f.write(ply_header(P, gmap.M, gmap.F))
        n = fetch(0) if starts else 0
        for k in range(len(starts)):
            n_next = fetch(k + 1) if k + 1 < len(starts) else 0
            done[k % 2].synchronize()
            f.write(memoryview(stage[k % 2][:n].numpy()).cast("B"))
            n = n_next
    _replace_with(path, write)


def load_ply(path: str, lrs: Dict[str, float], device, F: Optional[int] = None, capacity: Optional[int] = None,
             percent_dense=0.01):
    """GaussianModel.load_ply -> a GaussianMap: the parameters from the file (properties found by name, in any order, unknown
    ones ignored), moments, statistics, max_radii, kf_id, n_obs and group_steps zero (:685-689)."""
    from .gaussian_map import GaussianMap
    _need_gpu(device, "load_ply")
    dev = torch.device(device)
    with open(path, "rb") as f:
        P, props, _ = read_ply_header(f)
        M, F, col = column_table(props, F)
        n_cols = len(props)
        if n_cols > _abi.MAP_PLY_MAX_COLS:
            raise ValueError(f"{n_cols} properties per vertex: at most {_abi.MAP_PLY_MAX_COLS} are read")
        host = torch.empty(P * n_cols, dtype=torch.float32, pin_memory=P > 0)
        if P > 0:
            got = f.readinto(memoryview(host.numpy()).cast("B"))
            if got != P * n_cols * 4:
                raise ValueError(f"the PLY body ended after {got} of {P * n_cols * 4} bytes")
    gmap = GaussianMap.blank(P, M, F, lrs, dev, capacity=capacity, percent_dense=percent_dense)
    if P > 0:
        rows = host.to(dev, non_blocking=True)
        table = (C.c_int32 * len(col))(*col)
        dst = gmap._struct(gmap._bufs[gmap._front])
        check(lib().olsr_map_ply_unpack(P, M, F, n_cols, table, rows.data_ptr(), C.byref(dst), stream_ptr(gmap.device)))
        torch.cuda.current_stream(dev).synchronize()   # `host` and `rows` may go once the copy and the launch have run
    return gmap


def save_state(gmap, path: str):
    """GaussianMap.state() as one .npz (np.savez, uncompressed): what load_state resumes from, bit for bit."""
    st = {k: (v if v is not None else torch.zeros(gmap.P, 0)).detach().cpu().numpy() for k, v in gmap.state().items()}
    st["pending_skip"] = np.array([n in gmap.pending_skip for n in _abi.ADAM_GROUPS], dtype=np.uint8)
    _replace_with(path, lambda f: np.savez(f, **st))


def load_state(path: str, lrs: Dict[str, float], device, capacity: Optional[int] = None, percent_dense=0.01):
    """A GaussianMap from save_state's file, through GaussianMap.from_state; the groups that were to skip the next Adam step
    (an edit since the last one) still do."""
    from .gaussian_map import GaussianMap
    with np.load(path) as z:
        st = {k: torch.from_numpy(z[k]) for k in z.files}
    skip = st.pop("pending_skip", None)
    gmap = GaussianMap.from_state(st, lrs, device, capacity=capacity, percent_dense=percent_dense)
    if skip is not None:
        gmap.pending_skip = {n for n, s in zip(_abi.ADAM_GROUPS, skip.tolist()) if s}
    return gmap
