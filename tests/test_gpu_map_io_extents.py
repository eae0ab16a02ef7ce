"""Neither entry of include/olsr_map_io.h writes outside the bytes it asked for: the extents rows of olsr_map_ply_pack and
olsr_map_ply_unpack, the way tests/test_gpu_single_stage_extents.py holds its header's, on tests/extent_harness.py as it is.

| entry               | shapes (P, M, F)                          | why these                                              | scratch |
| olsr_map_ply_pack   | (1,1,15) (255,1,15) (256,1,0) (257,4,3)   | 64 rows per block; width 17 is never 16-byte aligned   | none    |
| olsr_map_ply_unpack | the same, n_cols = width and width + 3    | fewer rows per block once n_cols > 94: (257,16,32) + 3 | none    |

Each entry runs three ways: plain buffers, guarded outputs (64 KiB of a known byte on either side, every output pre-filled
with a pattern no input holds), and guarded outputs AND inputs that start 4 bytes past a 256-byte boundary (bases that are
4-byte but not 16-byte aligned: the scalar heads and tails of every span).  Checked: the guards are intact; pack stored every
word of its P * width * 4 bytes; unpack stored every word of rows [0, P) of each destination array and left the rows from P
on with their pre-fill; the guarded runs give the plain run's bits, and those are the restated record's
(tests/map_io_ref.py).  Inputs hold no pre-fill word and every output word must differ from it afterwards, so a word that was
stored from memory the kernel had not filled (an LDS word read before it was written) shows as wrong bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import extent_harness as H
import map_io_ref as R
from online_lang_splatting_amd import _abi

pytestmark = pytest.mark.gpu
DEV = H.DEV
F32 = torch.float32
SPARE = 9      # destination rows beyond P
SHAPES = [(1, 1, 15), (255, 1, 15), (256, 1, 0), (257, 4, 3)]

COVERED = ("olsr_map_ply_pack", "olsr_map_ply_unpack")


def _L():
    from online_lang_splatting_amd._lib import lib
    return lib()


def _check_rc(rc):
    from online_lang_splatting_amd._lib import check
    check(rc)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


@pytest.fixture(autouse=True)
def _forget_buffers():
    yield
    H.reset()


def finite_map(P, M, F, seed):
    """Parameter arrays without a NaN (H.check looks for its NaN pre-fill) and without a zero language word."""
    g = np.random.default_rng(seed)
    shape = dict(means3D=(P, 3), shs=(P, M, 3), opacities=(P, 1), scales=(P, 3), rotations=(P, 4), language=(P, F))
    return {k: (g.standard_normal(s).astype(np.float32) + np.float32(3.0)) for k, s in shape.items()}


def placed(a, misalign):
    """A device copy of `a`: a plain tensor (misalign None) or a guarded one `misalign` bytes past a 256-byte boundary."""
    if misalign is None:
        return torch.from_numpy(a).to(DEV)
    t = H.guarded_tensor(a.shape, F32, misalign)
    if t.numel():
        t.copy_(torch.from_numpy(a))
    return t


def struct(t):
    p = lambda k: t[k].data_ptr() if k in t and t[k].numel() else None  # noqa: E731
    return _abi.OlsrMapBuffers(**{k: p(k) for k in ("means3D", "shs", "opacities", "scales", "rotations", "language")})


@pytest.mark.parametrize("P,M,F", SHAPES)
def test_map_ply_pack(hip, P, M, F):
    L = _L()
    a = finite_map(P, M, F, seed=P)
    want = R.record(a["means3D"], a["shs"], a["opacities"], a["scales"], a["rotations"], a["language"])
    width = 14 + 3 * M + F
    results = []
    for misalign in (None, 0, 4):
        H.reset()
        src = {k: placed(v, None if misalign is None else misalign) for k, v in a.items()}
        out = torch.empty(P, width, dtype=F32, device=DEV) if misalign is None else H.guarded_tensor((P, width), F32, misalign)
        s = struct(src)
        _check_rc(L.olsr_map_ply_pack(P, M, F, C.byref(s), out.data_ptr(), _stream()))
        if misalign is not None:
            assert out.data_ptr() % 256 == misalign
            H.check([out] + [t for t in src.values() if t.numel()], (), [out])      # exactly P * width * 4 bytes, all stored
            for k, t in src.items():
                assert H.same_bits(t.cpu(), torch.from_numpy(a[k])), f"pack wrote its source {k}"
        torch.cuda.synchronize()
        results.append(out.cpu())
    assert H.same_bits(results[0], torch.from_numpy(want)), "the plain run differs from the restated record"
    assert H.same_bits(results[1], results[0]) and H.same_bits(results[2], results[0]), "a guarded run differs from the plain run"


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("P,M,F", SHAPES + [(257, 16, 32)])
def test_map_ply_unpack(hip, P, M, F, extra):
    L = _L()
    a = finite_map(P, M, F, seed=P + 1)
    want = R.record(a["means3D"], a["shs"], a["opacities"], a["scales"], a["rotations"], a["language"])
    width = 14 + 3 * M + F
    n_cols = width + extra
    body = np.full((P, n_cols), 7.0, dtype=np.float32)
    body[:, extra:] = want                                # the unknown columns lead each row
    col = (C.c_int32 * width)(*[j + extra for j in range(width)])
    shapes = dict(means3D=(P + SPARE, 3), shs=(P + SPARE, M, 3), opacities=(P + SPARE, 1), scales=(P + SPARE, 3),
                  rotations=(P + SPARE, 4), language=(P + SPARE, F))
    results = []
    for misalign in (None, 0, 4):
        H.reset()
        rows = placed(body, misalign)
        if misalign is None:
            dst = {k: H.prefill(torch.empty(s, dtype=F32, device=DEV)) for k, s in shapes.items()}
        else:
            dst = {k: H.guarded_tensor(s, F32, misalign) for k, s in shapes.items()}
        s = struct(dst)
        _check_rc(L.olsr_map_ply_unpack(P, M, F, n_cols, col, rows.data_ptr(), C.byref(s), _stream()))
        torch.cuda.synchronize()
        live = [t for t in dst.values() if t.numel()]
        if misalign is not None:
            H.check(live + [rows], (), [t[:P] for t in live])                          # rows [0, P): every word stored
            assert H.same_bits(rows.cpu(), torch.from_numpy(body)), "unpack wrote the file's rows"
        for k, t in dst.items():
            if t.numel():
                assert bool((t[P:].reshape(-1).view(torch.int32) == H.F32_PREFILL).all()), f"{k}: a row from P on was written"
        results.append({k: t[:P].cpu() for k, t in dst.items()})
    for k in a:
        assert H.same_bits(results[0][k], torch.from_numpy(a[k])), f"{k}: the plain run differs from the inputs"
        for r in results[1:]:
            assert H.same_bits(r[k], results[0][k]), f"{k}: a guarded run differs from the plain run"
