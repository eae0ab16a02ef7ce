"""The sizing functions of include/olsr.h against their own carve (no GPU): with the carve log on, a sizing function's
null-base carve must hand out ascending, 256-byte aligned, disjoint ranges that end at least 256 bytes (the slack a base that
is not 256-byte aligned uses up) before the size it returns, and the size must not shrink when a size argument grows — a
buffer sized for a capacity must hold every smaller count (olsr_forward_async carves a capacity-sized binning buffer).

Every scratch of more than one array, and every one whose base the library rounds up, is carved.  The two sizing functions
whose entries still lay their buffer out by hand leave no records: they are listed with carved=False, checked for monotony
alone, and must indeed leave none.  olsr_backward_scratch_bytes sizes a single array and its byte count takes part in the
drop-in backward's row policy; olsr_hr_net_workspace_bytes sizes a workspace whose 16-byte alignment is an argument check and
whose exact size tests/test_hr_net_abi_cpu.py pins.

The two radix sorts' status words: whatever keys-per-thread and block shape the plan picks or a test forces, the rows the
passes publish (blocks x 128 words x 4 passes) fit the room the state's carve leaves for them behind the tickets, digit totals
and look-back words (olsr_debug_sort_status_room, computed from the carve itself)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from online_lang_splatting_amd import _abi
from online_lang_splatting_amd._lib import carve_log_read, lib

F_ALL = (0, 3, 15, 16, 32)
SWEEP = sorted(set(range(0, 9001)) | {(1 << k) + d for k in range(0, 23) for d in (-1, 0, 1)})
LIMIT = (1 << 31) - 1   # the entries take int32 counts: combinations whose element count passes it are outside every contract


def _log(L):
    return np.array(carve_log_read(), dtype=np.int64).reshape(-1, 3)


def _lang_query_bytes(L, n_pos, w, h):
    p = _abi.OlsrLangQueryParams()
    p.n_pos, p.out_width, p.out_height = n_pos, w, h
    return L.olsr_lang_query_scratch_bytes(C.byref(p))


# name, call(L, *sizes), per size argument: (swept from, the values it takes while another argument is swept[, swept up to]),
# further arguments that are no sizes (every combination), carved by Carver
ROWS = [
    ("olsr_geometry_bytes", lambda L, P, F: L.olsr_geometry_bytes(P, F), [(0, None)], [F_ALL], True),
    ("olsr_binning_bytes", lambda L, R, F: L.olsr_binning_bytes(R, F), [(0, None)], [F_ALL], True),
    ("olsr_image_bytes", lambda L, w, h, t: L.olsr_image_bytes(w, h, t), [(0, (1, 37)), (0, (1, 37))], [(15, 16)], True),
    ("olsr_knn_scratch_bytes", lambda L, P: L.olsr_knn_scratch_bytes(P), [(0, None)], [], True),
    ("olsr_emd_scratch_bytes", lambda L, B, a, b: L.olsr_emd_scratch_bytes(B, a, b), [(0, (1, 3)), (0, (0, 5)), (0, (0, 5))], [], True),
    ("olsr_chamfer_scratch_bytes", lambda L, B, a, b: L.olsr_chamfer_scratch_bytes(B, a, b), [(0, (1, 3)), (0, (0, 5)), (0, (0, 5))], [],
     True),
    ("olsr_query_eval_scratch_bytes", lambda L, P, H, W: L.olsr_query_eval_scratch_bytes(P, H, W), [(1, (1, 7), 65535), (2, (2, 33), 1 << 20), (2, (2, 33), 1 << 20)],
     [], True),   # (its documented domain: 1 <= P <= 65535, 2 <= H, W <= 2^20)
    ("olsr_image_psnr_scratch_bytes", lambda L: L.olsr_image_psnr_scratch_bytes(), [], [], True),
    ("olsr_debug_backward_ordered_scratch_bytes", lambda L, R, F: L.olsr_debug_backward_ordered_scratch_bytes(R, F), [(0, None)], [F_ALL],
     True),
    ("olsr_fused_loss_scratch_bytes", lambda L, w, h, t: L.olsr_fused_loss_scratch_bytes(w, h, t), [(1, (1, 37)), (1, (1, 37))], [(15, 16)],
     True),
    ("olsr_mapping_loss_scratch_bytes", lambda L, w, h: L.olsr_mapping_loss_scratch_bytes(w, h), [(0, (1, 37)), (0, (1, 37))], [], True),
    ("olsr_refinement_loss_scratch_bytes", lambda L, w, h: L.olsr_refinement_loss_scratch_bytes(w, h), [(0, (1, 37)), (0, (1, 37))], [], True),
    ("olsr_isotropic_reg_scratch_bytes", lambda L, P: L.olsr_isotropic_reg_scratch_bytes(P), [(0, None)], [], True),
    ("olsr_map_edit_scratch_bytes", lambda L, P: L.olsr_map_edit_scratch_bytes(P), [(0, None)], [], True),
    ("olsr_keyframe_seed_scratch_bytes", lambda L, W, H: L.olsr_keyframe_seed_scratch_bytes(W, H), [(1, (1, 37)), (1, (1, 37))], [], True),
    ("olsr_frontend_scratch_bytes", lambda L, n: L.olsr_frontend_scratch_bytes(n), [(0, None)], [], True),
    ("olsr_lang_ae_scratch_bytes", lambda L, N: L.olsr_lang_ae_scratch_bytes(N), [(0, None)], [], True),
    ("olsr_lang_query_scratch_bytes", _lang_query_bytes, [(0, (1, 3)), (1, (1, 33)), (1, (1, 33))], [], True),
    ("olsr_tsdf_surface_scratch_bytes", lambda L, X, Y, Z: L.olsr_tsdf_surface_scratch_bytes(X, Y, Z),
     [(0, (1, 7)), (0, (1, 7)), (0, (1, 7))], [], True),
    ("olsr_tsdf_mesh_scratch_bytes", lambda L, X, Y, Z: L.olsr_tsdf_mesh_scratch_bytes(X, Y, Z), [(0, (1, 7)), (0, (1, 7)), (0, (1, 7))],
     [], True),
    # ---- laid out by hand: the size alone.  The row scratch is a single array whose byte count takes part in the drop-in
    # backward's row policy; the workspace's 16-byte alignment is an argument check and its exact size is pinned
    ("olsr_backward_scratch_bytes", lambda L, rows, F: L.olsr_backward_scratch_bytes(rows, F), [(0, None)], [F_ALL], False),
    ("olsr_hr_net_workspace_bytes", lambda L, h, w: L.olsr_hr_net_workspace_bytes(h, w, 1, 1, 1, 1), [(1, (1, 3)), (1, (1, 3))], [], False),
]


def test_every_sizing_function_has_a_row():
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "olsr.h")).read()
    declared = set(re.findall(r"^size_t (olsr_\w+_bytes)\(", header, flags=re.M))
    assert declared == {r[0] for r in ROWS}, declared ^ {r[0] for r in ROWS}


def test_every_entry_has_a_row_or_a_reason():
    """tests/test_gpu_extents.py: COVERED (the entries its rows run) and NO_ROW (entry -> why it has none) together are
    exactly the functions include/olsr.h declares."""
    import re
    import test_gpu_extents as T
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "olsr.h")).read()
    declared = set(re.findall(r"^(?:const \w+ \*|\w+ \*?)\s*(olsr_\w+)\(", header, flags=re.M))
    assert len(declared) > 90
    assert not set(T.COVERED) & set(T.NO_ROW), set(T.COVERED) & set(T.NO_ROW)
    for name, reason in T.NO_ROW.items():   # the only reasons: nothing of the caller's on the device is written
        assert reason.startswith(T.REASONS), (name, reason)
    assert declared == set(T.COVERED) | set(T.NO_ROW), declared ^ (set(T.COVERED) | set(T.NO_ROW))
    import extent_harness
    source = open(T.__file__).read() + open(extent_harness.__file__).read()
    for name in T.COVERED:   # a covered entry is called somewhere in the file or in its harness
        assert f".{name}(" in source, name


def _check_carve(name, args, log, total):
    assert len(log) > 0, f"{name}{args}: no carve records"
    base, off, nbytes = log[:, 0], log[:, 1], log[:, 2]
    assert not base.any(), f"{name}{args}: a sizing carve has a base"
    assert not (off % 256).any(), f"{name}{args}: offsets {off.tolist()}"
    end = off + nbytes
    # ascending and disjoint: a range starts where its predecessor has ended, or later
    assert (off[1:] >= end[:-1]).all() and (np.diff(off) >= 0).all(), f"{name}{args}: ranges {log[:, 1:].tolist()}"
    assert int(end[-1]) + 256 <= total, f"{name}{args}: the last range ends at {int(end[-1])}, the size is {total}"


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_sizing_function(row):
    name, call, sizes, others, carved = row
    L = lib()
    L.olsr_debug_carve_log(0)
    try:
        for rest in itertools.product(*others):
            if not sizes:
                L.olsr_debug_carve_log(1)
                total = call(L, *rest)
                log = _log(L)
                L.olsr_debug_carve_log(0)
                _check_carve(name, rest, log, total) if carved else None
                continue
            for axis, spec in enumerate(sizes):
                first, last = spec[0], (spec[2] if len(spec) > 2 else LIMIT)
                held = [s[1] for i, s in enumerate(sizes) if i != axis]
                for fixed in itertools.product(*held):
                    prev = -1
                    for v in SWEEP:
                        if v < first:
                            continue
                        if v > last:
                            break
                        args = list(fixed)
                        args.insert(axis, v)
                        if int(np.prod(args, dtype=np.float64)) > LIMIT:
                            break
                        L.olsr_debug_carve_log(1)
                        total = call(L, *args, *rest)
                        log = _log(L)
                        L.olsr_debug_carve_log(0)
                        if carved:
                            _check_carve(name, tuple(args) + rest, log, total)
                        else:
                            assert len(log) == 0, f"{name} is carved by Carver now: give it carved=True"
                        assert total >= prev, f"{name}: {total} bytes at {tuple(args) + rest}, {prev} bytes one step below"
                        prev = total
    finally:
        L.olsr_debug_carve_log(0)


def test_log_is_per_call_and_off_by_default():
    L = lib()
    L.olsr_debug_carve_log(0)
    L.olsr_geometry_bytes(1000, 15)
    assert L.olsr_debug_carve_log_read(None, 0) == 0          # off: nothing is recorded
    L.olsr_debug_carve_log(1)
    try:
        L.olsr_image_bytes(45, 30, 15)
        n = L.olsr_debug_carve_log_read(None, 0)
        assert n == 6                                          # ImageState's six arrays
        out = (C.c_uint64 * 6)()
        assert L.olsr_debug_carve_log_read(out, 2) == n        # the count, however few are copied
        assert list(out) == [0, 0, 45 * 30 * 4, 0, 5632, 45 * 30 * 4]
        L.olsr_debug_carve_log(1)                              # switching it on again clears it
        assert L.olsr_debug_carve_log_read(None, 0) == 0
    finally:
        L.olsr_debug_carve_log(0)
    assert L.olsr_debug_carve_log_read(None, 0) == 0


def seeded_sort_knobs():
    """(keys per thread, legacy, one-launch sort, compaction): the values the library seeded from the environment when it was
    loaded (csrc/olsr_diag.hip), which is what a test that forces a knob puts back."""
    def num(name, default=0):
        try:
            return int(os.environ.get(name, "") or default)
        except ValueError:
            return 0   # (atoi)
    return (num("OLSR_SORT_KPT"), 1 if num("OLSR_SORT_LEGACY") == 1 else 0, 1 if num("OLSR_SORT_SMALL", 1) != 0 else 0,
            1 if num("OLSR_SORT_COMPACT", 1) != 0 else 0)


def _status_words(L, n, binning):
    """The words the state's carve leaves for the passes' status rows (whole rows of 128 words), and that they lie inside the
    largest range the carve logged."""
    L.olsr_debug_carve_log(1)
    L.olsr_binning_bytes(n, 0) if binning else L.olsr_geometry_bytes(n, 0)
    log = _log(L)
    L.olsr_debug_carve_log(0)
    room = int(L.olsr_debug_sort_status_room(n, 1 if binning else 0))
    assert 0 <= room * 4 <= int(log[:, 2].max()), (n, binning, room)
    return room // 128 * 128


def test_sort_status_rows_fit_the_carve():
    L = lib()
    threads0 = L.olsr_debug_sort_threads(-1)
    kpt0 = seeded_sort_knobs()[0]
    kpt, blocks = C.c_int32(0), C.c_int32(0)
    try:
        for n in SWEEP:
            room = (_status_words(L, n, False), _status_words(L, n, True))
            for threads in (256, 1024):
                L.olsr_debug_sort_threads(threads)
                for forced in (0, 2, 4, 8, 12, 16):
                    L.olsr_debug_sort_knobs(forced, -1, -1)
                    for cap in (0, 1):
                        if not L.olsr_debug_sort_plan(n, cap, C.byref(kpt), C.byref(blocks)):
                            continue
                        need = blocks.value * 128 * 4
                        assert blocks.value * threads * kpt.value >= n, (n, threads, forced, cap, kpt.value, blocks.value)
                        assert need <= min(room), (f"n={n} threads={threads} forced kpt={forced} capacity={cap}: {blocks.value} blocks of "
                                                   f"{kpt.value} keys per thread need {need} status words, the carve has {room}")
    finally:
        L.olsr_debug_sort_knobs(kpt0, -1, -1)
        L.olsr_debug_sort_threads(threads0)
        L.olsr_debug_carve_log(0)
