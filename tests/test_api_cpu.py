"""Host-side logic that needs no GPU: the C-ABI library loads and exports every symbol that
include/olsr.h declares, buffer-size functions behave, the Python API validates arguments with
the reference's exceptions, and the product never silently falls back to the CPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import build
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    from online_lang_splatting_amd import _lib
    return _lib.lib()


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "olsr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(olsr_[a-z0-9_]+)\s*\(", src)) - {"olsr_alloc_fn"})


def test_library_exports_every_declared_symbol(L):
    from online_lang_splatting_amd import _lib
    declared = _declared_functions()
    assert len(declared) >= 14
    assert sorted(_lib.EXPORTS) == declared
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name


def test_buffer_sizes(L):
    g1, g2 = L.olsr_geometry_bytes(1000, 15), L.olsr_geometry_bytes(500000, 15)
    assert 0 < g1 < g2
    assert g2 >= 500000 * (4 + 8 + 16 + 24 + 12 + 3 + 4 * 6)
    assert L.olsr_image_bytes(1200, 680, 15) >= 1200 * 680 * 8 + 80 * 46 * 8
    assert L.olsr_binning_bytes(1 << 20, 15) >= (1 << 20) * (5 * 4 + 1 + 4)  # keys x2, val, src, inst_gid, flags, rowbase
    # backward scratch: one row per live (instance, slot) pair, row stride = 10+F floats padded to 16
    s0, s15, s32 = (L.olsr_backward_scratch_bytes(1 << 20, F) for F in (0, 15, 32))
    assert s15 - s0 == (1 << 20) * 4 * (32 - 16) and s32 - s15 == (1 << 20) * 4 * (48 - 32)
    assert L.olsr_geometry_bytes(0, 0) > 0 and L.olsr_binning_bytes(0, 15) > 0 and L.olsr_backward_scratch_bytes(0, 15) > 0
    assert L.olsr_version().startswith(b"olsr")


def test_struct_layout_matches_header():
    from online_lang_splatting_amd._abi import OlsrScene
    # 10 int32 + 4 float + 13 pointers + 2 int32 + 1 pointer (tile_depth_cut, round 4) + 1 int64 (backward_row_capacity,
    # round 5), no implicit padding
    assert ctypes.sizeof(OlsrScene) == 10 * 4 + 4 * 4 + 13 * 8 + 2 * 4 + 8 + 8 + 8
    assert OlsrScene.background.offset == 56 and OlsrScene.cam_pos.offset == 56 + 12 * 8
    assert OlsrScene.tile_depth_cut.offset == 56 + 13 * 8 + 8
    assert OlsrScene.depth_order_carry.offset == 56 + 13 * 8 + 8 + 8 + 8
    from online_lang_splatting_amd._abi import OlsrGradBucket
    assert ctypes.sizeof(OlsrGradBucket) == 3 * 8 + 2 * 4 + 8 and OlsrGradBucket.row_mask.offset == 32


def test_c_abi_argument_errors(L):
    from online_lang_splatting_amd import _abi
    s = _abi.OlsrScene()
    s.P, s.width, s.height, s.tile, s.F = 10, 64, 64, 17, 15
    cb = _abi.ALLOC_FN(lambda u, n: None)
    R = ctypes.c_int32(0)
    rc = L.olsr_forward(ctypes.byref(s), cb, None, cb, None, cb, None, None, None, None, None, None, None,
                        ctypes.byref(R), None)
    assert rc == _abi.OLSR_ERR_ARG and b"tile" in L.olsr_last_error()
    s.tile, s.F = 15, 7
    rc = L.olsr_forward(ctypes.byref(s), cb, None, cb, None, cb, None, None, None, None, None, None, None,
                        ctypes.byref(R), None)
    assert rc == _abi.OLSR_ERR_ARG and b"language channels" in L.olsr_last_error()


def test_python_api_surface_and_exceptions():
    import diff_gaussian_rasterization as D
    from online_lang_splatting_amd import GaussianRasterizationSettings, LanguageGaussianRasterizer
    assert D.GaussianRasterizationSettings is GaussianRasterizationSettings
    assert GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "projmatrix_raw", "sh_degree", "campos", "prefiltered", "debug")
    rs = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), torch.eye(4), 0,
                                       torch.zeros(3), False, False)
    P = 4
    m, m2, o = torch.zeros(P, 3), torch.zeros(P, 3), torch.ones(P, 1)
    sh, col = torch.zeros(P, 1, 3), torch.zeros(P, 3)
    sc, rot, cov = torch.ones(P, 3), torch.zeros(P, 4), torch.zeros(P, 6)
    lang = torch.zeros(P, 15)
    for cls in (D.GaussianRasterizer, LanguageGaussianRasterizer):
        r = cls(rs)
        extra = dict(language_precomp=lang) if cls is LanguageGaussianRasterizer else {}
        with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
            r(m, m2, o, shs=None, colors_precomp=None, scales=sc, rotations=rot, **extra)
        with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
            r(m, m2, o, shs=sh, colors_precomp=col, scales=sc, rotations=rot, **extra)
        with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
            r(m, m2, o, shs=sh, scales=sc, rotations=None, **extra)
        with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
            r(m, m2, o, shs=sh, scales=sc, rotations=rot, cov3D_precomp=cov, **extra)
        # CPU tensors are refused loudly: there is no CPU fallback in the product
        with pytest.raises(RuntimeError, match="GPU"):
            r(m, m2, o, shs=sh, scales=sc, rotations=rot, **extra)
    with pytest.raises(RuntimeError, match=r"\(num_points, 3\)"):
        from online_lang_splatting_amd import _C
        _C.rasterize_gaussians(torch.zeros(3), torch.zeros(P, 4), col, o, sc, rot, 1.0, torch.empty(0), torch.eye(4),
                               torch.eye(4), torch.eye(4), 1.0, 1.0, 8, 8, torch.empty(0), 0, torch.zeros(3), False,
                               False)


def test_debug_settings_leave_a_snapshot_behind_on_failure(tmp_path, monkeypatch):
    """raster_settings.debug = True: a failing forward of the RGB rasterizer writes its CPU-copied arguments to
    snapshot_fw.dump before re-raising (DGR/diff_gaussian_rasterization/__init__.py:121-130); the language rasterizer does not
    (the reference has those lines commented out, :270-281)."""
    import diff_gaussian_rasterization as D
    from online_lang_splatting_amd import GaussianRasterizationSettings, LanguageGaussianRasterizer
    monkeypatch.chdir(tmp_path)
    rs = GaussianRasterizationSettings(8, 8, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), torch.eye(4), 0,
                                       torch.zeros(3), False, True)
    P = 4
    m, m2, o = torch.full((P, 3), 2.0), torch.zeros(P, 3), torch.ones(P, 1)
    sh, sc, rot = torch.zeros(P, 1, 3), torch.ones(P, 3), torch.zeros(P, 4)
    with pytest.raises(RuntimeError, match="GPU"):   # (CPU tensors: the product has no CPU path, so the call fails)
        LanguageGaussianRasterizer(rs)(m, m2, o, shs=sh, scales=sc, rotations=rot, language_precomp=torch.zeros(P, 15))
    assert not (tmp_path / "snapshot_fw.dump").exists()
    with pytest.raises(RuntimeError, match="GPU"):
        D.GaussianRasterizer(rs)(m, m2, o, shs=sh, scales=sc, rotations=rot)
    dump = torch.load(tmp_path / "snapshot_fw.dump")
    assert isinstance(dump, tuple) and torch.equal(dump[1], m) and dump[-1] is True   # (bg, means3D, ..., prefiltered, debug)


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "online_lang_splatting_amd")
    for dirpath, _dirs, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle_C" not in txt and "liboracle" not in txt and "import oracle" not in txt, f
    shim = open(os.path.join(ROOT, "diff_gaussian_rasterization", "__init__.py")).read()
    assert "oracle" not in shim


def test_scene_generator_is_deterministic():
    from online_lang_splatting_amd.scene import make_config_scene, make_scene
    a, b = make_scene(1000, 64, 48, 15, seed=3), make_scene(1000, 64, 48, 15, seed=3)
    for k in ("means3D", "opacities", "scales", "rotations", "shs", "language"):
        assert torch.equal(getattr(a, k), getattr(b, k))
    c = make_config_scene(1, P=500)
    assert c.shs.shape == (500, 16, 3) and c.F == 0 and c.sh_degree == 3
    assert torch.allclose(a.language.norm(dim=1), torch.ones(1000), atol=1e-5)
    assert torch.allclose(a.rotations.norm(dim=1), torch.ones(1000), atol=1e-5)


def test_compiled_torch_binding_loads_and_rejects_cpu_tensors():
    """The `_C` functions of DGR/ext.cpp:15-21 as a compiled torch extension (csrc/olsr_torch.cpp): it imports, holds
    the three entry points, reports the library's version, and — without a GPU — refuses a CPU tensor like the ctypes
    binding does."""
    from online_lang_splatting_amd import _C
    ext = _C.compiled_binding()
    assert ext is not None, getattr(_C.compiled_binding, "error", None)
    for name in ("forward", "backward", "mark_visible", "version"):
        assert callable(getattr(ext, name))
    assert ext.version() == _C.lib().olsr_version().decode()
    e = torch.empty(0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.forward(15, e, torch.zeros(4, 3), e, e, e, e, e, 1.0, e, e, e, e, 1.0, 1.0, 10, 10, e, 0, e, False, False,
                    15, 0, 1, 0)
    with pytest.raises(RuntimeError, match="num_points, 3"):
        ext.forward(15, e, torch.zeros(4, 2), e, e, e, e, e, 1.0, e, e, e, e, 1.0, 1.0, 10, 10, e, 0, e, False, False,
                    15, 0, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.mark_visible(torch.zeros(4, 3), e, e)


def test_binding_selector(monkeypatch):
    from online_lang_splatting_amd import _C
    monkeypatch.setenv("OLSR_BINDING", "ctypes")
    assert _C.compiled_binding() is None
    monkeypatch.setenv("OLSR_BINDING", "torch")
    assert _C.compiled_binding() is not None


def test_sort_plan_host_logic(L, monkeypatch):
    """Keys per thread / block count of the one-kernel radix passes (csrc/olsr_state.h: sort_plan): a round of at most
    256 resident blocks costs about (kpt + 11) us; status rows are reserved for the smallest chunk; 4096 blocks at
    most, beyond that the multi-kernel fallback."""
    L.olsr_debug_sort_knobs(0, 0, 0)
    kpt, nblk = ctypes.c_int32(), ctypes.c_int32()

    def plan(n, cap=0):
        ok = L.olsr_debug_sort_plan(n, cap, ctypes.byref(kpt), ctypes.byref(nblk))
        return ok, kpt.value, nblk.value
    # round 5: a scene with OLSR_FLAG_FRAMES_IN_FLIGHT sorts with four-wave (256-thread) blocks of sixteen keys per thread — they
    # get onto the CUs beside another frame's composite workgroups; olsr_debug_sort_threads forces a shape for every call
    assert L.olsr_debug_sort_threads(-1) == 0      # (default: the call decides; 1024 without the flag)
    assert L.olsr_debug_sort_threads(256) == 256
    for n in (1, 1023, 1024, 1025, 500_000, 2_700_146, 10_000_000, 60_000_000):
        ok, k, b = plan(n)
        assert ok == 1 and k == 16 and b == -(-n // (256 * 16)) and b <= 16384
    assert plan(16384 * 4096 + 1)[0] == 0          # more than 16 384 blocks even at kpt 16: the multi-kernel passes
    L.olsr_debug_sort_knobs(2, -1, -1)             # (kpt 2 does not exist for four-wave blocks: 4 runs)
    assert plan(500_000)[1] == 4
    L.olsr_debug_sort_knobs(0, -1, -1)
    assert L.olsr_debug_sort_threads(0) == 0       # the 1024-thread shape of rounds 2-4, below
    assert plan(500_000) == (1, 2, 245)            # the depth sort of the headline frame: one round at kpt 2
    assert plan(2_700_146) == (1, 12, 220)         # its tile sort: one round of 220 fat blocks
    ok, k, b = plan(3_440_000, 1)                  # the same sort launched against a capacity: planned for 85 % fill
    assert (ok, k) == (1, 12) and b == -(-3_440_000 // (1024 * 12))
    assert plan(3_440_000, 0)[1] == 16             # ... while an exact count of that size takes one round at kpt 16
    assert plan(0)[2] == 0
    for n in (1, 2047, 2048, 2049, 10_000_000, 60_000_000):
        ok, k, b = plan(n)
        assert ok == 1 and k in (2, 4, 8, 12, 16) and b == -(-n // (1024 * k)) and b <= 16384
    assert plan(4096 * 16384 + 1)[0] == 0          # beyond what the status rows are reserved for: the multi-kernel passes
    # the tuning knobs: set through the library (the environment is read once, at load), a forced value that would
    # overrun the status rows is ignored, a negative argument leaves a knob alone
    try:
        L.olsr_debug_sort_knobs(4, -1, -1)
        assert plan(500_000)[1:] == (4, 123)
        assert plan(40_000_000)[2] <= 16384
        L.olsr_debug_sort_knobs(-1, 64, -1)
        assert plan(500_000)[1:] == (4, 123)
        L.olsr_debug_sort_knobs(0, -1, -1)
        assert plan(500_000)[1] != 2  # 64 resident blocks per round: fatter blocks win
    finally:
        L.olsr_debug_sort_knobs(0, 0, 0)
    assert plan(500_000) == (1, 2, 245)
    assert L.olsr_debug_sort_threads(-1) == 0


def test_backward_row_policy_without_a_posted_count(L):
    """Host logic of the drop-in backward's scratch sizing (no GPU involved): with nothing posted for a token the bound of
    two rows per instance (packed survivor waves) or four (64-pixel slots) stands in, and waiting for a token that no
    forward ever issued times out."""
    import time
    assert L.olsr_backward_rows(0, 1, 1000, 15) == 2000
    assert L.olsr_backward_rows(0, 0, 1000, 15) == 4000
    assert L.olsr_backward_rows(0, 1, 0, 15) == 0 and L.olsr_backward_rows(0, 1, -5, 15) == 0
    assert L.olsr_live_rows(123, 1) == -1
    t0 = time.perf_counter()
    assert L.olsr_live_rows_wait(123, 1, 2000) == -1
    assert time.perf_counter() - t0 < 0.5
    assert L.olsr_last_forward_token() == 0  # (this thread issued no forward)


def test_backward_row_ratio_is_one_per_process_and_mode(L):
    """olsr_debug_rows_ratio: the rows-per-instance figure the drop-in backward guesses its scratch from is set and read
    per row layout, it reports the count of redone backwards, and both bindings' debug_rows_ratio read the same figure."""
    from online_lang_splatting_amd import _C
    redone = ctypes.c_int32(-1)
    keep = [L.olsr_debug_rows_ratio(m, -1.0, None) for m in (0, 1)]
    try:
        assert L.olsr_debug_rows_ratio(0, 0.25, ctypes.byref(redone)) == 0.25 and redone.value >= 0
        assert L.olsr_debug_rows_ratio(1, 1.5, None) == 1.5
        assert L.olsr_debug_rows_ratio(0, -1.0, None) == 0.25  # (setting one mode leaves the other alone)
        assert _C.debug_rows_ratio(False) == (0.25, redone.value) and _C.debug_rows_ratio(True) == (1.5, redone.value)
        assert _C.compiled_binding().debug_rows_ratio(True, -1.0) == (1.5, redone.value)
        assert _C.debug_rows_ratio(True, 0.0) == (0.0, redone.value)
    finally:
        for m, r in enumerate(keep):
            L.olsr_debug_rows_ratio(m, r, None)


def test_usable_cpus_respects_affinity_and_quota(monkeypatch, tmp_path):
    """The oracle's thread pool (and bench.py's cpu_baseline `cores`) is sized by the CPUs the container may use — the
    GPU box shows 256 hardware threads and grants 16 — not by os.cpu_count()."""
    import builtins
    import os
    from oracle import oracle_C
    n = oracle_C.usable_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)
    real_open = builtins.open

    def fake_open(path, *a, **k):
        if path == "/sys/fs/cgroup/cpu.max":
            p = tmp_path / "cpu.max"
            p.write_text("300000 100000\n")
            return real_open(p, *a, **k)
        return real_open(path, *a, **k)
    monkeypatch.setattr(builtins, "open", fake_open)
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(64)), raising=False)
    assert oracle_C.usable_cpus() == 3


def test_sparse_exchange_entries_validate_their_arguments(L):
    """The three local steps of the capacity-bound sparse exchange (include/olsr.h): argument errors come back before any
    launch, P == 0 is a no-op, and the scratch size is one int per 1024 rows."""
    from online_lang_splatting_amd import _abi
    assert L.olsr_sparse_exchange_scratch_ints(0) == 0 and L.olsr_sparse_exchange_scratch_ints(1) == 1
    assert L.olsr_sparse_exchange_scratch_ints(1024) == 1 and L.olsr_sparse_exchange_scratch_ints(500000) == 489
    assert L.olsr_sparse_exchange_mask(0, 29, None, None, None, None, None) == _abi.OLSR_OK
    assert L.olsr_sparse_exchange_mask(10, 0, None, None, None, None, None) == _abi.OLSR_ERR_ARG
    assert L.olsr_sparse_exchange_mask(10, 29, None, None, None, None, None) == _abi.OLSR_ERR_ARG
    assert b"must not be NULL" in L.olsr_last_error()
    assert L.olsr_sparse_exchange_pack(10, 29, 0, *([None] * 10)) == _abi.OLSR_ERR_ARG
    assert L.olsr_sparse_exchange_pack(10, 29, 4, *([None] * 10)) == _abi.OLSR_ERR_ARG
    assert L.olsr_sparse_exchange_pack(0, 29, 4, *([None] * 10)) == _abi.OLSR_OK
    assert L.olsr_sparse_exchange_unpack(10, 29, 4, None, None, None, None, None) == _abi.OLSR_ERR_ARG
    assert L.olsr_sparse_exchange_unpack(-1, 29, 4, None, None, None, None, None) == _abi.OLSR_ERR_ARG


def test_weak_scaling_poses_are_side_by_side_and_centred():
    """shard_cameras: what rank r of N renders in bench.py's weak-scaling mode - N poses 1.5 cm apart, no rotation, centred on
    the identity pose (N = 1: the identity pose itself), so that every rank's view costs what the N = 1 view costs."""
    import torch
    from online_lang_splatting_amd.scene import default_camera, shard_cameras
    ident = default_camera(1200, 680)
    one = shard_cameras(1200, 680, n=1)
    assert len(one) == 1 and torch.equal(one[0].world_view_transform, ident.world_view_transform)
    for n in (2, 4, 8):
        cams = shard_cameras(1200, 680, n=n)
        tx = torch.tensor([float(c.T[0]) for c in cams])
        assert len(cams) == n and all(torch.equal(c.R, ident.R) for c in cams)
        assert abs(float(tx.sum())) < 1e-6 and torch.allclose(tx[1:] - tx[:-1], torch.full((n - 1,), 0.015), atol=1e-6)
        assert float(tx.abs().max()) <= 0.015 * 3.5 + 1e-6


def _argument_error_table(L):
    """(label, call, return code, olsr_last_error()) of every argument check that several entries share.  Pointers that
    only have to be non-NULL are a made-up address: each call returns before anything could follow it."""
    import ctypes as C
    from online_lang_splatting_amd import _abi
    ARG, CAP = _abi.OLSR_ERR_ARG, _abi.OLSR_ERR_CAPACITY
    X = 0x1000
    nine = [X] * 9                                  # the parameter arrays and both moment buffers
    ok, step0 = _abi.OlsrAdamParams(), _abi.OlsrAdamParams()
    ok.step, step0.step = 1, 0
    gok, gstep0 = _abi.OlsrAdamGroupParams(), _abi.OlsrAdamGroupParams()
    for g in range(7):
        gok.group_step[g] = gstep0.group_step[g] = 1
    gstep0.group_step[3] = 0
    one, hole = (C.c_void_p * 1)(X), (C.c_void_p * 2)(X, None)
    bad_F = "P, M must be >= 0 and F one of 0, 3, 15, 16, 32"
    bad_step = "adam params are required and step must be >= 1"
    no_params = "every parameter array and both moment buffers are required"
    rows = [
        ("adam_step F", lambda: L.olsr_adam_step(10, 16, 7, ok, X, *nine, None), ARG, bad_F),
        ("adam_step step", lambda: L.olsr_adam_step(10, 16, 15, step0, X, *nine, None), ARG, bad_step),
        ("adam_step no params", lambda: L.olsr_adam_step(10, 16, 15, None, X, *nine, None), ARG, bad_step),
        ("adam_step NULL bucket", lambda: L.olsr_adam_step(10, 16, 15, ok, None, *nine, None), ARG,
         "the bucket, " + no_params),
        ("adam_step NULL parameters", lambda: L.olsr_adam_step(10, 16, 15, ok, X, *([None] * 9), None), ARG,
         "the bucket, " + no_params),
        ("adam_step NULL language", lambda: L.olsr_adam_step(10, 0, 15, ok, X, X, None, X, X, X, None, X, X, None), ARG,
         "the bucket, " + no_params),
    ]
    for name, prefix, fn, extra in (
            ("adam_step_sum", "adam_step_sum", L.olsr_adam_step_sum, ()),
            ("adam_step_masked", "adam_step_sum", L.olsr_adam_step_masked, (None,)),
            ("adam_step_groups", "adam_step_groups", L.olsr_adam_step_groups, (None,))):
        groups = fn is L.olsr_adam_step_groups
        p, p0 = (gok, gstep0) if groups else (ok, step0)
        call = lambda P, M, F, par, n, flats, arrays, fn=fn, extra=extra: fn(P, M, F, par, n, flats, *extra, *arrays, None)
        rows += [
            (name + " F", lambda c=call, p=p: c(10, 16, 7, p, 1, one, nine), ARG, bad_F),
            (name + " M", lambda c=call, p=p: c(10, -1, 15, p, 1, one, nine), ARG, bad_F),
            (name + " step", lambda c=call, p0=p0: c(10, 16, 15, p0, 1, one, nine), ARG,
             "adam_step_groups: the step count of every group that steps must be >= 1" if groups else bad_step),
            (name + " no params", lambda c=call: c(10, 16, 15, None, 1, one, nine), ARG,
             "adam group params are required" if groups else bad_step),
            (name + " no buckets", lambda c=call, p=p: c(10, 16, 15, p, 0, one, nine), ARG,
             prefix + ": between 1 and 8 gradient buckets"),
            (name + " nine buckets", lambda c=call, p=p: c(10, 16, 15, p, 9, one, nine), ARG,
             prefix + ": between 1 and 8 gradient buckets"),
            (name + " NULL bucket list", lambda c=call, p=p: c(10, 16, 15, p, 1, None, nine), ARG,
             prefix + ": between 1 and 8 gradient buckets"),
            (name + " NULL bucket", lambda c=call, p=p: c(10, 16, 15, p, 2, hole, nine), ARG,
             prefix + ": a gradient bucket is NULL"),
            (name + " NULL parameters", lambda c=call, p=p: c(10, 16, 15, p, 1, one, [None] * 9), ARG, no_params),
            (name + " NULL shs", lambda c=call, p=p: c(10, 16, 0, p, 1, one, [X, None] + [X] * 7), ARG, no_params),
        ]

    # the sync-free forwards (an empty scene passes the scene check with no array at all)
    s = _abi.OlsrScene()
    s.P, s.width, s.height, s.tile, s.F, s.binning = 0, 64, 48, 15, 15, 0
    lf = _abi.OlsrLossFusion()
    lf.params.width, lf.params.height = 64, 48
    no_state = "state buffers and a non-negative capacity are required"
    tail = [None] * 8
    for name, call in (
            ("forward_async", lambda g, b, cap, i: L.olsr_forward_async(s, g, b, cap, i, *tail, None)),
            ("forward_async_loss", lambda g, b, cap, i: L.olsr_forward_async_loss(s, g, b, cap, i, *tail, lf, None)),
            ("forward_async_loss (no loss)", lambda g, b, cap, i: L.olsr_forward_async_loss(s, g, b, cap, i, *tail, None, None))):
        rows += [
            (name + " NULL geometry", lambda c=call: c(None, X, 16, X), ARG, no_state),
            (name + " NULL binning", lambda c=call: c(X, None, 16, X), ARG, no_state),
            (name + " NULL image", lambda c=call: c(X, X, 16, None), ARG, no_state),
            (name + " capacity", lambda c=call: c(X, X, -1, X), ARG, no_state),
        ]
    wide, tall = _abi.OlsrLossFusion(), _abi.OlsrLossFusion()
    wide.params.width, wide.params.height = 65, 48
    tall.params.width, tall.params.height = 64, 47
    for name, f in (("width", wide), ("height", tall)):
        rows.append(("fused loss " + name, lambda f=f: L.olsr_forward_async_loss(s, X, X, 16, X, *tail, f, None), ARG,
                     "fused loss: params.width / height must equal the scene's"))

    # the stand-alone losses
    lp, lp0 = _abi.OlsrLossParams(), _abi.OlsrLossParams()
    lp.width, lp.height, lp.F = 64, 48, 15
    lp0.width, lp0.height, lp0.F = 64, 48, 0
    m_need = "image, depth, their targets, their gradient outputs, loss and scratch are required"
    t_need = "image, depth, opacity, their targets, the gradient outputs, loss and scratch are required"

    def mapping(p, **null):
        a = dict(image=X, depth=X, language=X, gt_image=X, gt_depth=X, gt_language=None, exposure=None, dL_dimage=X,
                 dL_ddepth=X, dL_dlanguage=X, loss=X, dL_dexposure=None, scratch=X)
        a.update(null)
        return L.olsr_mapping_loss(p, *a.values(), None)

    def tracking(p, **null):
        a = dict(image=X, depth=X, opacity=X, gt_image=X, gt_depth=X, grad_mask=None, exposure=None, dL_dimage=X,
                 dL_ddepth=X, loss=X, dL_dexposure=None, scratch=X)
        a.update(null)
        return L.olsr_tracking_loss(p, *a.values(), None)

    rows += [("mapping_loss no params", lambda: mapping(None), ARG, "loss params are NULL"),
             ("tracking_loss no params", lambda: tracking(None), ARG, "loss params are NULL")]
    for k in ("image", "depth", "gt_image", "gt_depth", "dL_dimage", "dL_ddepth", "loss", "scratch"):
        rows.append(("mapping_loss NULL " + k, lambda k=k: mapping(lp0, **{k: None}), ARG, m_need))
    for k in ("language", "dL_dlanguage"):
        rows.append(("mapping_loss NULL " + k, lambda k=k: mapping(lp, **{k: None}), ARG,
                     "language and dL_dlanguage are required when F > 0"))
    for k in ("image", "depth", "opacity", "gt_image", "gt_depth", "dL_dimage", "dL_ddepth", "loss", "scratch"):
        rows.append(("tracking_loss NULL " + k, lambda k=k: tracking(lp0, **{k: None}), ARG, t_need))
    for i, k in enumerate(("image", "gt_image", "dL_dimage", "loss", "scratch")):
        if k == "dL_dimage":
            continue                                # (optional: values only)
        a = [X] * 5
        a[i] = None
        rows.append(("refinement_loss NULL " + k, lambda a=a: L.olsr_refinement_loss(64, 48, 0.2, *a, None), ARG,
                     "image, gt_image, loss and scratch are required"))
    rows.append(("refinement_loss size", lambda: L.olsr_refinement_loss(0, 48, 0.2, X, X, X, X, X, None), ARG,
                 "image size must be positive"))

    # map edits
    def params(mode, n_append=0):
        p = _abi.OlsrMapEditParams()
        p.mode, p.n_append = mode, n_append
        return p

    def buffers(**null):
        b = _abi.OlsrMapBuffers()
        for f, _ in _abi.OlsrMapBuffers._fields_:
            setattr(b, f, None if f in null else X)
        return b
    full, empty = buffers(), _abi.OlsrMapBuffers()
    dens, mask = params(_abi.MAP_EDIT_DENSIFY), params(_abi.MAP_EDIT_MASK)
    plan_need = "map_edit_plan: P >= 0, params, src, scratch and status are required"
    apply_need = "map_edit_apply: P, M >= 0, F one of 0, 3, 15, 16, 32; params, scratch and status are required"
    plan, apply = L.olsr_map_edit_plan, L.olsr_map_edit_apply
    rows += [
        ("map_edit_plan P", lambda: plan(-1, mask, full, None, X, X, None), ARG, plan_need),
        ("map_edit_plan no params", lambda: plan(10, None, full, None, X, X, None), ARG, plan_need),
        ("map_edit_plan no src", lambda: plan(10, mask, None, None, X, X, None), ARG, plan_need),
        ("map_edit_plan no scratch", lambda: plan(10, mask, full, None, None, X, None), ARG, plan_need),
        ("map_edit_plan no status", lambda: plan(10, mask, full, None, X, None, None), ARG, plan_need),
        ("map_edit_plan mode", lambda: plan(10, params(2), full, None, X, X, None), ARG, "map_edit_plan: unknown mode"),
        ("map_edit_plan n_append", lambda: plan(10, params(1, -1), full, None, X, X, None), ARG,
         "map_edit_plan: n_append must be >= 0"),
        ("map_edit_plan densify appends", lambda: plan(10, params(0, 3), full, None, X, X, None), ARG,
         "map_edit_plan: densify mode appends nothing"),
        ("map_edit_plan densify stats", lambda: plan(10, dens, buffers(stats=1), None, X, X, None), ARG,
         "map_edit_plan: densify mode reads stats, scales and opacities"),
        ("map_edit_apply F", lambda: apply(10, 16, 7, mask, full, None, None, X, X, 10, 16, full, X, None), ARG, apply_need),
        ("map_edit_apply no status", lambda: apply(10, 16, 15, mask, full, None, None, X, None, 10, 16, full, X, None), ARG,
         apply_need),
        ("map_edit_apply capacity", lambda: apply(10, 16, 15, mask, full, None, None, X, X, 17, 16, full, X, None), CAP,
         "map_edit_apply: P_new exceeds the destination's capacity"),
        ("map_edit_apply dst", lambda: apply(10, 16, 15, mask, full, None, None, X, X, 10, 16, buffers(n_obs=1), X, None), ARG,
         "map_edit_apply: every destination buffer is required"),
        ("map_edit_apply no dst", lambda: apply(10, 16, 15, mask, full, None, None, X, X, 10, 16, None, X, None), ARG,
         "map_edit_apply: every destination buffer is required"),
        ("map_edit_apply src_index", lambda: apply(10, 16, 15, mask, full, None, None, X, X, 10, 16, full, None, None), ARG,
         "map_edit_apply: every destination buffer is required"),
        ("map_edit_apply src", lambda: apply(10, 16, 15, mask, empty, None, None, X, X, 10, 16, full, X, None), ARG,
         "map_edit_apply: every source buffer is required"),
        ("map_edit_apply z", lambda: apply(10, 16, 15, dens, full, None, None, X, X, 10, 16, full, X, None), ARG,
         "map_edit_apply: densify mode needs z [P,2,3]"),
        ("map_edit_apply append", lambda: apply(10, 16, 15, params(1, 2), full, None, buffers(shs=1), X, X, 12, 16, full, X, None),
         ARG, "map_edit_apply: the appended rows need means3D, shs, opacities, scales and rotations"),
        ("map_edit_apply no append", lambda: apply(10, 16, 15, params(1, 2), full, None, None, X, X, 12, 16, full, X, None),
         ARG, "map_edit_apply: the appended rows need means3D, shs, opacities, scales and rotations"),
    ]
    return rows


def test_shared_argument_checks_keep_their_codes_and_messages(L):
    """The argument checks that several C-ABI entries share — the four Adam entries, the sync-free forwards' state buffers and
    capacity, the fused loss's size, the stand-alone losses' pointers, the map edits — return the code and leave the
    olsr_last_error() text listed here, whichever entry they are reached through.  Every one of them returns before the
    first HIP call, so no GPU is involved."""
    rows = _argument_error_table(L)
    assert len(rows) >= 90
    wrong = []
    for label, call, code, message in rows:
        rc = call()
        got = L.olsr_last_error().decode()
        if rc != code or got != message:
            wrong.append((label, rc, got))
    assert not wrong, wrong
