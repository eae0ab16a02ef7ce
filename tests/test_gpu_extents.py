"""No entry of include/olsr.h stores outside the bytes it asked for, reads a word before it is written, or needs a base that is
256-byte aligned where its carve rounds the base up (tests/extent_harness.py has the mechanics).

Every case runs its entry through lib() three ways:
  plain      outputs, scratch and state in ordinary tensors; the result is held to the entry's existing yardstick under the
             assertion its own test file makes (the helper or constant is imported, never restated);
  guarded    every output, scratch and state buffer a guarded view of exactly the bytes the entry asks for, outputs pre-filled
             with a pattern no kernel writes, state and scratch pre-filled with 0xA5, the carve log on: guards intact, the gaps
             Carver::take aligns over intact, every word of every output written, the same bits as the plain run (so nothing
             depended on what the buffers held before);
  misaligned one shape per entry again with every scratch and state buffer 4 bytes past a 256-byte boundary: the same bits.

Shapes straddle the kernels' block quanta; each row of the table names the quantum its shapes are taken from.

| entry | shapes | quanta (source) | scratch |
|---|---|---|---|
| olsr_forward + olsr_backward | P 1..8193 on 45x30; 157x101, 15x15, 16x16 at P 257; F 0/3/15/16/32 at P 1025; all culled; screen-filling x 300; every one with both binnings, both tiles and both modes | preprocess 256 Gaussians / block (part_* sums), one-launch depth sort <= 8192, EMIT_CHUNK 1024, tau_partials 128, wave 64 | three state buffers: Carver (log); row scratch: by hand in olsr_api.hip (outer guards only), served by the callback, and caller-provided with exactly olsr_backward_scratch_bytes(rows) for rows = olsr_live_rows and for the 2 / 4 rows per instance bound |
| olsr_forward + olsr_backward, non-finite rows | the mixture scene of tests/nonfinite_scenes.py at P 257: 45x30 with 15 language channels (tile 15), 64x48 with none (tile 16); both binnings and modes, misaligned as well | as above; radii 0, 2^20 - 1, 2^20 and 2^31 - 1, NaN and infinite means, depths and conics | as above |
| forced sort paths | P 1025, both tiles and modes | legacy passes, kpt 2/4/8/12/16 x 256/1024 threads, one-launch sort off, compaction off | as above |
| olsr_forward_async | binning sized for R, R + 1, R - 1 (overflow) | carve by capacity | state: Carver |
| olsr_debug_backward_ordered | P 257 | one row per instance | Carver (rows, then the flag bytes) |
| olsr_knn_mean_dist2 | P 1, 2, 3, 4, 63, 64, 65, 4095, 4096, 4097 | KNN_BOX 64, superbox 64 boxes = 4096, SORT_CHUNK 4096 | Carver |
| olsr_mark_visible | P 1, 255, 257 | 256 threads | none |
| olsr_mask_smooth, olsr_query_eval | 64x64, 65x63, 70x75 | QE_TILE 64 | Carver |
| olsr_image_psnr | n 1, 3, 4, 5, 1024 * 1024 + 1 | 4 elements / thread, 256 threads, 1024 blocks (grid-stride beyond) | Carver |
| olsr_accumulate_gradients, olsr_bucket_add, olsr_isotropic_reg | P 1, 63, 64, 65, 129; M 1, 16; F 0, 15, 32 | 64 rows / wave, 256 / block (ISO_T 256) | isotropic_reg: Carver (one double per block) |
| olsr_sparse_exchange_mask / _pack / _unpack | P 1, 1023, 1024, 1025; capacity = rows, rows - 1 | 1024 rows per scan block (scratch ints) | int32[ceil(P / 1024)] from the caller |
| olsr_adam_step, _sum, _masked, _groups, _groups_reg | P 1, 63, 64, 65, 129; M 1, 16; F 0, 15, 32 | 64 rows per mask word, 256 per block | none: parameters, moments, buckets and masks between guards |
| olsr_grad_mask | global: 65x63, 64x64, 17x241 (4095, 4096, 4097 pixels); blocks: 65x63, 64x64, 33x65 | FE_CHUNK 4096, 256 threads, 32 x 32 image blocks | Carver (global mode; the block mode takes none) |
| olsr_median_depth | N 1, 4095, 4096, 4097; a mask and none | FE_CHUNK 4096 | as above |
| olsr_covisibility, olsr_keyframe_decide | P 1, 2047, 2048, 2049; K 0, 1, 16 | 8 Gaussians per thread, 2048 per block | none |
| olsr_mapping_loss, olsr_tracking_loss | 45x30 (a width that is no multiple of 4), 157x101; F 0, 15; a mask and none | four pixels per load, blocks of 256 | Carver (per-block partials) |
| olsr_refinement_loss | 45x30, 157x101 | 32 x 16 tiles | Carver (partials; the three [3,H,W] planes as one array) |
| olsr_emd_cost, olsr_chamfer | B 1 and 3 with one empty segment; 255 / 257 / 65 / 63 points | CM_TILE 256 | Carver |
| olsr_debug_activate | P 1, 255, 256, 257 | 256 threads | none |
| olsr_pose_step, _gated, olsr_window_pose_step | V 1, 3 | one wave per view, an 80-float state and 2 status words each | none |
| olsr_forward_async_loss | 45x30 (tile 15), 157x101 (tile 16); mapping with 15 language channels, tracking with a mask | the composite's tiles; a width that is no multiple of 4 | state: Carver; the loss's per-tile partials: Carver |
| olsr_lang_ae_train_step / _encode / _decode | N 1, 255, 256, 257; codes as rows and as channels | 256 rows per block, one partial gradient per block | Carver (train step; encode and decode take none) |
| olsr_lang_query_sims / _relevancy | 24x40, 33x31 | 64 pixels per tile of stage A (960 = 15 tiles, 1023 = 16 less one) | Carver (relevancy; sims takes none) |
| olsr_lang_encoder_encode | N 1, 63, 64, 65; both code layouts | 64 rows per block | none |
| olsr_hr_net_forward | its golden sizes, 2x3 and 3x5 coarse pixels | no multiple of any tile | workspace by hand, 16-byte aligned by contract: no misaligned run |
| olsr_tsdf_init / _integrate / _surface_* / _mesh_* | 8x8x8, 9x7x5; vertex and face capacity = the planned count, and one less | 256 voxels per block (512 = two blocks, 315 = one and a ragged one) | Carver (surface and mesh; init and integrate take none) |
| olsr_map_edit_plan / _apply | P 1, 255, 256, 257; the destination holds exactly P_new rows | 256 source rows per block | Carver |
| olsr_keyframe_seed_plan / _finish | 40x24, the smallest golden image; the staging holds exactly (W H) / downsample rows | - | Carver; the kNN scratch: Carver |

Floating-point atomics: none of the entries above accumulates with them (the backward sums rows in a fixed order, the losses
and metrics add per-block partials in block order), so every row compares the guarded runs with the plain run by bits.

NO_ROW at the end of the file lists every other entry of include/olsr.h with the reason it has none: it is a sizing function
(tests/test_extents_cpu.py), or it writes no device memory of the caller's."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import extent_harness as H
from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.scene import make_scene
from parity_common import assert_elementwise, assert_tau_sum_fixed_order, fwd_args, rel_err, run_backend

pytestmark = pytest.mark.gpu
DEV = H.DEV
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
VP = C.c_void_p


def _L():
    from online_lang_splatting_amd._lib import lib
    return lib()


def _check_rc(rc):
    from online_lang_splatting_amd._lib import check
    check(rc)


def _stream():
    return VP(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _p(t):
    return t.data_ptr() if t is not None and t.numel() > 0 else None


class Case:
    """One run of an entry: `new` makes its outputs (guarded and pre-filled, or plain), `scratch` its scratch buffers."""

    def __init__(self, guard, misalign=0):
        self.guard, self.misalign = guard, misalign
        self.buffers, self.written, self.out = [], [], {}

    def new(self, name, shape, dtype, written=True):
        if self.guard:
            t = H.guarded_tensor(shape, dtype)
            if t.numel():
                self.buffers.append(t)
                if written:
                    self.written.append(t)
        else:
            t = torch.empty(shape, dtype=dtype, device=DEV)
        self.out[name] = t
        return t

    def scratch(self, nbytes, misalign_ok=True):
        if not self.guard:
            return torch.empty(int(nbytes), dtype=U8, device=DEV)
        t = H.guarded(nbytes, self.misalign if misalign_ok else 0)
        self.buffers.append(t)
        return t

    def inout(self, name, value):
        """An array the entry updates in place: a guarded (or plain) copy of `value`."""
        t = self.new(name, value.shape, value.dtype, written=False)
        t.copy_(value)
        return t


def three_ways(entry, misaligned=True):
    """entry(case) runs the entry and fills case.out.  Returns the plain run's outputs after the guarded (and misaligned) runs
    passed check() and gave the same bits."""
    L = _L()
    plain = Case(False)
    entry(plain)
    torch.cuda.synchronize()
    for misalign in (0, 4) if misaligned else (0,):
        H.reset()
        case = Case(True, misalign)
        H.log_on()
        try:
            entry(case)
            torch.cuda.synchronize()
        finally:
            log = H.log_off()
        H.check(case.buffers, log, case.written)
        assert case.out.keys() == plain.out.keys()
        for k, t in plain.out.items():
            assert H.same_bits(case.out[k], t), f"{k}: the guarded run (base + {misalign}) differs from the plain run"
    H.reset()
    return plain.out


@pytest.fixture(autouse=True)
def _carve_log_off():
    yield
    _L().olsr_debug_carve_log(0)
    H.reset()


# ------------------------------------------------------------------------------------------------ the rasteriser
GRAD_SHAPES = dict(dL_dmeans2D=(3,), dL_dconic=(2, 2), dL_dopacity=(1,), dL_dcolors=(3,), dL_dlanguage=None, dL_ddepths=(1,),
                   dL_dmeans3D=(3,), dL_dcov3D=(6,), dL_dsh=None, dL_dscales=(3,), dL_drotations=(4,), dL_dtau=(6,))
FWD_KEYS = ("color", "language", "depth", "opacity", "radii", "n_touched")


def _scene_struct(sc, tile, mode, binning):
    from online_lang_splatting_amd import _C
    dev = torch.device(DEV)
    F = max(sc.F, 0)
    a = fwd_args(sc, dev)
    off = 1 if F > 0 else 0
    bg, means3D, colors = a[0], a[1], a[2]
    language = a[3] if F > 0 else None
    opacity, scales, rotations, scale_modifier, cov3D = a[3 + off], a[4 + off], a[5 + off], a[6 + off], a[7 + off]
    view, proj, proj_raw, tanx, tany, height, width, sh, degree, campos = a[8 + off:18 + off]
    return _C._scene(F, bg, means3D, colors, language, opacity, scales, rotations, scale_modifier, cov3D, view, proj, proj_raw,
                     tanx, tany, height, width, sh, degree, campos, False, False, cfg=(tile, mode, binning))


def raster(case, sc, tile, mode, binning, seed, scratch_form="callback"):
    """olsr_forward + olsr_backward on `sc`; scratch_form: "callback", "live" (caller-provided, olsr_live_rows rows) or "bound"
    (caller-provided, the 2 / 4 rows per instance bound)."""
    L = _L()
    s, keep = _scene_struct(sc, tile, mode, binning)
    P, F, M, Hh, W = sc.P, max(sc.F, 0), s.M, sc.camera.height, sc.camera.width
    alloc = H.Allocator(_abi.ALLOC_FN, guard=case.guard, misalign=case.misalign)
    color, lang = case.new("color", (3, Hh, W), F32), case.new("language", (F, Hh, W), F32)
    depth, opac = case.new("depth", (1, Hh, W), F32), case.new("opacity", (1, Hh, W), F32)
    radii, n_touched = case.new("radii", (P,), I32), case.new("n_touched", (P,), I32)
    R = C.c_int32(-1)
    _check_rc(L.olsr_forward(C.byref(s), alloc.cb, VP(0), alloc.cb, VP(1), alloc.cb, VP(2), _p(color), _p(lang), _p(depth),
                             _p(opac), _p(radii), _p(n_touched), C.byref(R), _stream()))
    token = L.olsr_last_forward_token()
    geom, binb, img = alloc.of(0)[0], alloc.of(1)[0], alloc.of(2)[0]
    assert geom.numel() == L.olsr_geometry_bytes(P, F) and binb.numel() == L.olsr_binning_bytes(R.value, F)
    assert img.numel() == L.olsr_image_bytes(W, Hh, tile)
    case.R = R.value
    dc, dl, dd = [None if t is None else t.to(DEV).contiguous() for t in sc.cotangents(seed)]
    g = {}
    for k, tail in GRAD_SHAPES.items():
        tail = ((F,) if k == "dL_dlanguage" else (M, 3)) if tail is None else tail
        g[k] = case.new(k, (P,) + tail, F32)
    g["dL_dtau_sum"] = case.new("dL_dtau_sum", (6,), F32)
    status = case.new("status", (2,), I32)
    packed = 1 if (mode == _abi.BWD_REFERENCE and tile == 15) else 0
    if scratch_form == "callback":
        sa, su, tok, scratch, rows = alloc.cb, VP(3), token, None, 0
    else:
        torch.cuda.synchronize()
        rows = L.olsr_live_rows(token, packed) if scratch_form == "live" else L.olsr_backward_rows(0, packed, R.value, F)
        assert rows >= 0 and (scratch_form == "live" or rows == (2 if packed else 4) * R.value)
        scratch = case.scratch(L.olsr_backward_scratch_bytes(rows, F))
        sa, su, tok = _abi.ALLOC_FN(), None, 0
    _check_rc(L.olsr_backward(C.byref(s), _p(radii), geom.data_ptr(), R.value, binb.data_ptr(), img.data_ptr(), sa, su, tok,
                              _p(scratch), rows, _p(dc), _p(dl), _p(dd),
                              _p(g["dL_dmeans2D"]), _p(g["dL_dconic"]), _p(g["dL_dopacity"]), _p(g["dL_dcolors"]),
                              _p(g["dL_dlanguage"]), _p(g["dL_ddepths"]), _p(g["dL_dmeans3D"]), _p(g["dL_dcov3D"]), _p(g["dL_dsh"]),
                              _p(g["dL_dscales"]), _p(g["dL_drotations"]), _p(g["dL_dtau"]), _p(g["dL_dtau_sum"]), None,
                              _p(status), _stream()))
    torch.cuda.synchronize()
    if case.guard:
        case.buffers += alloc.buffers
    else:
        case.keep = (alloc, keep)
    case.out["R"] = torch.tensor([R.value])


_ORACLE = {}


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    """The oracle's forward + backward of a scene, once per (scene, tile, mode)."""
    def run(key, sc, seed, tile, mode):
        k = (key, seed, tile, mode)
        if k not in _ORACLE:
            _ORACLE[k] = run_backend(oracle, sc, None, seed, tile, mode)
        return _ORACLE[k]
    yield run
    for fo, _ in _ORACLE.values():
        oracle.release(fo["geom"])
    _ORACLE.clear()


def _against_oracle(out, fo, go, binning, name):
    """tests/test_gpu_parity.py's statements about one binning mode (its _check): the forward bit for bit, every gradient to
    its RTOL in the max norm, the composite-level ones also per element."""
    import test_gpu_parity as TP
    composite_worst = inspect.signature(TP._check).parameters["composite_worst_bound"].default
    R = int(out["R"])
    assert R == fo["R"] if binning == _abi.BINNING_RECT else R <= fo["R"], (name, R, fo["R"])
    assert torch.equal(out["radii"].cpu(), fo["radii"]) and torch.equal(out["n_touched"].cpu(), fo["n_touched"]), name
    for k in ("color", "language", "depth", "opacity"):
        if fo[k] is not None and fo[k].numel():
            assert torch.equal(out[k].cpu().reshape(-1), fo[k].reshape(-1)), f"{name}: forward {k} not bit-identical"
    for k in go:
        if go[k].numel() and k in out:
            r, e = rel_err(out[k].reshape(-1), go[k].reshape(-1))
            assert r <= TP.RTOL, f"{name}: {k}: rel {r:.2e} abs {e:.2e}"
            if k in TP.COMPOSITE_GRADS:
                assert_elementwise(out[k].reshape(-1), go[k].reshape(-1), f"{name}:{k}", composite_worst)
    tau_sum = go["dL_dtau"].double().sum(0).float()
    r, _ = rel_err(out["dL_dtau_sum"], tau_sum)
    assert r <= TP.RTOL, f"{name}: dL_dtau_sum: rel {r:.2e}"
    assert_tau_sum_fixed_order(out, where=f"{name}: ")
    assert int(out["status"][1]) == 0, name


def _raster_case(oracle_runs, key, sc, seed, tile, mode, binnings=(_abi.BINNING_RECT, _abi.BINNING_ELLIPSE), forms=("callback",),
                 misaligned=False):
    fo, go = oracle_runs(key, sc, seed, tile, mode)
    outs = {}
    for binning in binnings:
        for form in forms:
            name = f"{key} tile {tile} mode {mode} binning {binning} scratch {form}"
            out = three_ways(lambda c: raster(c, sc, tile, mode, binning, seed, form), misaligned=misaligned)
            _against_oracle(out, fo, go, binning, name)
            outs[(binning, form)] = out
    return outs


MODES = (_abi.BWD_REFERENCE, _abi.BWD_EXACT)
# preprocess sums 256 Gaussians per block (part_rect / part_count / part_vis: ceil(P / 256) + 1 words), the backward's dL_dtau
# reduction 128 (tau_partials), the emission scans EMIT_CHUNK = 1024 depth ranks per block, a wave holds 64, and the one-launch
# depth sort takes up to 8192 Gaussians (k_sort.hip): one below, at and one above each
RASTER_P = (1, 64, 65, 255, 256, 257, 1023, 1024, 1025, 8192, 8193)


@pytest.mark.parametrize("tile", [15, 16])
@pytest.mark.parametrize("P", RASTER_P)
def test_forward_backward_over_the_block_quanta(hip, oracle_runs, P, tile):
    sc = make_scene(P, 45, 30, 15, seed=100 + P)
    for mode in MODES:
        _raster_case(oracle_runs, f"P{P}", sc, 3, tile, mode, misaligned=(P == 257))


@pytest.mark.parametrize("tile", [15, 16])
def test_forward_backward_non_finite_gaussians(hip, oracle, tile):
    """The mixture scene of tests/nonfinite_scenes.py (NaN, infinite, overflowing and saturating rows among ordinary ones) at
    P = 257: a saturated radius or a NaN that escaped a clamp on its way to an index shows here as a changed guard byte or a
    touched carve gap.  The forward is the oracle's by bits (NaN where it has NaN); tests/test_gpu_nonfinite.py holds the rest."""
    import nonfinite_scenes as NF
    from parity_common import same_bits
    p = NF.planted_scene("mix_all", 257, 45 if tile == 15 else 64, 30 if tile == 15 else 48, 15 if tile == 15 else 0, seed=11)
    want = NF.oracle_forward(p.scene, tile)
    assert int((want["radii"][p.idx] == (1 << 31) - 1).sum()) > 0 and int((want["radii"][p.idx] == 0).sum()) > 0
    for mode in MODES:
        for binning in (_abi.BINNING_RECT, _abi.BINNING_ELLIPSE):
            out = three_ways(lambda c: raster(c, p.scene, tile, mode, binning, 3), misaligned=True)
            name = f"tile {tile} mode {mode} binning {binning}"
            assert int(out["R"]) == want["R"] if binning == _abi.BINNING_RECT else int(out["R"]) <= want["R"], name
            assert torch.equal(out["radii"].cpu(), want["radii"]) and torch.equal(out["n_touched"].cpu(), want["n_touched"]), name
            for k in ("color", "language", "depth", "opacity"):
                if want[k] is not None and want[k].numel():
                    assert same_bits(out[k], want[k]), f"{name}: forward {k}"
            assert int(out["status"][1]) == 0, name


@pytest.mark.parametrize("W,Hh,tile", [(157, 101, 15), (157, 101, 16), (15, 15, 15), (16, 16, 16), (16, 16, 15), (15, 15, 16)])
def test_forward_backward_image_sizes(hip, oracle_runs, W, Hh, tile):
    """A ragged image of several tiles each way, and images of exactly one tile (and of one tile and a sliver)."""
    sc = make_scene(257, W, Hh, 15, seed=7 + W)
    for mode in MODES:
        _raster_case(oracle_runs, f"{W}x{Hh}", sc, 4, tile, mode)


@pytest.mark.parametrize("F", [0, 3, 15, 16, 32])
def test_forward_backward_language_widths(hip, oracle_runs, F):
    """gacc and the row scratch are grad_row(F) floats wide."""
    sc = make_scene(1025, 45, 30, F, seed=31 + F)
    for tile in (15, 16):
        for mode in MODES:
            _raster_case(oracle_runs, f"F{F}", sc, 5, tile, mode, misaligned=(tile == 15) == (mode == _abi.BWD_REFERENCE))


def test_forward_backward_all_culled(hip, oracle_runs):
    """R = 0: everything behind the near plane (tests/test_gpu_parity.py: test_empty_culled_and_single)."""
    sc = make_scene(300, 45, 30, 15, seed=1)
    sc.means3D[:, 2] = 0.2
    for tile in (15, 16):
        for mode in MODES:
            outs = _raster_case(oracle_runs, "culled", sc, 1, tile, mode, forms=("callback", "live", "bound"), misaligned=True)
            assert all(int(o["R"]) == 0 and float(o["dL_dmeans3D"].abs().max()) == 0 for o in outs.values())


def test_forward_backward_screen_filling(hip, oracle_runs):
    """tests/test_gpu_parity.py's test_emission_of_screen_filling_splats scaled down to 300 Gaussians: every one covers most
    of the tiles, the emission's row tables refill, a Gaussian straddles several 1024-instance windows."""
    sc = make_scene(300, 160, 120, 3, seed=91, scale_mult=25.0)
    for tile in (15, 16):
        for mode in MODES:
            _raster_case(oracle_runs, "filling", sc, 9, tile, mode)


@pytest.mark.parametrize("form", ["live", "bound"])
@pytest.mark.parametrize("tile,mode", [(15, _abi.BWD_REFERENCE), (15, _abi.BWD_EXACT), (16, _abi.BWD_REFERENCE)])
def test_backward_row_scratch_from_the_caller(hip, oracle_runs, tile, mode, form):
    """scratch_alloc == NULL with exactly olsr_backward_scratch_bytes(rows, F) bytes, rows from olsr_live_rows and from the
    bound (2 rows per instance in the reference mode of 15 x 15 tiles, else 4)."""
    for P in (257, 1025):
        sc = make_scene(P, 45, 30, 15, seed=100 + P)
        outs = _raster_case(oracle_runs, f"P{P}", sc, 3, tile, mode, forms=(form,), misaligned=True)
        assert all(int(o["status"][1]) == 0 and int(o["status"][0]) > 0 for o in outs.values())


def _forced(fn):
    """fn(L) with whatever knobs it forces; afterwards the knobs hold what was in force before: the block shape as read back,
    the others (which have no read-back) as the library seeded them from the environment."""
    from test_extents_cpu import seeded_sort_knobs
    L = _L()
    threads0 = L.olsr_debug_sort_threads(-1)
    kpt0, legacy0, small0, compact0 = seeded_sort_knobs()
    try:
        fn(L)
    finally:
        L.olsr_debug_sort_knobs(kpt0, -1, legacy0)
        L.olsr_debug_sort_threads(threads0)
        L.olsr_debug_sort_small(small0)
        L.olsr_debug_sort_compact(compact0)


SORT_PATHS = ([("legacy", lambda L: L.olsr_debug_sort_knobs(-1, -1, 1)), ("small_off", lambda L: L.olsr_debug_sort_small(0)),
               ("compact_off", lambda L: (L.olsr_debug_sort_small(0), L.olsr_debug_sort_compact(0)))]
              + [(f"kpt{k}_t{t}", (lambda k, t: lambda L: (L.olsr_debug_sort_small(0), L.olsr_debug_sort_knobs(k, -1, -1),
                                                          L.olsr_debug_sort_threads(t)))(k, t))
                 for k in (2, 4, 8, 12, 16) for t in (256, 1024)])


@pytest.mark.parametrize("path", SORT_PATHS, ids=[p[0] for p in SORT_PATHS])
def test_forced_sort_paths(hip, oracle_runs, path):
    """Every radix path on one scene: the multi-kernel passes (radix_table, scan_partials), every keys-per-thread with both
    block shapes (the status rows), the radix passes where the one-launch sort would run, and the depth sort over every
    Gaussian instead of the emitting ones.  (A forced kpt acts on the depth sort only with the one-launch sort off.)"""
    sc = make_scene(1025, 45, 30, 15, seed=100 + 1025)

    def run(L):
        path[1](L)
        for tile in (15, 16):
            for mode in MODES:
                _raster_case(oracle_runs, "P1025", sc, 3, tile, mode)
    _forced(run)


def test_forward_async_capacity(hip, oracle_runs):
    """olsr_forward_async carves the binning buffer by the caller's capacity: R exactly, R + 1, and R - 1, which must report
    the overflow (status 1) and still store nowhere outside the buffers."""
    L = _L()
    sc = make_scene(1025, 45, 30, 15, seed=100 + 1025)
    tile, mode, binning = 15, _abi.BWD_REFERENCE, _abi.BINNING_ELLIPSE
    fo, go = oracle_runs("P1025", sc, 3, tile, mode)
    first = Case(False)
    raster(first, sc, tile, mode, binning, 3)
    R = int(first.out["R"])
    assert R > 1
    s, keep = _scene_struct(sc, tile, mode, binning)
    P, F, Hh, W = sc.P, sc.F, sc.camera.height, sc.camera.width

    def entry(capacity, overflow):
        def run(case):
            geom, img = case.scratch(L.olsr_geometry_bytes(P, F)), case.scratch(L.olsr_image_bytes(W, Hh, tile))
            binb = case.scratch(L.olsr_binning_bytes(capacity, F))
            w = not overflow   # (nothing is rendered on overflow: the images are not promised then)
            o = [case.new(k, shape, dt, written=w) for k, shape, dt in (
                ("color", (3, Hh, W), F32), ("language", (F, Hh, W), F32), ("depth", (1, Hh, W), F32), ("opacity", (1, Hh, W), F32),
                ("radii", (P,), I32), ("n_touched", (P,), I32))]
            nr = case.new("num_rendered", (2,), I32)
            _check_rc(L.olsr_forward_async(C.byref(s), geom.data_ptr(), binb.data_ptr(), capacity, img.data_ptr(), *[_p(t) for t in o],
                                           _p(nr), None, _stream()))
            torch.cuda.synchronize()
            if overflow:   # only the count and the status are promised
                case.out = dict(num_rendered=nr)
        return run

    for capacity in (R, R + 1):
        out = three_ways(entry(capacity, False))
        assert out["num_rendered"].tolist() == [R, 0]
        for k in FWD_KEYS:
            assert H.same_bits(out[k], first.out[k]), (capacity, k)
    out = three_ways(entry(R - 1, True))
    assert out["num_rendered"].tolist() == [R, 1]


def test_debug_backward_ordered_scratch(hip, oracle_runs):
    """The ordered composite backward's scratch (one row and one flag byte per instance), on the state of a plain forward;
    its yardstick is the oracle, bit for bit (parity_common.assert_ordered_equals_oracle)."""
    from parity_common import COMPOSITE_KEYS, assert_ordered_equals_oracle
    L = _L()
    P, tile, mode, binning = 257, 15, _abi.BWD_REFERENCE, _abi.BINNING_RECT
    sc = make_scene(P, 45, 30, 15, seed=100 + P)
    fo, go = oracle_runs(f"P{P}", sc, 3, tile, mode)
    first = Case(False)
    raster(first, sc, tile, mode, binning, 3)
    alloc, _ = first.keep
    geom, binb, img = alloc.of(0)[0], alloc.of(1)[0], alloc.of(2)[0]
    R, F = int(first.out["R"]), sc.F
    s, keep = _scene_struct(sc, tile, mode, binning)
    dc, dl, dd = [t.to(DEV).contiguous() for t in sc.cotangents(3)]

    def entry(case):
        scratch = case.scratch(L.olsr_debug_backward_ordered_scratch_bytes(R, F))
        g = {k: case.new(k, (P,) + (GRAD_SHAPES[k] or (F,)), F32) for k in COMPOSITE_KEYS}
        _check_rc(L.olsr_debug_backward_ordered(C.byref(s), geom.data_ptr(), R, binb.data_ptr(), img.data_ptr(), _p(dc), _p(dl), _p(dd),
                                                scratch.data_ptr(), *[_p(g[k]) for k in COMPOSITE_KEYS], 0, _stream()))
    out = three_ways(entry)
    assert_ordered_equals_oracle(go, out)


# ------------------------------------------------------------------------------------------------ kNN, visibility
# KNN_BOX = 64 points per box (`sorted` is padded to whole boxes), 64 boxes per superbox = 4096 points, SORT_CHUNK = 4096 keys
# per block of the radix passes (k_knn.hip, olsr_state.h)
@pytest.mark.parametrize("P", [1, 2, 3, 4, 63, 64, 65, 4095, 4096, 4097])
def test_knn_mean_dist2(hip, oracle, P):
    from test_gpu_knn import _cloud
    L = _L()
    pts = _cloud(P, P, "clusters" if P == 65 else "uniform")
    dev_pts = pts.to(DEV).contiguous()

    def entry(case):
        out = case.new("mean_dist2", (P,), F32)
        scratch = case.scratch(L.olsr_knn_scratch_bytes(P))
        _check_rc(L.olsr_knn_mean_dist2(P, dev_pts.data_ptr(), out.data_ptr(), scratch.data_ptr(), _stream()))
    out = three_ways(entry, misaligned=P in (65, 4097))
    assert torch.equal(out["mean_dist2"].cpu(), oracle.distCUDA2(pts))   # (tests/test_gpu_knn.py: bit for bit)


@pytest.mark.parametrize("P", [1, 255, 257])   # 256 Gaussians per block
def test_mark_visible(hip, oracle, P):
    L = _L()
    sc = make_scene(P, 45, 30, 0, seed=11 + P)
    cam = sc.camera
    m, v, pr = [t.to(DEV).contiguous() for t in (sc.means3D, cam.world_view_transform, cam.full_proj_transform)]

    def entry(case):
        present = case.new("present", (P,), torch.bool)
        _check_rc(L.olsr_mark_visible(P, m.data_ptr(), v.data_ptr(), pr.data_ptr(), present.data_ptr(), _stream()))
    out = three_ways(entry, misaligned=False)
    assert torch.equal(out["present"].cpu(), oracle.mark_visible(sc.means3D, cam.world_view_transform, cam.full_proj_transform))


# ------------------------------------------------------------------------------------------------ query scoring
# QE_TILE = 64 pixels each way (k_query_eval.hip): exactly one tile, one above and one below, and two tiles each way with
# neither extent a multiple of the tile or of 4
@pytest.mark.parametrize("Hh,W", [(64, 64), (65, 63), (70, 75)])
def test_mask_smooth_and_query_eval(hip, Hh, W):
    import query_eval_ref as R
    L = _L()
    rng = np.random.default_rng(Hh * 100 + W)
    P = 3
    mask = (rng.random((P, Hh, W)) < 0.5).astype(np.uint8)
    gt = (rng.random((P, Hh, W)) < 0.4).astype(np.uint8)
    sm = rng.random((P, Hh, W)).astype(np.float32)
    sm[0, Hh - 1, W - 1] = 2.0   # a maximum in the last pixel of the last tile
    sm[1, 0, 0] = sm[1, Hh // 2, W - 1] = 2.0
    boxes = np.float32([[W - 3, Hh - 3, W - 1, Hh - 1], [5, 5, 6, 6], [0, 0, W, Hh]])
    off = np.int32([0, 1, 2, 3])
    want = R.score_image(mask, sm, gt, boxes, off)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in dict(mask=mask, gt=gt, sm=sm, boxes=boxes, off=off).items()}
    score = d["sm"].reshape(P, -1).max(dim=1).values.contiguous()

    def smooth(case):
        out = case.new("smoothed", (P, Hh, W), U8)
        _check_rc(L.olsr_mask_smooth(P, Hh, W, d["mask"].data_ptr(), out.data_ptr(), _stream()))
    out = three_ways(smooth, misaligned=False)
    assert np.array_equal(out["smoothed"].cpu().numpy(), np.stack([R.smooth(m) for m in mask]))

    def evaluate(case):
        res, ms = case.new("result", (P, 4), I32), case.new("mask_smoothed", (P, Hh, W), U8)
        scratch = case.scratch(L.olsr_query_eval_scratch_bytes(P, Hh, W))
        _check_rc(L.olsr_query_eval(P, Hh, W, d["mask"].data_ptr(), d["sm"].data_ptr(), score.data_ptr(), d["gt"].data_ptr(),
                                    d["boxes"].data_ptr(), d["off"].data_ptr(), res.data_ptr(), ms.data_ptr(), scratch.data_ptr(),
                                    _stream()))
    out = three_ways(evaluate)
    assert out["result"].cpu().numpy().tolist() == np.stack([want[k] for k in ("intersection", "union", "n_max", "hit")], 1).tolist()
    assert np.array_equal(out["mask_smoothed"].cpu().numpy(), want["mask_smoothed"])


# a thread takes 4 elements (one 16-byte load), a block 256 threads, the grid at most 1024 blocks = 1024 * 1024 elements in one
# sweep: the last size takes the grid-stride loop for its one element
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1024 * 1024 + 1])
def test_image_psnr(hip, n):
    import query_eval_ref as R
    L = _L()
    rng = np.random.default_rng(n)
    gt = rng.random(n).astype(np.float32)
    gt[rng.random(n) < 0.2] = 0.0
    gt[-1] = 0.5
    image = (gt + rng.normal(0.0, 0.15, n)).astype(np.float32)
    a, g = torch.from_numpy(image).to(DEV), torch.from_numpy(gt).to(DEV)

    def entry(case):
        out = case.new("out", (2,), torch.float64)
        scratch = case.scratch(L.olsr_image_psnr_scratch_bytes())
        _check_rc(L.olsr_image_psnr(1, 1, n, a.data_ptr(), g.data_ptr(), out.data_ptr(), scratch.data_ptr(), _stream()))
    s, cnt = three_ways(entry)["out"].tolist()
    keep = gt > 0
    d = np.clip(image[keep], np.float32(0), np.float32(1)).astype(np.float64) - gt[keep].astype(np.float64)
    want = float((d * d).sum())
    assert cnt == int(keep.sum()) and abs(s - want) <= R.PSNR_FLOOR * want   # (test_gpu_query_eval.py's floor on the mse)


# ------------------------------------------------------------------------------------------------ bucket, optimiser
# One thread per row, 64 rows per wave (a mask word), 256 per block (k_accumulate.hip, k_adam.hip: ISO_T = 256): P below, at and
# above a wave, and above a multiple of it with a partial last word.  The element index of accumulate / bucket_add comes from
# an fp32 division by the row width: widths 14 (M 1, F 0) to 91 (M 16, F 32).
BUCKET_P = (1, 63, 64, 65, 129)
BUCKET_MF = [(M, F) for M in (1, 16) for F in (0, 15, 32)]


def _bucket_inputs(P, M, F, seed):
    g = torch.Generator().manual_seed(seed)
    grads = dict(dL_dmeans3D=torch.randn(P, 3, generator=g), dL_dsh=torch.randn(P, M, 3, generator=g),
                 dL_dopacity=torch.randn(P, 1, generator=g), dL_dscales=torch.randn(P, 3, generator=g),
                 dL_drotations=torch.randn(P, 4, generator=g), dL_dlanguage=torch.randn(P, F, generator=g),
                 dL_dmeans2D=torch.randn(P, 3, generator=g))
    radii = torch.randint(0, 5, (P,), generator=g, dtype=torch.int32)
    return grads, radii


@pytest.mark.parametrize("assign", [1, 0])
@pytest.mark.parametrize("P", BUCKET_P)
def test_accumulate_gradients(hip, P, assign):
    """Yardstick: GradientBucket's torch formulation on CPU tensors, to the tolerance of
    tests/test_gpu_api.py::test_fused_accumulate_matches_torch_formulation (rtol = atol = 1e-6; max_radii exact)."""
    from online_lang_splatting_amd.frame_shard import GradLayout, GradientBucket
    from test_gpu_api import ACCUMULATE_TOL
    L = _L()
    for M, F in BUCKET_MF:
        lay = GradLayout(M, F)
        grads, radii = _bucket_inputs(P, M, F, 3 + P)
        g0 = torch.Generator().manual_seed(17)
        init = (torch.randn(P, lay.width, generator=g0), torch.rand(P, 2, generator=g0),
                torch.randint(0, 5, (P,), generator=g0, dtype=torch.int32))
        ref = GradientBucket(P, lay, "cpu")
        if not assign:
            ref.flat.copy_(init[0]), ref.densify.copy_(init[1]), ref.max_radii.copy_(init[2])
        ref.accumulate(grads, radii, first=bool(assign))
        d = {k: v.to(DEV).contiguous() for k, v in grads.items()}
        rad = radii.to(DEV)

        def entry(case):
            if assign:   # overwritten: every word must be written
                flat, den, mr = case.new("flat", (P, lay.width), F32), case.new("densify", (P, 2), F32), case.new("max_radii", (P,), I32)
            else:
                flat, den, mr = [case.inout(k, v.to(DEV)) for k, v in zip(("flat", "densify", "max_radii"), init)]
            _check_rc(L.olsr_accumulate_gradients(P, M, F, assign, _p(d["dL_dmeans3D"]), _p(d["dL_dsh"]), _p(d["dL_dopacity"]),
                                                  _p(d["dL_dscales"]), _p(d["dL_drotations"]), _p(d["dL_dlanguage"]), _p(d["dL_dmeans2D"]),
                                                  rad.data_ptr(), flat.data_ptr(), den.data_ptr(), mr.data_ptr(), _stream()))
        out = three_ways(entry, misaligned=False)
        torch.testing.assert_close(out["flat"].cpu(), ref.flat, rtol=ACCUMULATE_TOL, atol=ACCUMULATE_TOL)
        torch.testing.assert_close(out["densify"].cpu(), ref.densify, rtol=ACCUMULATE_TOL, atol=ACCUMULATE_TOL)
        assert torch.equal(out["max_radii"].cpu(), ref.max_radii)


def _mask_words(bits):
    P = bits.numel()
    pad = torch.zeros((P + 63) // 64 * 64, dtype=torch.int64)
    pad[:P] = bits
    w = pad.view(-1, 64)
    mask = torch.zeros(w.shape[0], dtype=torch.int64)
    for b in range(64):
        mask |= w[:, b] << b
    return mask


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("P", BUCKET_P)
def test_bucket_add(hip, P, masked):
    """Yardstick: torch's dense add and maximum, bit for bit (tests/test_gpu_row_mask.py: "the lane sum")."""
    L = _L()
    for M, F in BUCKET_MF:
        width = 11 + 3 * M + F
        g = torch.Generator().manual_seed(5 + P)
        dst = (torch.randn(P, width, generator=g), torch.rand(P, 2, generator=g), torch.randint(0, 9, (P,), generator=g, dtype=torch.int32))
        src = (torch.randn(P, width, generator=g), torch.rand(P, 2, generator=g), torch.randint(0, 9, (P,), generator=g, dtype=torch.int32))
        src_bits = torch.rand(P, generator=g) < 0.5
        dst_bits = torch.rand(P, generator=g) < 0.5
        if masked:   # the mask's invariant: a row whose bit is clear holds +0.0
            src[0][~src_bits] = 0.0
            dst[0][~dst_bits] = 0.0
        want = (dst[0] + src[0], dst[1] + src[1], torch.maximum(dst[2], src[2]))
        s_dev = [t.to(DEV) for t in src]
        sm = _mask_words(src_bits).to(DEV) if masked else None

        def entry(case):
            flat, den, mr = [case.inout(k, v.to(DEV)) for k, v in zip(("flat", "densify", "max_radii"), dst)]
            dm = case.inout("row_mask", _mask_words(dst_bits).to(DEV)) if masked else None
            _check_rc(L.olsr_bucket_add(P, width, flat.data_ptr(), den.data_ptr(), mr.data_ptr(), _p(dm), s_dev[0].data_ptr(),
                                        s_dev[1].data_ptr(), s_dev[2].data_ptr(), _p(sm), _stream()))
        out = three_ways(entry, misaligned=False)
        assert torch.equal(out["flat"].cpu(), want[0]) and torch.equal(out["densify"].cpu(), want[1])
        assert torch.equal(out["max_radii"].cpu(), want[2])
        if masked:
            assert torch.equal(out["row_mask"].cpu(), _mask_words(src_bits | dst_bits))


@pytest.mark.parametrize("P", BUCKET_P + (255, 256, 257))
def test_isotropic_reg(hip, P):
    """Yardstick: tests/window_ba_ref.py — the gradient bit for bit, the loss within 6 x 2^-24 x weight x max s of the float64
    statement (tests/test_gpu_mapping_ba.py::test_isotropic_reg).  The scratch is carved: one double per block of 256 rows."""
    import window_ba_ref as ref
    from test_gpu_adam import A
    from test_gpu_mapping_ba import ISO_LOSS_BOUND
    L = _L()
    rng = np.random.default_rng(P)
    s = np.exp(rng.standard_normal((P, 3)) * 0.7 - 4.0).astype(np.float32)
    weight = 10.0
    x = torch.from_numpy(s).to(DEV)

    def entry(case):
        grad, loss = case.new("grad", (P, 3), F32), case.new("loss", (1,), torch.float64)
        scratch = case.scratch(L.olsr_isotropic_reg_scratch_bytes(P))
        _check_rc(L.olsr_isotropic_reg(P, x.data_ptr(), 0, weight, grad.data_ptr(), loss.data_ptr(), scratch.data_ptr(), _stream()))
    out = three_ways(entry)
    want, _ = ref.isotropic_rows(s, False, weight)
    assert A.same_bits(out["grad"].cpu().numpy(), want).all()
    assert abs(float(out["loss"]) - float(ref.isotropic_loss(s, False, weight))) <= ISO_LOSS_BOUND * weight * s.max()


ADAM_ENTRIES = ("step", "sum", "masked", "groups", "groups_reg")


@pytest.mark.parametrize("entry_name", ADAM_ENTRIES)
@pytest.mark.parametrize("P", BUCKET_P)
def test_adam_steps(hip, P, entry_name):
    """The five olsr_adam_step* entries on the first step of tests/adam_ref.py's shape cases at these shapes; yardstick: its
    restatement, bit for bit (tests/test_gpu_adam.py).  groups_reg: the restatement fed one extra bucket that holds the
    regulariser's rows (tests/window_ba_ref.py) in its scale columns, as include/olsr.h defines the entry.  Parameters, both
    moments, the buckets and the row masks all sit between guards."""
    import window_ba_ref as ref
    from test_gpu_adam import PARAMS, A, _assert_same, _hp, _join
    L = _L()
    for M, F in BUCKET_MF:
        case_ = A.shape_case(P, M, F, "groups" if entry_name == "groups_reg" else entry_name)
        s = case_.steps[0]
        W = A.width_of(M, F)
        c = 4 + 3 * M
        weight = 10.0
        if entry_name == "groups_reg":
            extra = np.zeros((P, W), dtype=np.float32)
            extra[:, c:c + 3] = ref.isotropic_rows(case_.params[:, c:c + 3], False, weight)[0]
            masks = (list(s.masks) + [None]) if s.masks is not None else None
            want = A.gaussian_step(case_.params, case_.exp_avg, case_.exp_avg_sq, list(s.buckets) + [extra], masks, case_.lrs, M, F,
                                   group_steps=s.group_steps, skip=s.skip)
        else:
            want = A.run(case_)[0]
        cols = dict(means3D=slice(0, 3), shs=slice(3, 3 + 3 * M), opacities=slice(c - 1, c), scales=slice(c, c + 3),
                    rotations=slice(c + 3, c + 7), language=slice(c + 7, W))
        shapes = dict(means3D=(P, 3), shs=(P, M, 3), opacities=(P, 1), scales=(P, 3), rotations=(P, 4), language=(P, F))

        def entry(case):
            params = {k: case.inout(k, torch.from_numpy(np.ascontiguousarray(case_.params[:, cols[k]])).reshape(shapes[k]).to(DEV))
                      for k in PARAMS}
            m = case.inout("exp_avg", torch.from_numpy(case_.exp_avg.copy()).to(DEV))
            v = case.inout("exp_avg_sq", torch.from_numpy(case_.exp_avg_sq.copy()).to(DEV))
            flats_t = [case.inout(f"bucket{i}", torch.from_numpy(b).to(DEV)) for i, b in enumerate(s.buckets)]
            words = s.masks if s.masks is not None else [None] * len(flats_t)
            masks_t = [None if w is None else case.inout(f"mask{i}", torch.from_numpy(w.view(np.int64).copy()).to(DEV))
                       for i, w in enumerate(words)]
            flats = (C.c_void_p * len(flats_t))(*[t.data_ptr() for t in flats_t])
            mk = (C.c_void_p * len(flats_t))(*[t.data_ptr() if t is not None else None for t in masks_t])
            tail = [_p(params[k]) for k in PARAMS] + [m.data_ptr(), v.data_ptr()]
            if entry_name == "step":
                _check_rc(L.olsr_adam_step(P, M, F, C.byref(_hp(case_, s.step)), flats_t[0].data_ptr(), *tail, _stream()))
            elif entry_name == "sum":
                _check_rc(L.olsr_adam_step_sum(P, M, F, C.byref(_hp(case_, s.step)), len(flats_t), flats, *tail, _stream()))
            elif entry_name == "masked":
                _check_rc(L.olsr_adam_step_masked(P, M, F, C.byref(_hp(case_, s.step)), len(flats_t), flats, mk, *tail, _stream()))
            else:
                gp = _abi.OlsrAdamGroupParams(base=_hp(case_, 1), skip_mask=sum(1 << g for g in s.skip))
                for g in range(7):
                    gp.group_step[g] = s.group_steps[g]
                mk_arg = mk if s.masks is not None else None
                if entry_name == "groups":
                    _check_rc(L.olsr_adam_step_groups(P, M, F, C.byref(gp), len(flats_t), flats, mk_arg, *tail, _stream()))
                else:
                    reg = _abi.OlsrAdamReg(isotropic_weight=weight, activations=0, P_total=P)
                    _check_rc(L.olsr_adam_step_groups_reg(P, M, F, C.byref(gp), len(flats_t), flats, mk_arg, *tail, C.byref(reg),
                                                          _stream()))
            torch.cuda.synchronize()
        out = three_ways(entry, misaligned=False)
        for i, b in enumerate(s.buckets):   # inputs: untouched
            assert A.same_bits(out[f"bucket{i}"].cpu().numpy(), b).all()
        got = (_join({k: out[k] for k in PARAMS}), out["exp_avg"].cpu().numpy(), out["exp_avg_sq"].cpu().numpy())
        _assert_same(f"{entry_name} P={P} M={M} F={F}", got, want)


# ------------------------------------------------------------------------------------------------ sparse exchange
# the pack counts and scans 1024 rows per block: scratch is int32[ceil(P / 1024)] (olsr_sparse_exchange_scratch_ints)
@pytest.mark.parametrize("P", [1, 1023, 1024, 1025])
def test_sparse_exchange(hip, P):
    """mask -> pack -> unpack on one rank (the two collectives are identities): the statements of
    tests/test_gpu_sparse_exchange.py's _two_ranks, all exact.  Capacity equal to the union's row count, and one less: the
    overflow is reported and only the first `capacity` rows are packed."""
    from test_gpu_sparse_exchange import _bits, _bucket
    L = _L()
    width = 29
    rows = min(P, max(1, P // 3))
    flat, den, rad, mask = _bucket(P, width, rows, 1, torch.device(DEV), "superset")
    union = (flat != 0).any(1)
    n = int(union.sum())
    urows = torch.nonzero(union).reshape(-1)
    nscr = int(L.olsr_sparse_exchange_scratch_ints(P))
    assert nscr == (P + 1023) // 1024 and n >= 1

    def mask_entry(case):
        imax = case.new("imax", (2 * P,), I32)
        _check_rc(L.olsr_sparse_exchange_mask(P, width, flat.data_ptr(), mask.data_ptr(), rad.data_ptr(), imax.data_ptr(), _stream()))
    imax = three_ways(mask_entry, misaligned=False)["imax"]
    assert torch.equal(imax[:P].bool(), union) and torch.equal(imax[P:], rad)

    for cap in (n, n - 1):
        if cap < 1:
            continue
        used = min(n, cap)

        def pack_entry(case):
            mr, rm = case.inout("max_radii", rad), case.inout("row_mask", mask)
            idx, fsum = case.new("idx", (cap,), I32), case.new("fsum", (cap * width + 2 * P,), F32)
            status = case.new("status", (2,), I32)
            scr = case.scratch(4 * nscr, misalign_ok=False).view(I32)
            _check_rc(L.olsr_sparse_exchange_pack(P, width, cap, flat.data_ptr(), imax.data_ptr(), mr.data_ptr(), rm.data_ptr(),
                                                  den.data_ptr(), idx.data_ptr(), fsum.data_ptr(), scr.data_ptr(), status.data_ptr(),
                                                  _stream()))
        out = three_ways(pack_entry, misaligned=False)
        assert out["status"].tolist() == [n, int(n > cap)]
        assert torch.equal(out["idx"][:used].long(), urows[:used]) and bool((out["idx"][used:] == P).all())
        assert torch.equal(out["fsum"][: cap * width].view(cap, width)[:used].nan_to_num(7.0), flat[urows[:used]].nan_to_num(7.0))
        assert torch.equal(out["fsum"][cap * width:].view(P, 2), den) and torch.equal(out["max_radii"], rad)
        assert torch.equal(_bits(out["row_mask"], P), union)
        assert not bool(_bits(out["row_mask"], out["row_mask"].numel() * 64)[P:].any())
        idx, fsum = out["idx"], out["fsum"]

        def unpack_entry(case):
            f2, d2 = case.inout("flat", torch.zeros_like(flat)), case.new("densify", (P, 2), F32)
            _check_rc(L.olsr_sparse_exchange_unpack(P, width, cap, idx.data_ptr(), fsum.data_ptr(), f2.data_ptr(), d2.data_ptr(),
                                                    _stream()))
        out = three_ways(unpack_entry, misaligned=False)
        assert torch.equal(out["densify"], den)
        assert torch.equal(out["flat"][urows[:used]].nan_to_num(7.0), flat[urows[:used]].nan_to_num(7.0))
        if used == n:
            assert torch.equal(out["flat"].nan_to_num(7.0), flat.nan_to_num(7.0))


# ------------------------------------------------------------------------------------------------ the front end
# k_frontend.hip: 256 threads, 16 elements per thread of a pass over N (FE_CHUNK = 4096), the threshold pass one pixel per
# thread (256), the covisibility pass 8 Gaussians per thread (2048 per block).  The scratch is carved: the select's state, four
# histograms, N keys.
@pytest.mark.parametrize("W,Hh,mode", [(65, 63, "global"), (64, 64, "global"), (17, 241, "global"),   # 4095, 4096, 4097 pixels
                                       (65, 63, "blocks"), (64, 64, "blocks"), (33, 65, "blocks")])   # blocks of 1 x 2 / 2 x 2 / 2 x 1
def test_grad_mask(hip, W, Hh, mode):
    import frontend_ref as R
    from test_gpu_frontend import frame_image, same
    L = _L()
    img, thr = frame_image(W * 1000 + Hh, Hh, W), 1.1
    want = (R.grad_mask_blocks if mode == "blocks" else R.grad_mask_global)(img, thr, np.float32)[0]
    t = torch.from_numpy(img).to(DEV)
    N = W * Hh

    def entry(case):
        mask = case.new("mask", (Hh, W), F32)
        scratch = case.scratch(L.olsr_frontend_scratch_bytes(N)) if mode == "global" else None
        _check_rc(L.olsr_grad_mask(W, Hh, N, 0 if mode == "blocks" else 1, thr, t.data_ptr(), mask.data_ptr(), _p(scratch), _stream()))
    out = three_ways(entry)
    assert same(out["mask"].cpu().numpy(), want)


@pytest.mark.parametrize("N", [1, 4095, 4096, 4097])
def test_median_depth(hip, N):
    import frontend_ref as R
    from test_gpu_frontend import depth_case, same
    L = _L()
    d, o, m = depth_case(N, N)
    td, to, tm = torch.from_numpy(d).to(DEV), torch.from_numpy(o).to(DEV), torch.from_numpy(m.astype(np.uint8)).to(DEV)
    for mask, dev_mask in ((None, None), (m, tm)):
        def entry(case):
            med, cnt = case.new("median", (1,), F32), case.new("count", (1,), I32)
            scratch = case.scratch(L.olsr_frontend_scratch_bytes(N))
            _check_rc(L.olsr_median_depth(N, td.data_ptr(), to.data_ptr(), _p(dev_mask), scratch.data_ptr(), med.data_ptr(),
                                          cnt.data_ptr(), _stream()))
        out = three_ways(entry)
        want, n = R.median_depth(d, o, mask)
        assert int(out["count"]) == n and same(out["median"].cpu().numpy()[0], np.float32(want))


@pytest.mark.parametrize("P", [1, 2047, 2048, 2049])
def test_covisibility_and_keyframe_decide(hip, P):
    import frontend_ref as R
    from test_gpu_frontend import TRAIN, random_pose, same
    L = _L()
    for K in (0, 1, 16):
        g = np.random.default_rng(1000 * K + P)
        n_touched = (g.integers(0, 5, size=P) * (g.random(P) < 0.7)).astype(np.int32)
        vis = [((g.random(P) < 0.5) * g.integers(1, 255, size=P)).astype(np.uint8) for _ in range(K)]
        kf = [random_pose(g, 1.5) for _ in range(K)]
        cur_pose, median = random_pose(g, 1.5), np.float32(2.5)
        params = dict(window_size=8, check_time=1, single_thread=0, **TRAIN)
        nt = torch.from_numpy(n_touched).to(DEV)
        tv = [torch.from_numpy(v).to(DEV) for v in vis]
        views = _abi.OlsrCovisViews(K=K)
        for k, t in enumerate(tv):
            views.vis[k] = t.data_ptr()
        med = torch.tensor([median], dtype=F32, device=DEV)
        cp = torch.from_numpy(np.ascontiguousarray(cur_pose, dtype=np.float32).reshape(16)).to(DEV)
        kp = torch.from_numpy(np.ascontiguousarray(kf, dtype=np.float32).reshape(K, 16)).to(DEV) if K else None
        p = _abi.OlsrKeyframeDecideParams(window_len=K, **{k: (float(v) if k.startswith("kf_") else int(v)) for k, v in params.items()})

        def entry(case):
            cur, counts = case.new("cur", (P,), U8), case.new("counts", (_abi.COVIS_COUNTS,), torch.int64)
            rec = case.new("record", (_abi.KEYFRAME_RECORD_BYTES // 4,), I32)
            _check_rc(L.olsr_covisibility(P, nt.data_ptr(), C.byref(views), cur.data_ptr(), counts.data_ptr(), _stream()))
            _check_rc(L.olsr_keyframe_decide(C.byref(p), counts.data_ptr(), med.data_ptr(), cp.data_ptr(), _p(kp), rec.data_ptr(),
                                             _stream()))
        out = three_ways(entry, misaligned=False)
        wcur, wcounts = R.covisibility(n_touched, vis)
        assert np.array_equal(out["cur"].cpu().numpy(), wcur) and np.array_equal(out["counts"].cpu().numpy(), wcounts)
        wi, wf = R.record(R.decide(params, wcounts, median, cur_pose, kf, np.float32), wcounts, median)
        raw = out["record"].cpu().numpy()
        assert np.array_equal(raw[:8], wi) and same(raw[8:].view(np.float32).copy(), wf)


# ------------------------------------------------------------------------------------------------ the losses
# 45 x 30: a width that is no multiple of 4 (the pixel passes load four pixels where a row allows it), 157 x 101: several blocks
# each way with ragged edges.  Scratch: per-block partial sums, carved.
LOSS_SIZES = [(45, 30), (157, 101)]


def _loss_case(F, Hh, W, lh, lw):
    g = torch.Generator().manual_seed(F + Hh)
    c = dict(image=torch.rand(3, Hh, W, generator=g), depth=torch.rand(1, Hh, W, generator=g) * 5,
             lang=torch.randn(F, Hh, W, generator=g) * 0.3 if F else None, gt_image=torch.rand(3, Hh, W, generator=g),
             gt_depth=torch.rand(Hh, W, generator=g) * 5, gt_lang=torch.randn(F, lh, lw, generator=g) * 0.3 if F else None,
             a=torch.tensor([0.11]), b=torch.tensor([-0.03]), opacity=torch.rand(1, Hh, W, generator=g) * 0.2 + 0.85,
             grad_mask=(torch.rand(Hh, W, generator=g) > 0.5).float())
    c["gt_image"][:, : Hh // 3] *= 0.001
    c["gt_depth"][:, : W // 4] = 0.0
    return c


@pytest.mark.parametrize("W,Hh", LOSS_SIZES)
@pytest.mark.parametrize("F", [0, 15])
def test_mapping_loss(hip, W, Hh, F):
    """Yardstick: oracle/loss_oracle.py under tests/test_gpu_loss.py's _close (and its bounds on the exposure gradient and on
    the language cotangent's sign flips)."""
    import test_gpu_loss as TL
    L = _L()
    lh, lw = 37, 53
    c = _loss_case(F, Hh, W, lh, lw)
    kw = dict(alpha=0.95, rgb_boundary_threshold=0.01, lamda_lang=1.0)
    ref = TL.loss_oracle.mapping_loss_and_grads(c["image"], c["depth"], c["lang"], c["gt_image"], c["gt_depth"], c["gt_lang"],
                                                c["a"], c["b"], **kw)
    d = {k: (None if v is None else v.to(DEV).contiguous()) for k, v in c.items()}
    expo = torch.cat([c["a"], c["b"]]).float().to(DEV)
    p = _abi.OlsrLossParams(width=W, height=Hh, F=F, lang_width=lw if F else 0, lang_height=lh if F else 0, initialization=0, **kw)

    def entry(case):
        o = dict(loss=case.new("loss", (4,), F32), dL_dimage=case.new("dL_dimage", (3, Hh, W), F32),
                 dL_ddepth=case.new("dL_ddepth", (1, Hh, W), F32), dL_dlanguage=case.new("dL_dlanguage", (F, Hh, W), F32),
                 dL_dexposure=case.new("dL_dexposure", (2,), F32))
        scratch = case.scratch(L.olsr_mapping_loss_scratch_bytes(W, Hh))
        _check_rc(L.olsr_mapping_loss(C.byref(p), _p(d["image"]), _p(d["depth"]), _p(d["lang"]), _p(d["gt_image"]), _p(d["gt_depth"]),
                                      _p(d["gt_lang"]), _p(expo), _p(o["dL_dimage"]), _p(o["dL_ddepth"]), _p(o["dL_dlanguage"]),
                                      _p(o["loss"]), _p(o["dL_dexposure"]), scratch.data_ptr(), _stream()))
    o = three_ways(entry)
    TL._close(o["loss"][0], ref["loss"], "loss")
    TL._close(o["loss"][1], ref["rgb"], "rgb")
    TL._close(o["loss"][2], ref["depth"], "depth")
    TL._close(o["dL_dimage"], ref["dL_dimage"], "dL_dimage")
    TL._close(o["dL_ddepth"], ref["dL_ddepth"], "dL_ddepth")
    if F:
        TL._close(o["loss"][3], ref["lang"], "lang")
        bad = int(((o["dL_dlanguage"].cpu() - ref["dL_dlanguage"]).abs() > TL.RTOL * float(ref["dL_dlanguage"].abs().max())).sum())
        assert bad <= TL.LANG_FLIPS, bad
    assert abs(float(o["dL_dexposure"][0]) - float(ref["dL_da"])) <= TL.EXPOSURE_ATOL
    assert abs(float(o["dL_dexposure"][1]) - float(ref["dL_db"])) <= TL.EXPOSURE_ATOL


@pytest.mark.parametrize("W,Hh", LOSS_SIZES)
@pytest.mark.parametrize("masked", [True, False])
def test_tracking_loss(hip, W, Hh, masked):
    """Yardstick: oracle/loss_oracle.py's tracking loss under tests/test_gpu_loss.py's _close."""
    import test_gpu_loss as TL
    L = _L()
    c = _loss_case(0, Hh, W, 0, 0)
    gm = c["grad_mask"] if masked else None
    ref = TL.loss_oracle.tracking_loss_and_grads(c["image"], c["depth"], c["opacity"], c["gt_image"], c["gt_depth"],
                                                 (gm.bool() if masked else torch.ones(Hh, W, dtype=torch.bool)).reshape(1, Hh, W),
                                                 c["a"], c["b"])   # (no mask = every pixel)
    d = {k: (None if v is None else v.to(DEV).contiguous()) for k, v in c.items()}
    expo = torch.cat([c["a"], c["b"]]).float().to(DEV)
    p = _abi.OlsrLossParams(width=W, height=Hh, F=0, lang_width=0, lang_height=0, initialization=0, alpha=0.95,
                            rgb_boundary_threshold=0.01, lamda_lang=0.0)

    def entry(case):
        o = dict(loss=case.new("loss", (4,), F32), dL_dimage=case.new("dL_dimage", (3, Hh, W), F32),
                 dL_ddepth=case.new("dL_ddepth", (1, Hh, W), F32), dL_dexposure=case.new("dL_dexposure", (2,), F32))
        scratch = case.scratch(L.olsr_mapping_loss_scratch_bytes(W, Hh))
        _check_rc(L.olsr_tracking_loss(C.byref(p), _p(d["image"]), _p(d["depth"]), _p(d["opacity"]), _p(d["gt_image"]), _p(d["gt_depth"]),
                                       _p(d["grad_mask"]) if masked else None, _p(expo), _p(o["dL_dimage"]), _p(o["dL_ddepth"]),
                                       _p(o["loss"]), _p(o["dL_dexposure"]), scratch.data_ptr(), _stream()))
    o = three_ways(entry)
    TL._close(o["loss"][0], ref["loss"], "loss")
    TL._close(o["dL_dimage"], ref["dL_dimage"], "dL_dimage")
    TL._close(o["dL_ddepth"], ref["dL_ddepth"], "dL_ddepth")
    assert abs(float(o["dL_dexposure"][0]) - float(ref["dL_da"])) <= TL.EXPOSURE_ATOL


@pytest.mark.parametrize("W,Hh", LOSS_SIZES)
def test_refinement_loss(hip, W, Hh):
    """Yardstick: tests/ssim_ref.py in float64, the error held to a multiple of the float32 restatement's own
    (tests/test_gpu_ssim.py's _check).  Scratch: partial sums and three [3,H,W] planes (one array), carved."""
    import ssim_ref
    import test_gpu_ssim as TS
    L = _L()
    lam = 0.2
    image, gt = TS._full_size_inputs("smooth", W, Hh, seed=W + Hh)
    truth = ssim_ref.loss_and_grad(image, gt, lam, dtype=torch.float64)
    ref32 = ssim_ref.loss_and_grad(image, gt, lam, dtype=torch.float32)
    a, g = image.to(DEV).contiguous(), gt.to(DEV).contiguous()

    def entry(case):
        loss, grad = case.new("loss", (4,), F32), case.new("dL_dimage", (3, Hh, W), F32)
        scratch = case.scratch(L.olsr_refinement_loss_scratch_bytes(W, Hh))
        _check_rc(L.olsr_refinement_loss(W, Hh, lam, a.data_ptr(), g.data_ptr(), grad.data_ptr(), loss.data_ptr(), scratch.data_ptr(),
                                         _stream()))
    o = three_ways(entry)
    TS._check(f"{W}x{Hh}", "smooth", dict(loss=o["loss"].cpu(), dL_dimage=o["dL_dimage"].cpu()), truth, ref32)


# ------------------------------------------------------------------------------------------------ cloud metrics
# tiles of 256 points (CM_TILE), partial results per chunk and point (Carver: offsets, then arrays of total1 / total2 rows)
CLOUD_BATCHES = {"B1": ["uniform_255_257"], "B3_one_empty": ["uniform_257_255", None, "uniform_65_63"]}


def _cloud_batch(names):
    import cloud_metrics_ref as R
    cases = R.cases()
    pairs = [cases[n] if n else (np.zeros((0, 3), np.float32), cases["uniform_3_5"][1]) for n in names]
    off1 = np.concatenate([[0], np.cumsum([len(p[0]) for p in pairs])]).astype(np.int32)
    off2 = np.concatenate([[0], np.cumsum([len(p[1]) for p in pairs])]).astype(np.int32)
    x = torch.from_numpy(np.concatenate([p[0] for p in pairs]).astype(np.float32)).to(DEV)
    y = torch.from_numpy(np.concatenate([p[1] for p in pairs]).astype(np.float32)).to(DEV)
    return pairs, off1, off2, x, y


@pytest.mark.parametrize("batch", sorted(CLOUD_BATCHES))
def test_chamfer(hip, batch):
    """Yardstick: tests/cloud_metrics_ref.py's float32 brute force, per point bit for bit, the means to the bound of
    tests/test_gpu_cloud_metrics.py::test_chamfer_points_equal_the_float32_brute_force; an empty side gives NaN and -1."""
    import cloud_metrics_ref as R
    from test_gpu_cloud_metrics import mean_bound
    L = _L()
    pairs, off1, off2, x, y = _cloud_batch(CLOUD_BATCHES[batch])
    B, t1, t2 = len(pairs), int(off1[-1]), int(off2[-1])
    max1, max2 = int(np.diff(off1).max()), int(np.diff(off2).max())

    def entry(case):
        o = dict(d1=case.new("d1", (t1,), F32), i1=case.new("i1", (t1,), I32), d2=case.new("d2", (t2,), F32), i2=case.new("i2", (t2,), I32),
                 mean=case.new("mean", (B, 2), torch.float64), valid=case.new("valid", (B,), I32))
        scratch = case.scratch(L.olsr_chamfer_scratch_bytes(B, t1, t2))
        _check_rc(L.olsr_chamfer(B, off1.ctypes.data, off2.ctypes.data, max1, max2, x.data_ptr(), y.data_ptr(), o["d1"].data_ptr(),
                                 o["i1"].data_ptr(), o["d2"].data_ptr(), o["i2"].data_ptr(), o["mean"].data_ptr(), o["valid"].data_ptr(),
                                 scratch.data_ptr(), _stream()))
    o = {k: v.cpu().numpy() for k, v in three_ways(entry).items()}
    for b, (px, py) in enumerate(pairs):
        s1, s2 = slice(off1[b], off1[b + 1]), slice(off2[b], off2[b + 1])
        if len(px) == 0 or len(py) == 0:
            assert np.isnan(o["mean"][b]).all() and np.isnan(o["d1"][s1]).all() and np.isnan(o["d2"][s2]).all()
            assert (o["i1"][s1] == -1).all() and (o["i2"][s2] == -1).all() and o["valid"][b] == 0
            continue
        want = R.chamfer_ref(px, py, np.float32)
        assert np.array_equal(o["d1"][s1].view(np.uint32), want["min_d2_x"].view(np.uint32))
        assert np.array_equal(o["d2"][s2].view(np.uint32), want["min_d2_y"].view(np.uint32))
        assert np.array_equal(o["i1"][s1], want["nn_x"]) and np.array_equal(o["i2"][s2], want["nn_y"]) and o["valid"][b] == 1
        for k, (key, n) in enumerate((("x_to_y", len(px)), ("y_to_x", len(py)))):
            assert abs(o["mean"][b, k] - want[key]) <= mean_bound(n, want[key])


@pytest.mark.parametrize("batch", sorted(CLOUD_BATCHES))
def test_emd_cost(hip, batch):
    """Yardstick: tests/cloud_metrics_ref.py's float64 truth under the rule of
    tests/test_gpu_cloud_metrics.py::test_emd_against_the_truth (4 x the float32 variants' own deviation, 16 x 2^-24 at least)."""
    import cloud_metrics_ref as R
    from test_gpu_cloud_metrics import ULP
    L = _L()
    pairs, off1, off2, x, y = _cloud_batch(CLOUD_BATCHES[batch])
    B, t1, t2 = len(pairs), int(off1[-1]), int(off2[-1])
    max1, max2 = int(np.diff(off1).max()), int(np.diff(off2).max())

    def entry(case):
        cost, res, valid = case.new("cost", (B,), torch.float64), case.new("residual", (B, 2), F32), case.new("valid", (B,), I32)
        scratch = case.scratch(L.olsr_emd_scratch_bytes(B, t1, t2))
        _check_rc(L.olsr_emd_cost(B, off1.ctypes.data, off2.ctypes.data, max1, max2, x.data_ptr(), y.data_ptr(), cost.data_ptr(),
                                  res.data_ptr(), valid.data_ptr(), scratch.data_ptr(), _stream()))
    o = {k: v.cpu().numpy() for k, v in three_ways(entry).items()}
    for b, (px, py) in enumerate(pairs):
        if len(px) == 0 or len(py) == 0:
            assert np.isnan(o["cost"][b]) and np.isnan(o["residual"][b]).all() and o["valid"][b] == 0
            continue
        truth, dev_c, dev_r = R.emd_yardstick(px, py)
        assert abs(o["cost"][b] - truth["cost"]) <= max(4.0 * dev_c, 16 * ULP * abs(truth["cost"]))
        err_r = max(abs(float(o["residual"][b, k]) - truth["residual"][k]) for k in (0, 1))
        assert err_r <= max(4.0 * dev_r, 16 * ULP * max(len(px), len(py))) and o["valid"][b] == 1


# ------------------------------------------------------------------------------------------------ the activation hook
@pytest.mark.parametrize("P", [1, 255, 256, 257])   # a Gaussian per thread, 256 per block (olsr_diag.hip)
def test_debug_activate(hip, P):
    """Yardstick: tests/test_gpu_activations.py::test_activation_hook_against_float64 — expf within 1 ulp of the float64 value,
    the sigmoid within (2 (1 - sigma) + 2) x 2^-24 x sigma, an unflagged array copied bit for bit."""
    import act_ref as A
    L = _L()
    g = torch.Generator().manual_seed(P)
    xo = (torch.randn(P, generator=g) * 3).to(DEV)
    xs = (torch.randn(P, 3, generator=g) * 2 - 3).to(DEV)
    xr = torch.randn(P, 4, generator=g).to(DEV)

    def entry(case):
        o, sc_, r = case.new("opacities", (P,), F32), case.new("scales", (P, 3), F32), case.new("rotations", (P, 4), F32)
        _check_rc(L.olsr_debug_activate(P, _abi.ACT_OPACITY_SIGMOID | _abi.ACT_SCALE_EXP, xo.data_ptr(), xs.data_ptr(), xr.data_ptr(),
                                        o.data_ptr(), sc_.data_ptr(), r.data_ptr(), _stream()))
    out = three_ways(entry, misaligned=False)
    assert torch.equal(out["rotations"], xr)
    assert A.ulp_error(out["scales"].cpu().numpy(), np.exp(xs.cpu().numpy().astype(np.float64))).max() <= 1.0
    sig = 1.0 / (1.0 + np.exp(-xo.cpu().numpy().astype(np.float64)))
    err = np.abs(out["opacities"].cpu().numpy().astype(np.float64) - sig)
    assert (err <= (2.0 * (1.0 - sig) + 2.0) * A.U * sig + A.TINY).all()


# ------------------------------------------------------------------------------------------------ pose steps
POSE_WORDS = dict(tau=slice(64, 70), tau_m=slice(52, 58), tau_v=slice(58, 64), exposure=slice(70, 72), exposure_m=slice(72, 74),
                  exposure_v=slice(74, 76))


def _pose_inputs(s):
    from test_gpu_pose import G
    state = np.zeros(80, dtype=np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = G[f"seq{s}_R0"], G[f"seq{s}_T0"]
    state[:16] = T.reshape(-1)
    lr = tuple(float(x) for x in G[f"seq{s}_lr"])
    hp = _abi.OlsrPoseParams(lr_rot=lr[0], lr_trans=lr[1], lr_exposure=lr[2], beta1=0.9, beta2=0.999, eps=1e-8,
                             converged_threshold=1e-4, step=1)
    return state, G[f"seq{s}_grad_tau"][0], G[f"seq{s}_grad_exposure"][0], G[f"seq{s}_proj"].astype(np.float32), lr, hp


@pytest.mark.parametrize("V", [1, 3])
def test_pose_steps(hip, V):
    """olsr_pose_step and olsr_pose_step_gated on the first step of the golden sequences (one wave, an 80-float state and two
    status words per view), olsr_window_pose_step over V views.  Yardsticks: tests/adam_ref.py's pose_step_adam, bit for bit,
    and the golden pose within 5e-7 (tests/test_gpu_pose.py); a gated step keeps the optimiser's words; the window entry has
    the single call's bits per view (include/olsr.h)."""
    import adam_ref
    from test_gpu_pose import POSE_STEP_ATOL, G
    L = _L()
    singles = []
    for v in range(V):
        state0, gt, ge, proj, lr, hp = _pose_inputs(v)
        d_gt, d_ge, d_proj = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV) for a in (gt, ge, proj.reshape(-1))]

        def entry(case, gated=None):
            st = case.inout("state", torch.from_numpy(state0).to(DEV))
            status = case.inout("status", torch.zeros(2, dtype=I32, device=DEV))
            if gated is None:
                _check_rc(L.olsr_pose_step(C.byref(hp), d_gt.data_ptr(), d_ge.data_ptr(), d_proj.data_ptr(), st.data_ptr(),
                                           status.data_ptr(), _stream()))
            else:
                _check_rc(L.olsr_pose_step_gated(C.byref(hp), d_gt.data_ptr(), d_ge.data_ptr(), d_proj.data_ptr(), st.data_ptr(),
                                                 status.data_ptr(), gated.data_ptr(), _stream()))
        out = three_ways(entry, misaligned=False)
        after = out["state"].cpu().numpy()
        want = adam_ref.pose_step_adam(state0, gt, ge, lr, 1)
        for name, sl in POSE_WORDS.items():
            assert adam_ref.same_bits(after[sl], want[name]).all(), (v, name)
        np.testing.assert_allclose(after[:16].reshape(4, 4)[:3, :3], G[f"seq{v}_R"][0], rtol=0, atol=POSE_STEP_ATOL)
        np.testing.assert_allclose(after[:16].reshape(4, 4)[:3, 3], G[f"seq{v}_T"][0], rtol=0, atol=POSE_STEP_ATOL)
        np.testing.assert_allclose(after[16:32].reshape(4, 4), G[f"seq{v}_view"][0], rtol=0, atol=POSE_STEP_ATOL)
        assert out["status"].tolist() == [int(bool(G[f"seq{v}_converged"][0])), 1]
        singles.append(out)
        missed = torch.tensor([5, 3], dtype=I32, device=DEV)   # a frame that missed its depth cut-offs: no step
        out = three_ways(lambda c: entry(c, missed), misaligned=False)
        kept = out["state"].cpu().numpy()
        assert kept[:16].tobytes() == state0[:16].tobytes() and kept[52:76].tobytes() == state0[52:76].tobytes()
        assert out["status"].tolist() == [0, 0]
        used = torch.tensor([5, 0], dtype=I32, device=DEV)
        out = three_ways(lambda c: entry(c, used), misaligned=False)
        assert H.same_bits(out["state"], singles[-1]["state"]) and H.same_bits(out["status"], singles[-1]["status"])

    # every view shares one projection matrix and one set of rates in the window entry: sequence 0's, on each view's own pose
    state0, _, _, proj, lr, hp = _pose_inputs(0)
    states = np.stack([_pose_inputs(v)[0] for v in range(V)])
    gts = np.stack([_pose_inputs(v)[1] for v in range(V)]).astype(np.float32)
    ges = np.stack([_pose_inputs(v)[2] for v in range(V)]).astype(np.float32)
    d_gt, d_ge, d_proj = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (gts, ges, proj.reshape(-1))]
    flags = (C.c_int32 * V)(*[_abi.WINDOW_OPT_POSE | _abi.WINDOW_OPT_EXPOSURE] * V)

    def window(case):
        st = case.inout("state", torch.from_numpy(states).to(DEV))
        status = case.inout("status", torch.zeros(V, 2, dtype=I32, device=DEV))
        _check_rc(L.olsr_window_pose_step(C.byref(hp), V, flags, d_gt.data_ptr(), d_ge.data_ptr(), d_proj.data_ptr(), st.data_ptr(),
                                          status.data_ptr(), None, _stream()))
    out = three_ways(window, misaligned=False)
    for v in range(V):
        def one(case):
            st = case.inout("state", torch.from_numpy(states[v]).to(DEV))
            status = case.inout("status", torch.zeros(2, dtype=I32, device=DEV))
            _check_rc(L.olsr_pose_step(C.byref(hp), d_gt[v].data_ptr(), d_ge[v].data_ptr(), d_proj.data_ptr(), st.data_ptr(),
                                       status.data_ptr(), _stream()))
        single = Case(False)
        one(single)
        torch.cuda.synchronize()
        assert H.same_bits(out["state"][v], single.out["state"]) and H.same_bits(out["status"][v], single.out["status"]), v


# ------------------------------------------------------------------------------------------------ the fused loss
@pytest.mark.parametrize("W,Hh,tile", [(45, 30, 15), (157, 101, 16)])
@pytest.mark.parametrize("tracking", [False, True])
def test_forward_async_loss(hip, W, Hh, tile, tracking):
    """olsr_forward_async_loss: the forward with the mapping (15 language channels) or the tracking loss (with a gradient mask)
    in the composite's epilogue.  Yardstick: the two-kernel path on the same render, under the assertions of
    tests/test_gpu_loss.py::test_fused_mapping_loss_equals_the_two_kernel_path — images and cotangents bit for bit, the loss
    under _close, the exposure gradient within FUSED_EXPOSURE_ATOL.  State buffers and the loss's per-tile partial sums: Carver."""
    import test_gpu_loss as TL
    from online_lang_splatting_amd import losses
    L = _L()
    F = 15
    sc = make_scene(1025, W, Hh, F, seed=500 + W)
    mode, binning = _abi.BWD_REFERENCE, _abi.BINNING_ELLIPSE
    first = Case(False)
    raster(first, sc, tile, mode, binning, 3)
    R = int(first.out["R"])
    assert R > 1
    s, keep = _scene_struct(sc, tile, mode, binning)
    P = sc.P
    lh, lw = 37, 53
    c = {k: (None if v is None else v.to(DEV).contiguous()) for k, v in _loss_case(F, Hh, W, lh, lw).items()}
    expo = torch.cat([c["a"], c["b"]]).float().contiguous()
    lang = not tracking
    if tracking:
        two = losses.tracking_loss(first.out["color"], first.out["depth"], first.out["opacity"], c["gt_image"], c["gt_depth"],
                                   c["grad_mask"], expo)
    else:
        two = losses.mapping_loss(first.out["color"], first.out["depth"], first.out["language"], c["gt_image"], c["gt_depth"],
                                  c["gt_lang"], expo)
    p = _abi.OlsrLossParams(width=W, height=Hh, F=F if lang else 0, lang_width=lw if lang else 0, lang_height=lh if lang else 0,
                            initialization=0, alpha=0.95, rgb_boundary_threshold=0.01, lamda_lang=1.0,
                            one_minus_alpha=1.0 - 0.95)   # as losses.py fills it: the yardstick below goes through losses.py

    def entry(case):
        geom, img = case.scratch(L.olsr_geometry_bytes(P, F)), case.scratch(L.olsr_image_bytes(W, Hh, tile))
        binb = case.scratch(L.olsr_binning_bytes(R, F))
        o = [case.new(k, shape, dt) for k, shape, dt in (
            ("color", (3, Hh, W), F32), ("language", (F, Hh, W), F32), ("depth", (1, Hh, W), F32), ("opacity", (1, Hh, W), F32),
            ("radii", (P,), I32), ("n_touched", (P,), I32))]
        nr = case.new("num_rendered", (2,), I32)
        g = dict(loss=case.new("loss", (4,), F32), dL_dimage=case.new("dL_dimage", (3, Hh, W), F32),
                 dL_ddepth=case.new("dL_ddepth", (1, Hh, W), F32), dL_dexposure=case.new("dL_dexposure", (2,), F32),
                 dL_dlanguage=case.new("dL_dlanguage", (F, Hh, W), F32) if lang else None)
        scratch = case.scratch(L.olsr_fused_loss_scratch_bytes(W, Hh, tile))
        lf = _abi.OlsrLossFusion(params=p, tracking=int(tracking), skip_images=0, gt_image=_p(c["gt_image"]), gt_depth=_p(c["gt_depth"]),
                                 gt_language=_p(c["gt_lang"]) if lang else None, exposure=_p(expo),
                                 grad_mask=_p(c["grad_mask"]) if tracking else None, dL_dimage=_p(g["dL_dimage"]),
                                 dL_ddepth=_p(g["dL_ddepth"]), dL_dlanguage=_p(g["dL_dlanguage"]), loss=_p(g["loss"]),
                                 dL_dexposure=_p(g["dL_dexposure"]), scratch=_p(scratch))
        _check_rc(L.olsr_forward_async_loss(C.byref(s), geom.data_ptr(), binb.data_ptr(), R, img.data_ptr(), *[_p(t) for t in o],
                                            _p(nr), None, C.byref(lf), _stream()))
        torch.cuda.synchronize()
        if not lang:
            case.out.pop("dL_dlanguage", None)
    out = three_ways(entry)
    assert out["num_rendered"].tolist() == [R, 0]
    for k in FWD_KEYS:
        assert H.same_bits(out[k], first.out[k]), k
    assert torch.equal(out["dL_dimage"], two["dL_dimage"]) and torch.equal(out["dL_ddepth"], two["dL_ddepth"])
    if lang:
        assert torch.equal(out["dL_dlanguage"], two["dL_dlanguage"])
    TL._close(out["loss"], two["loss"], "loss")
    assert float(two["loss"][0]) > 0
    assert float((out["dL_dexposure"] - two["dL_dexposure"]).abs().max()) <= TL.FUSED_EXPOSURE_ATOL


# ------------------------------------------------------------------------------------------------ the language codec
# k_lang_codec.hip: 256 rows per block, one float32 partial gradient [2351] per block in the scratch (carved: the gradient
# partials, then the loss partials): one row, one row short of a block, a whole block, one row into the second
_CODEC_REFS = {}


def _codec_case(N):
    import lang_codec_ref as R
    if N not in _CODEC_REFS:
        flat, q, _ = R.make_case(N, 5)
        x = R.unit(q)
        _CODEC_REFS[N] = (flat, x, R.train(flat, x, 1e-3, 1, torch.float64), R.train(flat, x, 1e-3, 1, torch.float32))
    return _CODEC_REFS[N]


@pytest.mark.parametrize("layout", ["rows", "channels"])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_lang_ae(hip, N, layout):
    """olsr_lang_ae_train_step (one step from zero moments, with the codes and the gradient), _encode and _decode.  Yardstick:
    tests/lang_codec_ref.py in float64 under tests/test_gpu_lang_codec.py's _ratio_rule / _scalar_rule (_check_step0, and
    test_encode_decode_are_the_train_steps_path for decode); encode gives the train step's codes bit for bit."""
    import lang_codec_ref as R
    from online_lang_splatting_amd.lang_codec import LAYOUTS
    from test_gpu_lang_codec import LOSS_NAMES, _ratio_rule, _scalar_rule
    L = _L()
    flat, x, t64, t32 = _codec_case(N)
    lay = LAYOUTS[layout]
    code_shape = (N, _abi.LANG_AE_CODE) if layout == "rows" else (_abi.LANG_AE_CODE, N)
    xd, fd = x.to(DEV).contiguous(), flat.to(DEV).contiguous()
    hp = _abi.OlsrLangAeParams(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=0, code_layout=lay, in_dim=_abi.LANG_AE_IN,
                               hidden_dim=_abi.LANG_AE_HIDDEN, code_dim=_abi.LANG_AE_CODE)

    def train(case):
        params = case.inout("params", fd)
        m, v = case.inout("exp_avg", torch.zeros_like(fd)), case.inout("exp_avg_sq", torch.zeros_like(fd))
        step = case.inout("step", torch.zeros(1, dtype=I32, device=DEV))
        loss, codes, grad = case.new("loss", (4,), F32), case.new("codes", code_shape, F32), case.new("grad", (R.N_PARAMS,), F32)
        scratch = case.scratch(L.olsr_lang_ae_scratch_bytes(N))
        _check_rc(L.olsr_lang_ae_train_step(C.byref(hp), N, xd.data_ptr(), params.data_ptr(), m.data_ptr(), v.data_ptr(), step.data_ptr(),
                                            loss.data_ptr(), codes.data_ptr(), grad.data_ptr(), scratch.data_ptr(), _stream()))
    out = three_ways(train)
    label = f"N = {N} {layout}"
    grad, loss = out["grad"].cpu(), out["loss"].cpu()
    codes = out["codes"].cpu() if layout == "rows" else out["codes"].cpu().t()
    for (name, _), g_hip, g_t, g_r in zip(R.STATE, R.unflatten(grad).values(), R.unflatten(t64["grad0"]).values(),
                                          R.unflatten(t32["grad0"]).values()):
        _ratio_rule(f"{label} d {name}", g_hip, g_t, g_r)
    for k, name in enumerate(LOSS_NAMES):
        _scalar_rule(f"{label} {name}", loss[k], t64["loss"][0, k], t32["loss"][0, k])
    _ratio_rule(f"{label} codes", codes, t64["codes_pre0"], t32["codes_pre0"])
    assert int(out["step"]) == 1 and not torch.equal(out["params"].cpu(), flat)
    trained = out["codes"]

    def encode(case):
        codes = case.new("codes", code_shape, F32)
        _check_rc(L.olsr_lang_ae_encode(N, xd.data_ptr(), fd.data_ptr(), lay, codes.data_ptr(), _stream()))
    enc = three_ways(encode, misaligned=False)["codes"]
    assert torch.equal(enc, trained)

    def decode(case):
        recon = case.new("recon", (N, _abi.LANG_AE_IN), F32)
        _check_rc(L.olsr_lang_ae_decode(N, enc.data_ptr(), fd.data_ptr(), lay, recon.data_ptr(), _stream()))
    rec = three_ways(decode, misaligned=False)["recon"].cpu()
    _ratio_rule(f"{label} decode", rec, R.codec_from(flat, torch.float64).decode(t64["codes_pre0"]).detach(),
                R.codec_from(flat, torch.float32).decode(t32["codes_pre0"]).detach())


# ------------------------------------------------------------------------------------------------ text queries
# k_lang_query.hip: stage A takes 64 pixels per tile of the matrix cores, stage B works in 16 x 16 and 32 x 8 pixel tiles: 24 x 40
# = 960 pixels is 15 whole tiles of 64, 33 x 31 = 1023 one pixel short of 16, with odd extents.  Scratch: carved.
@pytest.mark.parametrize("h,w,n_pos,n_labels", [(24, 40, 3, 2), (33, 31, 2, 0)])
def test_lang_query(hip, h, w, n_pos, n_labels):
    """olsr_lang_query_sims and _relevancy at the codes' own size.  Yardstick: tests/lang_query_ref.py under the statements of
    tests/test_gpu_lang_query.py's _check (its _check_outputs)."""
    import lang_query_ref as R
    from test_gpu_lang_query import _check_outputs, _query, _reference
    L = _L()
    case_ = R.make_case(h, w, 20 + n_pos, n_pos, n_labels)
    t64, t32 = _reference(case_, None, None)
    q = _query(case_)
    codes = case_["codes"].to(DEV).contiguous()
    p = q._params("extents", codes, None, None, want_mask=True, want_labels=n_labels > 0)
    K = int(p.K)

    def sims_entry(case):
        sims = case.new("similarities", (K, h, w), F32)
        _check_rc(L.olsr_lang_query_sims(C.byref(p), codes.data_ptr(), q.codec.flat.data_ptr(), q.decoder.flat.data_ptr(),
                                         q._phrases.data_ptr(), sims.data_ptr(), _stream()))
    sims = three_ways(sims_entry, misaligned=False)["similarities"]

    def relevancy(case):
        o = dict(relevancy=case.new("relevancy", (n_pos, h, w), F32), smoothed=case.new("smoothed", (n_pos, h, w), F32),
                 blended=case.new("blended", (n_pos, h, w), F32), score=case.new("score", (n_pos,), F32),
                 coord=case.new("coord", (n_pos, 2), I32), minmax=case.new("minmax", (n_pos, 2), F32),
                 mask=case.new("mask", (n_pos, h, w), U8))
        if n_labels > 0:
            o["labels"] = case.new("labels", (h, w), I32)
        scratch = case.scratch(L.olsr_lang_query_scratch_bytes(C.byref(p)))
        _check_rc(L.olsr_lang_query_relevancy(C.byref(p), sims.data_ptr(), o["relevancy"].data_ptr(), o["smoothed"].data_ptr(),
                                              o["blended"].data_ptr(), o["score"].data_ptr(), o["coord"].data_ptr(),
                                              o["minmax"].data_ptr(), o["mask"].data_ptr(), _p(o.get("labels")), scratch.data_ptr(),
                                              _stream()))
    out = three_ways(relevancy)
    hip_out = {k: v.cpu() for k, v in out.items()}
    hip_out["similarities"] = sims.cpu()
    _check_outputs(f"{w} x {h}", case_, hip_out, t64, t32)


# ------------------------------------------------------------------------------------------------ the general language encoder
# k_lang_encoder.hip: a tile of 64 rows per block: one row, one short of a tile, a tile, one row into the second.  No scratch.
@pytest.mark.parametrize("code_layout", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_lang_encoder_encode(hip, N, code_layout):
    """Yardstick: tests/lang_encoder_ref.py in float64 under _ratio_rule (tests/test_gpu_lang_encoder.py::
    test_sizes_in_both_layouts); the fused codes are olsr_lang_ae_encode's of the unit rows bit for bit
    (test_fused_codes_equal_the_codec)."""
    from test_gpu_lang_codec import _ratio_rule
    from test_gpu_lang_encoder import _codec, _encoder, _rows257
    L = _L()
    x, t64, t32 = _rows257()
    enc, codec = _encoder(), _codec(2)
    p = _abi.OlsrLangEncoderParams(n_widths=len(_abi.LANG_ENCODER_WIDTHS), in_layout=_abi.LANG_ENCODER_IN_ROWS, code_layout=code_layout,
                                   plane_stride=0, bn_eps=enc.eps)
    for k, v in enumerate(_abi.LANG_ENCODER_WIDTHS):
        p.widths[k] = v
    xd = x[:N].to(DEV).contiguous()
    code_shape = (N, 15) if code_layout == 0 else (15, N)

    def entry(case):
        f, c = case.new("features32", (N, 32), F32), case.new("codes", code_shape, F32)
        _check_rc(L.olsr_lang_encoder_encode(C.byref(p), N, xd.data_ptr(), enc.flat.data_ptr(), codec.flat.data_ptr(), f.data_ptr(),
                                             c.data_ptr(), _stream()))
    out = three_ways(entry, misaligned=False)
    _ratio_rule(f"N = {N} rows", out["features32"].cpu(), t64[:N], t32[:N])
    assert torch.equal(out["codes"], codec.encode(out["features32"], "rows" if code_layout == 0 else "channels"))


# ------------------------------------------------------------------------------------------------ the high-resolution feature net
# k_hr_net.hip: its two golden sizes (2 x 3 and 3 x 5 coarse pixels: no multiple of any tile).  The workspace is laid out by hand
# and must be 16-byte aligned (include/olsr.h): outer guards, no misaligned run.
def test_hr_net_forward(hip):
    """Yardstick: tests/hr_net_ref.py in float64 under _ratio_rule, and the golden file's 32 channels
    (tests/test_gpu_hr_net.py::test_golden)."""
    import hr_net_ref as R
    from test_gpu_hr_net import _net
    from test_gpu_lang_codec import _ratio_rule
    L = _L()
    z = R.golden()
    ch = [int(c) for c in z["channels"]]
    for key, (sizes, seed) in R.GOLDEN_CASES.items():
        state, inputs = R.make_case(key)
        net = _net(300 + seed)
        fv, f3, f2 = (t.to(DEV).contiguous() for t in inputs)
        h, w = sizes[0]
        n = 64 * h * w
        nbytes = int(L.olsr_hr_net_workspace_bytes(*(s_ for t in inputs for s_ in t.shape[1:])))
        p = _abi.OlsrHrNetParams(h=h, w=w, h3=f3.shape[1], w3=f3.shape[2], h2=f2.shape[1], w2=f2.shape[2], c_fv=768, c_f3=384, c_f2=192,
                                 c_out=768, launches=0, fv_stride=fv.stride(0), f3_stride=f3.stride(0), f2_stride=f2.stride(0), out_stride=n,
                                 bn_eps=net.eps, workspace_bytes=nbytes)

        def entry(case):
            out = case.new("out", (768, 8 * h, 8 * w), F32)
            work = case.scratch(nbytes, misalign_ok=False)
            _check_rc(L.olsr_hr_net_forward(C.byref(p), fv.data_ptr(), f3.data_ptr(), f2.data_ptr(), net.flat.data_ptr(), work.data_ptr(),
                                            out.data_ptr(), _stream()))
        out = three_ways(entry, misaligned=False)["out"].cpu()
        _ratio_rule(f"golden {key}, 32 channels", out[ch], torch.from_numpy(z[f"{key}_out_f64"]), torch.from_numpy(z[f"{key}_out_f32"]))
        _ratio_rule(f"golden {key}, all channels", out, R.forward(state, *inputs, torch.float64), R.forward(state, *inputs, torch.float32))


# ------------------------------------------------------------------------------------------------ TSDF fusion and extraction
# k_tsdf.hip: a voxel per thread, 256 per block; the extraction counts and prefixes per block of 256 voxels.  8 x 8 x 8 = 512
# voxels: two whole blocks; 9 x 7 x 5 = 315: one and a ragged one, odd extents.  Scratch: carved (the block counts and offsets;
# for the mesh the vertices' and the faces', then the voxel words).
@pytest.mark.parametrize("dim", [(8, 8, 8), (9, 7, 5)])
def test_tsdf(hip, dim):
    """olsr_tsdf_init + _integrate (five views in one launch), _surface_plan / _emit and _mesh_plan / _emit with capacities equal
    to the planned counts and one less: include/olsr.h promises every row below the capacity and nothing above, so every
    output is declared fully written.  Yardsticks: tests/tsdf_ref.py and tests/tsdf_mesh_ref.py, bit for bit
    (tests/test_gpu_tsdf.py's _assert_equals_reference and _assert_surface, tests/test_gpu_tsdf_mesh.py's _assert_mesh)."""
    import tsdf_mesh_ref as M
    import tsdf_ref as R
    from test_gpu_tsdf import IMAGES, VOXEL, _device_view, _reference, _views, _volume
    from test_gpu_tsdf_mesh import _equals_restatement
    L = _L()
    feature, (W, Hh) = 3, IMAGES[1]
    X, Y, Z = dim
    helper = _volume(dim, feature)   # (the geometry, and the views' structs)
    views = [helper._view("extents", **_device_view(v)) for v in _views(dim, W, Hh, feature)]
    arr = (_abi.OlsrTsdfView * len(views))(*[v for v, _ in views])
    ref, _ = _reference(dim, W, Hh, feature)
    t, w, f = ref.arrays()

    def volume(tsdf, weight, feat):
        v = _abi.OlsrTsdfVolume.from_buffer_copy(helper._vol)
        v.tsdf, v.weight, v.feat = tsdf.data_ptr(), weight.data_ptr(), feat.data_ptr()
        return v

    def fuse(case):
        tsdf, weight, feat = case.new("tsdf", dim, F32), case.new("weight", dim, F32), case.new("feat", (feature,) + dim, F32)
        vol = volume(tsdf, weight, feat)
        _check_rc(L.olsr_tsdf_init(C.byref(vol), _stream()))
        _check_rc(L.olsr_tsdf_integrate(C.byref(vol), len(views), arr, _stream()))
    fused = three_ways(fuse, misaligned=False)
    assert torch.equal(fused["weight"].cpu(), torch.from_numpy(w)) and torch.equal(fused["tsdf"].cpu(), torch.from_numpy(t))
    assert torch.equal(fused["feat"].cpu(), torch.from_numpy(f))
    assert int((w > 0).sum()) > 0

    vol = volume(fused["tsdf"], fused["weight"], fused["feat"])
    want = R.surface(t, w, f, helper.vol_origin, VOXEL, 0.0, False)
    n = len(want[2])
    assert n > 1
    for cap in (n, n - 1):
        def surface(case):
            scratch = case.scratch(L.olsr_tsdf_surface_scratch_bytes(X, Y, Z))
            status = case.new("status", (2,), I32)
            _check_rc(L.olsr_tsdf_surface_plan(C.byref(vol), 0.0, scratch.data_ptr(), status.data_ptr(), _stream()))
            pts, fe, idx = case.new("points", (cap, 3), F32), case.new("feats", (cap, feature), F32), case.new("index", (cap,), I32)
            _check_rc(L.olsr_tsdf_surface_emit(C.byref(vol), 0.0, scratch.data_ptr(), cap, pts.data_ptr(), fe.data_ptr(), idx.data_ptr(),
                                               _stream()))
        out = three_ways(surface)
        assert out["status"].tolist() == [n, 0]
        assert torch.equal(out["index"].cpu(), torch.from_numpy(want[2][:cap])), "order"
        assert torch.equal(out["points"].cpu(), torch.from_numpy(want[0][:cap])), "points"
        assert torch.equal(out["feats"].cpu(), torch.from_numpy(want[1][:cap])), "feats"

    mesh = M.mesh(t, w, f, helper.vol_origin, VOXEL, 0.0, False)
    nv, nf = len(mesh[0]), len(mesh[1])
    assert nv == n and nf > 1
    for cv, cf in ((nv, nf), (nv - 1, nf - 1)):
        def extract(case):
            scratch = case.scratch(L.olsr_tsdf_mesh_scratch_bytes(X, Y, Z))
            status = case.new("status", (4,), I32)
            _check_rc(L.olsr_tsdf_mesh_plan(C.byref(vol), 0.0, scratch.data_ptr(), status.data_ptr(), _stream()))
            o = dict(verts=case.new("verts", (cv, 3), F32), norms=case.new("norms", (cv, 3), F32), colors=case.new("colors", (cv, feature), F32),
                     index=case.new("index", (cv,), I32), faces=case.new("faces", (cf, 3), I32))
            _check_rc(L.olsr_tsdf_mesh_emit(C.byref(vol), 0.0, scratch.data_ptr(), cv, cf, o["verts"].data_ptr(), o["norms"].data_ptr(),
                                            o["colors"].data_ptr(), o["index"].data_ptr(), o["faces"].data_ptr(), _stream()))
        out = three_ways(extract)
        assert out["status"].tolist() == [nv, nf, 0, 0]
        assert torch.equal(out["faces"].cpu(), torch.from_numpy(mesh[1][:cf])), "faces"
        assert torch.equal(out["index"].cpu(), torch.from_numpy(want[2][:cv])), "vertex owners"
        assert _equals_restatement(out["verts"], mesh[0][:cv]) and _equals_restatement(out["norms"], mesh[2][:cv])
        assert _equals_restatement(out["colors"], mesh[3][:cv])


# ------------------------------------------------------------------------------------------------ map edits
# k_map_edit.hip: a source row per thread, 256 per block (the plan's segment counts are per block).  Scratch: carved
# (class bytes, block counts, block offsets).  The destination holds exactly P_new rows (dst_capacity = P_new): every word of it
# is written.
@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_map_edit(hip, P):
    """olsr_map_edit_plan + _apply in densify mode (clones, splits and drops).  Yardstick: MapSpec, the CPU specification, under
    tests/test_gpu_map_edit.py's compare (the map's state bit for bit, split children within 2^-20 of the row)."""
    from online_lang_splatting_amd.gaussian_map import GaussianMap
    from test_gpu_map_edit import FUSED_LRS, compare, random_map, spec_from_state
    L = _L()
    M, F = 1, 15
    st, z = random_map(P, M, F, seed=40 + P)
    spec = spec_from_state(st, DEV)
    want_src = spec.densify_and_prune(2e-4, 0.7, 1.0, 20, z=z.to(DEV))
    m = GaussianMap.from_state(st, FUSED_LRS, DEV)
    src = m._struct(m._bufs[m._front])
    ep = _abi.OlsrMapEditParams(mode=_abi.MAP_EDIT_DENSIFY, n_append=0, append_kf_id=0, screen_size_term=1, max_grad=2e-4,
                                min_opacity=0.7, clone_max_scale=m.percent_dense * 1.0, big_scale=0.1 * 1.0)
    zd = z.to(DEV).float().contiguous()
    width = 11 + 3 * M + F
    tails = dict(means3D=(3,), shs=(M, 3), opacities=(1,), scales=(3,), rotations=(4,), language=(F,), exp_avg=(width,),
                 exp_avg_sq=(width,), kf_id=(), n_obs=(), stats=(2,), max_radii=())

    def entry(case):
        scratch = case.scratch(L.olsr_map_edit_scratch_bytes(P))
        status = case.new("status", (8,), I32)
        _check_rc(L.olsr_map_edit_plan(P, C.byref(ep), C.byref(src), None, scratch.data_ptr(), status.data_ptr(), _stream()))
        torch.cuda.synchronize()
        n = int(status[0])
        d = {k: case.new(k, (n,) + tail, I32 if k in ("kf_id", "n_obs", "max_radii") else F32) for k, tail in tails.items()}
        src_index = case.new("src_index", (n,), I32)
        dst = m._struct(d)
        _check_rc(L.olsr_map_edit_apply(P, M, F, C.byref(ep), C.byref(src), zd.data_ptr(), None, scratch.data_ptr(), status.data_ptr(),
                                        n, n, C.byref(dst), _p(src_index), _stream()))
    out = three_ways(entry)
    n = int(out["status"][0])
    assert n == want_src.numel()
    got = GaussianMap.from_state(st, FUSED_LRS, DEV)   # the plain run's destination, installed as a map's front buffers
    back = 1 - got._front
    got._bufs[back] = dict({k: out[k] for k in tails}, cap=n)
    got._front, got.P = back, n
    got.status.copy_(out["status"])
    got._views()
    compare(got, spec.export(), out["src_index"], want_src, f"P={P}")


# ------------------------------------------------------------------------------------------------ keyframe seeding
# k_keyframe_seed.hip on the smallest golden image, 40 x 24 = 960 pixels, downsample 8: the staging holds exactly the
# (W H) / downsample = 120 rows the sample has, so every row is written.  Scratch: carved; the kNN scratch of
# olsr_keyframe_seed_finish is olsr_knn_mean_dist2's (Carver).
def test_keyframe_seed(hip):
    """olsr_keyframe_seed_plan + _finish.  Yardstick: tests/keyframe_seed_ref.py under tests/test_gpu_keyframe_seed.py's
    check_plan (bit for bit) and check_scales.  status int32[8]: only words 0 and 1 are specified (include/olsr.h)."""
    from test_gpu_keyframe_seed import SHAPES, W2C, _intrinsics, check_plan, check_scales, reference
    L = _L()
    W, Hh = SHAPES[0]
    Mm = 1
    image, depth, kw, ref = reference(W, Hh, Mm, False)
    img, dep, w2c = torch.from_numpy(image).to(DEV), torch.from_numpy(depth).to(DEV), torch.from_numpy(W2C).to(DEV).contiguous()
    fx, fy, cx, cy = _intrinsics(W, Hh)
    cap = W * Hh // kw["downsample"]
    assert ref["n_keep"] == cap
    p = _abi.OlsrKeyframeSeedParams(W=W, H=Hh, plane_stride=W * Hh, M=Mm, downsample=kw["downsample"], seed=kw["seed"], fx=fx, fy=fy,
                                    cx=cx, cy=cy, rgb_boundary_threshold=0.01, depth_trunc=100.0, point_size=0.05,
                                    adaptive_pointsize=1, capacity=cap)
    tails = dict(means3D=(3,), shs=(Mm, 3), opacities=(1,), scales=(3,), rotations=(4,))

    def entry(case):
        st = {k: case.new(k, (cap,) + tail, F32) for k, tail in tails.items()}
        pix = case.new("pix_index", (cap,), I32)
        rows = _abi.OlsrMapBuffers(**{k: st[k].data_ptr() for k in tails})
        scratch = case.scratch(L.olsr_keyframe_seed_scratch_bytes(W, Hh))
        status, aux = case.new("status", (8,), I32, written=False), case.new("aux", (4,), F32)
        _check_rc(L.olsr_keyframe_seed_plan(C.byref(p), img.data_ptr(), dep.data_ptr(), None, w2c.data_ptr(), C.byref(rows),
                                            pix.data_ptr(), scratch.data_ptr(), status.data_ptr(), aux.data_ptr(), _stream()))
        torch.cuda.synchronize()
        n_keep = int(status[1])
        knn = case.scratch(L.olsr_knn_scratch_bytes(n_keep))
        _check_rc(L.olsr_keyframe_seed_finish(C.byref(p), n_keep, C.byref(rows), aux.data_ptr(), scratch.data_ptr(), knn.data_ptr(),
                                              _stream()))
        case.out["status"] = status[:2]
    out = three_ways(entry)
    n_keep = int(out["status"][1])
    got = {k: out[k][:n_keep] for k in list(tails) + ["pix_index"]}
    got.update(n_valid=out["status"][0], median_depth=out["aux"][0], point_size=out["aux"][1], n_keep=n_keep)
    check_plan(got, ref, Mm)
    check_scales(got, ref)
    assert out["aux"][2:].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ the table's coverage
# tests/test_extents_cpu.py holds these two against include/olsr.h: every entry is in exactly one of them.
COVERED = (
    "olsr_forward", "olsr_backward", "olsr_forward_async", "olsr_debug_backward_ordered", "olsr_knn_mean_dist2", "olsr_mark_visible",
    "olsr_mask_smooth", "olsr_query_eval", "olsr_image_psnr", "olsr_accumulate_gradients", "olsr_bucket_add", "olsr_isotropic_reg",
    "olsr_adam_step", "olsr_adam_step_sum", "olsr_adam_step_masked", "olsr_adam_step_groups", "olsr_adam_step_groups_reg",
    "olsr_sparse_exchange_mask", "olsr_sparse_exchange_pack", "olsr_sparse_exchange_unpack", "olsr_grad_mask", "olsr_median_depth",
    "olsr_covisibility", "olsr_keyframe_decide", "olsr_mapping_loss", "olsr_tracking_loss", "olsr_refinement_loss", "olsr_emd_cost",
    "olsr_chamfer", "olsr_debug_activate", "olsr_pose_step", "olsr_pose_step_gated", "olsr_window_pose_step",
    "olsr_forward_async_loss", "olsr_lang_ae_train_step", "olsr_lang_ae_encode", "olsr_lang_ae_decode", "olsr_lang_query_sims",
    "olsr_lang_query_relevancy", "olsr_lang_encoder_encode", "olsr_hr_net_forward", "olsr_tsdf_init", "olsr_tsdf_integrate",
    "olsr_tsdf_surface_plan", "olsr_tsdf_surface_emit", "olsr_tsdf_mesh_plan", "olsr_tsdf_mesh_emit", "olsr_map_edit_plan",
    "olsr_map_edit_apply", "olsr_keyframe_seed_plan", "olsr_keyframe_seed_finish",
    # driven by the rows above, on the host: the row counts and knobs the rasteriser rows go through
    "olsr_last_forward_token", "olsr_live_rows", "olsr_backward_rows", "olsr_debug_sort_knobs", "olsr_debug_sort_small",
    "olsr_debug_sort_compact", "olsr_debug_sort_threads",
)
_HOST = "writes no device memory"
_SIZING = "a sizing function: tests/test_extents_cpu.py"
_OWN = "writes no memory of the caller's"
REASONS = (_HOST, _SIZING, _OWN)   # what a reason in NO_ROW starts with (tests/test_extents_cpu.py holds it to that)
NO_ROW = {
    **{n: _SIZING for n in (
        "olsr_geometry_bytes", "olsr_image_bytes", "olsr_binning_bytes", "olsr_backward_scratch_bytes", "olsr_isotropic_reg_scratch_bytes",
        "olsr_map_edit_scratch_bytes", "olsr_knn_scratch_bytes", "olsr_keyframe_seed_scratch_bytes", "olsr_frontend_scratch_bytes",
        "olsr_mapping_loss_scratch_bytes", "olsr_fused_loss_scratch_bytes", "olsr_refinement_loss_scratch_bytes",
        "olsr_lang_ae_scratch_bytes", "olsr_lang_query_scratch_bytes", "olsr_hr_net_workspace_bytes", "olsr_tsdf_surface_scratch_bytes",
        "olsr_tsdf_mesh_scratch_bytes", "olsr_emd_scratch_bytes", "olsr_chamfer_scratch_bytes", "olsr_query_eval_scratch_bytes",
        "olsr_image_psnr_scratch_bytes", "olsr_debug_backward_ordered_scratch_bytes", "olsr_sparse_exchange_scratch_ints")},
    **{n: _HOST for n in (
        "olsr_live_rows_wait", "olsr_live_rows_overwritten", "olsr_geometry_field", "olsr_binning_field", "olsr_image_field",
        "olsr_set_profiling", "olsr_get_stage_times", "olsr_debug_sort_plan", "olsr_debug_sort_status_room", "olsr_debug_sync_fault",
        "olsr_debug_rows_ratio", "olsr_debug_carve_log", "olsr_debug_carve_log_read", "olsr_last_error", "olsr_version")},
    "olsr_debug_sort_timing": _HOST + " itself: it registers a diagnostic buffer that later forwards fill by its own max_blocks x "
                              "max_launches bound; none is registered in any row",
    "olsr_debug_composite_stamps": _HOST + " itself: it registers a diagnostic buffer that later composites fill up to its own "
                                   "capacity; none is registered in any row",
    "olsr_debug_exp_sweep": _OWN + ": it allocates its four result words with hipMalloc and copies them to the host",
}
