"""The float sums of the per-Gaussian backward (csrc/k_preprocess_bwd.hip), each held to EQUALITY with the host model of its
summation order (tests/bwd_sums_ref.py) on the data the same call leaves readable.

Row sums: the composite's partial-gradient rows lie at the start of the workspace's caller-owned scratch; rowbase, inst_start,
tiles_touched, blended and counters are fields of its state buffers.  From those the model computes dL_dmeans2D, dL_dconic,
dL_dopacity, dL_dcolors, dL_dlanguage and dL_ddepths addition by addition - inline for up to OLSR_MID_FOOTPRINT tiles, a wave
per Gaussian above (row_reduce_big_kernel: persistent grid, two work lists, early exit, hand-written prefetch pipeline, one
multi-value butterfly per F) - and the kernel's tensors must hold the same bits.  The scene (tests/bwd_sums_scenes.py) is
built so that every path runs, and the test asserts that it did: footprints on both sides of both thresholds, both lists,
three trips of the pipeline, runs longer than a wave, listed Gaussians without a row between ones with rows.
(tests/test_bwd_sums_ref_cpu.py proves the same facts about the scene on the oracle, without a GPU.)

dL_dtau_sum: the fixed-order sum of the dL_dtau the call wrote (block partials, then tau_final_kernel), at every P where a
wave, a block or the final pass's stride of 256 partials begins or ends."""
import numpy as np
import pytest
import torch

import bwd_sums_ref as ref
import bwd_sums_scenes as bs
from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.scene import make_scene
from parity_common import COMPOSITE_KEYS, assert_tau_sum_fixed_order, first_difference, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _workspace(sc, capacity, tile=15, mode=_abi.BWD_REFERENCE, row_capacity=None):
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    dev = torch.device(DEV)
    cam = sc.camera
    ws = RasterWorkspace(sc.P, cam.width, cam.height, sc.F, sc.shs.shape[1], capacity, dev, tile=tile, bwd_mode=mode,
                         row_capacity=row_capacity, binning=_abi.BINNING_ELLIPSE)
    ws.set_scene(bg=sc.bg.to(dev), means3D=sc.means3D.to(dev), opacities=sc.opacities.to(dev), scales=sc.scales.to(dev),
                 rotations=sc.rotations.to(dev), shs=sc.shs.to(dev), language=sc.language.to(dev) if sc.F > 0 else None,
                 viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
                 projmatrix_raw=cam.projection_matrix.to(dev), campos=cam.camera_center.to(dev), tanfovx=cam.tanfovx,
                 tanfovy=cam.tanfovy, sh_degree=sc.sh_degree)
    return ws


def _state(hip, ws, R):
    """the fields the row sums read, as numpy: carved with the workspace's own sizes (its capacity is the R it carves with)"""
    P, F = ws.P, ws.F
    geo = lambda name, dtype, count: hip.state_field("geometry", ws.geom, name, P=P, F=F, dtype=dtype,  # noqa: E731
                                                     count=count).cpu().numpy()
    return dict(tiles_touched=geo("tiles_touched", torch.int32, P), inst_start=geo("inst_start", torch.int32, P),
                blended=geo("blended", torch.uint8, P), conic_opacity=geo("conic_opacity", torch.float32, 4 * P).reshape(P, 4),
                rowbase=hip.state_field("binning", ws.binning, "rowbase", R=ws.capacity, F=F, dtype=torch.int32,
                                        count=R + 1).cpu().numpy())


ROW_CASES = [(0, 15, _abi.BWD_REFERENCE, True), (3, 15, _abi.BWD_REFERENCE, True), (15, 15, _abi.BWD_REFERENCE, True),
             (16, 15, _abi.BWD_REFERENCE, True), (32, 15, _abi.BWD_REFERENCE, True), (15, 16, _abi.BWD_EXACT, True),
             (15, 15, _abi.BWD_REFERENCE, False)]


@pytest.mark.parametrize("F,tile,mode,lang_cotangent", ROW_CASES,
                         ids=[f"F{c[0]}_t{c[1]}_{'ref' if c[2] == _abi.BWD_REFERENCE else 'exact'}{'' if c[3] else '_nolang'}"
                              for c in ROW_CASES])
def test_row_sums_equal_the_model(hip, F, tile, mode, lang_cotangent):
    from online_lang_splatting_amd.frame_shard import GradLayout, GradientBucket
    dev = torch.device(DEV)
    sc = bs.make(F)
    P = sc.P
    capacity = 150_000   # (tests/test_bwd_sums_ref_cpu.py: the lists hold fewer than that whatever the kernel decides)
    ws = _workspace(sc, capacity, tile, mode, row_capacity=4 * capacity)
    bucket = GradientBucket(P, GradLayout(sc.shs.shape[1], F), dev)
    dc, dl, dd = [None if t is None else t.to(dev).contiguous() for t in sc.cotangents(3)]
    if not lang_cotangent:
        dl = None
    F_rows = F if dl is not None else 0
    ROW = ref.grad_row(F_rows)
    ws.forward()
    g = ws.backward(dc, dl, dd, bucket=bucket, first=True)
    torch.cuda.synchronize()
    R, overflow = ws.rendered()
    live, row_overflow = ws.backward_status()
    assert 0 < R <= capacity and not overflow and live > 0 and not row_overflow
    cnt = hip.state_field("geometry", ws.geom, "counters", P=P, F=F, dtype=torch.int32, count=16).cpu().numpy()
    assert cnt[0] == R and cnt[6] == live and cnt[7] == 0 and cnt[8] == 0 and cnt[9] == 0
    st = _state(hip, ws, R)
    radii = ws.out["radii"].cpu().numpy()
    rows = ws.scratch[: 4 * live * ROW].view(torch.float32).cpu().numpy()
    m = ref.composite_level(rows, ROW, F_rows, F, P, radii, st["blended"], st["tiles_touched"], st["inst_start"],
                            st["rowbase"], activations=0, conic_opacity=st["conic_opacity"][radii > 0])

    # ---- the frame is the one the test is about (else it would pass vacuously) ------------------------------------------
    tt, has, nrows = st["tiles_touched"].astype(np.int64), m["has_rows"], m["nrows"]
    listed = tt > ref.MID_FOOTPRINT
    nwaves = ref.rr_nwaves(P)
    n_big, n_mid = int(cnt[5]), int(cnt[4])
    count = n_big + n_mid
    trips = -(-count // nwaves)
    with_rows = {k: int((has & (tt == k)).sum()) for k in bs.TILE_COUNTS}
    flips = int((np.diff(has[listed].astype(np.int8)) != 0).sum())
    print(f"F={F} tile={tile} mode={mode} F_rows={F_rows}: P={P} R={R} live rows={live} listed={count} (big {n_big}, mid {n_mid}) "
          f"nwaves={nwaves} trips={trips} largest run={int(nrows.max())} listed without rows={int((listed & ~has).sum())} "
          f"has_rows flips along the listed={flips} with rows at {with_rows}")
    assert all(v > 0 for v in with_rows.values()), with_rows
    assert n_big > 0 and n_mid > 0
    assert n_big == int((tt > ref.BIG_FOOTPRINT).sum()) and n_mid == int((listed & (tt <= ref.BIG_FOOTPRINT)).sum())
    assert count >= 2 * nwaves + 1 and trips == 3
    assert int(nrows[listed].max()) > 64 and bool((nrows[listed & has] % 64 != 0).any())
    assert int((listed & ~has).sum()) >= 50
    assert flips >= 100, "the listed Gaussians without rows are not interleaved with ones that have rows"
    assert int(nrows.sum()) == live, "the runs of the Gaussians with rows are not all the live rows"

    # ---- the six composite-level tensors, bit for bit ---------------------------------------------------------------------
    unequal = []
    for k in COMPOSITE_KEYS:
        want = torch.from_numpy(m[k])
        assert g[k].numel() == want.numel(), k
        d = first_difference(g[k], want)
        if d is not None:
            unequal.append(f"{k}: {d[3]} of {want.numel()} elements differ, first at flat index {d[0]}: {d[1]!r}, model {d[2]!r}")
    assert not unequal, "; ".join(unequal)
    assert float(g["dL_dmeans2D"].abs().max()) > 0 and (F_rows == 0 or float(g["dL_dlanguage"].abs().max()) > 0)
    # the densification statistic of the view (assigned: first=True) is the norm of the summed screen-space gradient
    nrm = ref.densify_norm(m["dL_dmeans2D"][:, 0], m["dL_dmeans2D"][:, 1], radii)
    assert same_bits(bucket.densify[:, 0], torch.from_numpy(nrm)), first_difference(bucket.densify[:, 0], torch.from_numpy(nrm))
    assert_tau_sum_fixed_order(g)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 127, 128, 129, 32768, 32769, 65613])
def test_tau_sum_equals_the_model(hip, P):
    """P around a wave (64), a block (128: one partial) and the final pass's stride (256 partials = 32768 Gaussians);
    65613 = 512 partials and a tail block of 77."""
    dev = torch.device(DEV)
    sc = make_scene(P, 160, 120, 3, seed=700 + P % 101)
    sc.opacities.mul_(0.05)   # nothing saturates: every Gaussian some pixel sees has a pose gradient, the tail block's too
    ws = _workspace(sc, 600_000)
    dc, dl, dd = [t.to(dev).contiguous() for t in sc.cotangents(4)]
    ws.forward()
    g = {k: v.clone() for k, v in ws.backward(dc, dl, dd).items()}
    torch.cuda.synchronize()
    assert not ws.rendered()[1] and not ws.backward_status()[1]
    nz = int((g["dL_dtau"] != 0).any(dim=1).sum())
    print(f"P={P}: {ws.rendered()[0]} instances, {nz} Gaussians with a pose gradient, partials={(P + 127) // 128} "
          f"depth d={ref.tau_sum_depth(P)} dL_dtau_sum={g['dL_dtau_sum'].tolist()}")
    assert P < 63 or nz > P // 4, "too few terms: the sum says little"
    assert_tau_sum_fixed_order(g, where=f"P={P}: ")
    # tracking's form: only dL_dtau_sum is produced, no per-Gaussian array is written
    tracked = torch.full((6,), float("nan"), device=dev)
    ws.backward(dc, dl, dd, pose_only=True, tau_sum_out=tracked)
    torch.cuda.synchronize()
    assert_tau_sum_fixed_order(dict(dL_dtau=g["dL_dtau"], dL_dtau_sum=tracked), where=f"P={P}, pose_only: ")
