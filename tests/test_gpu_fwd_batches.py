"""The forward composite (k_render_fwd.hip) at its structural edges: the scenes of tests/fwd_batch_scenes.py put every wave's
stop entry on both sides of the 128-entry staging batches and on both halves of the two-entry iterations, entries that reach
no pixel next to entries that do, an entry its wave would blend right behind that wave's stop entry, waves without a pixel
inside the image, and lists no pixel ever leaves (tests/test_fwd_batch_scenes_cpu.py proves the scenes are what they claim).

Default accumulation, both binnings, every case: images, final_T, n_contrib, radii, n_touched and num_rendered equal the
oracle's bit for bit (n_contrib is a list position: under the exact lists it is the oracle's mapped through the entries that
binning kept), and the liveness the backward trusts - flags[], tile_work[2][tiles], blended[P], olsr_live_rows -
equals what the oracle's record of who blended what says (fwd_batch_scenes.expected_*): an independent truth, not the
product's other binning.

OLSR_FLAG_FWD_ACCUM_MFMA / _WEIGHT: every decision output is bit-identical to the default run; the images are within
test_gpu_mfma.IMG_TOL of the oracle and, where the features are non-negative (depth; colour over a zero background), within
2 (1 + n_contrib) 2^-24 of the oracle's value PER PIXEL: there the accumulated value is its own condition, and the two
roundings differ by one rounding of each product and one of each partial sum - a derived bound, under which a wrong dim pixel
cannot hide.  The two variants agree bit for bit (the MFMA is a k-ordered fma chain, a weight of 0 leaves a finite accumulator
unchanged), so do the two binnings, and tests/golden/fwd_batches.npz pins the bits per case
(tests/golden/make_golden_fwd_batches.py).

CUT (RasterWorkspace(depth_cut=True)): the first frame is the plain frame bit for bit, reports no miss, and every tile leaves
fl32(fl32(1.1f depth[stop]) + 0.01f) for the entry at which its last pixel terminated - +inf when a pixel never did; a second
frame of the view, now with cut-offs in force, is again the plain frame.

The fused loss epilogues (forward_loss) on the lists that saturate per wave, and the backward on them, are held to the
yardsticks of tests/test_gpu_loss.py and tests/test_gpu_bwd_batches.py.
"""
import os

import numpy as np
import pytest
import torch

import fwd_batch_scenes as fs
from online_lang_splatting_amd import _abi
from parity_common import assert_backward_criteria, rel_err, run_backend, run_forward, same_bits, tile_pairs
from test_gpu_loss import FUSED_EXPOSURE_ATOL, _close
from test_gpu_mfma import IMG_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_batches.npz")
EPS = 2.0 ** -24
BINNINGS = (("rect", _abi.BINNING_RECT), ("ellipse", _abi.BINNING_ELLIPSE))
CNT_RECT_INSTANCES, CNT_CUT_MISS = 3, 9   # csrc/olsr_state.h


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {str(i): d for i, d in zip(z["ids"], z["sha256"])}


def _oracle_forward(oracle, sc, tile):
    """The oracle's forward with its record of who blended what, and the liveness that record implies."""
    oracle.lib().oracle_set_record(1)
    try:
        fo, _ = run_forward(oracle, sc, None, tile)
    finally:
        oracle.lib().oracle_set_record(0)
    g = fo["geom"]
    W, H = sc.camera.width, sc.camera.height
    rec = dict(final_T=oracle.get_field(g, "final_T"), n_contrib=oracle.get_field(g, "n_contrib"),
               point_list=oracle.get_field(g, "point_list"), ranges=oracle.get_field(g, "ranges").view(-1, 2),
               flags=fs.expected_flags(oracle.get_field(g, "contrib_mask"), tile))
    rec["tile_work"] = fs.expected_tile_work(rec["flags"], rec["ranges"])
    rec["blended"] = fs.expected_blended(rec["flags"], rec["point_list"], sc.P)
    rec["nc_image"] = rec["n_contrib"].view(H, W)
    oracle.release(g)
    return fo, rec


def _decisions(hip, f, sc, tile):
    """Everything the forward decides, from a drop-in forward's state (CPU tensors)."""
    W, H, P, F, R = sc.camera.width, sc.camera.height, sc.P, sc.F, f["R"]
    hip.TILE = tile
    nt = ((W + tile - 1) // tile) * ((H + tile - 1) // tile)
    d = dict(R=R, radii=f["radii"].cpu(), n_touched=f["n_touched"].cpu(), opacity=f["opacity"].cpu(),
             final_T=hip.state_field("image", f["img"], "final_T", W=W, H=H, dtype=torch.float32, count=W * H).cpu(),
             n_contrib=hip.state_field("image", f["img"], "n_contrib", W=W, H=H, dtype=torch.int32, count=W * H).cpu(),
             tile_work=hip.state_field("image", f["img"], "tile_work", W=W, H=H, dtype=torch.int32, count=2 * nt).cpu().view(2, nt).long(),
             blended=hip.state_field("geometry", f["geom"], "blended", P=P, F=F, dtype=torch.uint8, count=P).cpu(),
             rect_instances=int(hip.state_field("geometry", f["geom"], "counters", P=P, F=F, dtype=torch.int32, count=8).cpu()[CNT_RECT_INSTANCES]))
    if R > 0:
        keys, flags, pos = tile_pairs(hip, f, sc, tile)
        d.update(keys=keys.cpu(), flags=flags.cpu(), pos=pos.cpu())
    else:
        d.update(keys=torch.zeros(0, dtype=torch.int64), flags=torch.zeros(0, dtype=torch.uint8), pos=torch.zeros(0, dtype=torch.int64))
    return d


DECISION_KEYS = ("R", "radii", "n_touched", "opacity", "final_T", "n_contrib", "tile_work", "blended", "rect_instances", "keys",
                 "flags")


def _assert_same_decisions(a, b, where):
    for k in DECISION_KEYS:
        same = (a[k] == b[k]) if not torch.is_tensor(a[k]) else (a[k].shape == b[k].shape and torch.equal(a[k], b[k]))
        assert same, f"{where}: {k} differs"


def _live_rows(hip):
    """olsr_live_rows of the forward this thread issued last, for both packings (after a synchronisation)"""
    from online_lang_splatting_amd._lib import lib
    tok = hip.last_forward_token()
    torch.cuda.synchronize()
    return lib().olsr_live_rows(tok, 0), lib().olsr_live_rows(tok, 1)


def _assert_decisions_equal_oracle(d, fo, rec, sc, tile, where):
    """d: {"rect": decisions, "ellipse": decisions} of the default accumulation"""
    for name, x in d.items():
        assert torch.equal(x["radii"], fo["radii"]) and torch.equal(x["n_touched"], fo["n_touched"]), f"{where}:{name}"
        assert torch.equal(x["final_T"], rec["final_T"]), f"{where}:{name}: final_T"
        assert x["rect_instances"] == fo["R"], f"{where}:{name}: the reference's num_rendered"
        assert torch.equal(x["tile_work"], rec["tile_work"]), f"{where}:{name}: tile_work {x['tile_work'].tolist()} != {rec['tile_work'].tolist()}"
        assert torch.equal(x["blended"], rec["blended"]), f"{where}:{name}: blended"
        # olsr_live_rows: the frame's row counts are the sums of tile_work, per packing (tests/test_gpu_api.py: test_live_row_counts_*)
        assert x["live_rows"] == (int(rec["tile_work"][0].sum()), int(rec["tile_work"][1].sum())), f"{where}:{name}: live rows {x['live_rows']}"
    r, e = d["rect"], d["ellipse"]
    assert r["R"] == fo["R"] and e["R"] <= fo["R"], where
    # the reference's lists: position for position the oracle's
    want = rec["flags"][r["pos"]]
    P = max(int(fo["radii"].numel()), 1)
    assert torch.equal(r["keys"] % P, rec["point_list"].long()[r["pos"]]), f"{where}: point_list"
    bad = (r["flags"] != want).nonzero().flatten()
    assert bad.numel() == 0, (f"{where}: rect flags differ from the oracle's record at {bad.numel()} entries, first at list position "
                              f"{int(r['pos'][bad[0]])}: {int(r['flags'][bad[0]]):#x} != {int(want[bad[0]]):#x}")
    # the exact lists: an order-preserving sub-list that keeps every blending entry
    keep = torch.isin(r["keys"], e["keys"])
    assert int(keep.sum()) == e["keys"].numel() and torch.equal(r["keys"][keep], e["keys"]), f"{where}: exact lists"
    assert torch.equal(e["flags"], want[keep]), f"{where}: ellipse flags"
    assert int((want[~keep] != 0).sum()) == 0, f"{where}: the exact binning dropped an entry that blends"
    # n_contrib counts list positions: the oracle's under the reference's lists; under the exact lists the number of entries
    # that binning kept among the oracle's first n_contrib positions of the pixel's tile
    assert torch.equal(r["n_contrib"], rec["n_contrib"]), f"{where}:rect: n_contrib"
    W, H = sc.camera.width, sc.camera.height
    gx = (W + tile - 1) // tile
    want_nc = rec["nc_image"].clone()
    tile_of = r["keys"] // P
    for t in range(rec["ranges"].shape[0]):
        kept = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(keep[tile_of == t].long(), 0)])
        ys, xs = slice((t // gx) * tile, (t // gx + 1) * tile), slice((t % gx) * tile, (t % gx + 1) * tile)
        want_nc[ys, xs] = kept[rec["nc_image"][ys, xs].long()].to(want_nc.dtype)
    assert torch.equal(e["n_contrib"].view(H, W), want_nc), f"{where}:ellipse: n_contrib"


def _assert_images_equal(f, fo, where):
    for k in fs.IMAGE_KEYS:
        if fo[k] is not None and fo[k].numel():
            assert torch.equal(f[k].cpu(), fo[k]), f"{where}: forward {k} differs from the oracle (rel {rel_err(f[k], fo[k])[0]:.2e})"


@pytest.mark.parametrize("F", fs.F_DEFAULT)
@pytest.mark.parametrize("tile", fs.TILES)
def test_default_accumulation_and_its_liveness_equal_the_oracle(hip, oracle, tile, F):
    dev = torch.device(DEV)
    n = 0
    for case in fs.cases(tile):
        cid = fs.case_id(tile, F, case)
        sc, _ = fs.make(case, tile, F)
        fo, rec = _oracle_forward(oracle, sc, tile)
        d = {}
        for name, binning in BINNINGS:
            f, _ = run_forward(hip, sc, dev, tile, 0, binning)
            live = _live_rows(hip)
            _assert_images_equal(f, fo, f"{cid}:{name}")
            d[name] = _decisions(hip, f, sc, tile)
            d[name]["live_rows"] = live
        _assert_decisions_equal_oracle(d, fo, rec, sc, tile, cid)
        n += 1
    print(f"default accumulation: {n} cases")


def _variant_forward(hip, sc, dev, tile, flag, binning):
    hip.FLAGS = flag
    try:
        f, _ = run_forward(hip, sc, dev, tile, 0, binning)
    finally:
        hip.FLAGS = 0
    return f


@pytest.mark.parametrize("F", fs.F_OTHER)
@pytest.mark.parametrize("tile", fs.TILES)
def test_accumulation_variants(hip, oracle, golden, tile, F):
    dev = torch.device(DEV)
    worst, n = 0.0, 0
    for case in fs.cases(tile):
        cid = fs.case_id(tile, F, case)
        sc, _ = fs.make(case, tile, F)
        fo, rec = _oracle_forward(oracle, sc, tile)
        base = {}
        for name, binning in BINNINGS:
            f, _ = run_forward(hip, sc, dev, tile, 0, binning)
            base[name] = _decisions(hip, f, sc, tile)
        bounded = ["depth"] + (["color"] if float(sc.bg.abs().max()) == 0.0 else [])
        images = {}
        for vname, flag in fs.ACCUM_VARIANTS:
            for name, binning in BINNINGS:
                where = f"{cid}:{vname}:{name}"
                fv = _variant_forward(hip, sc, dev, tile, flag, binning)
                _assert_same_decisions(_decisions(hip, fv, sc, tile), base[name], where)
                for k in ("color", "language", "depth"):
                    if fo[k] is not None and fo[k].numel():
                        r, _ = rel_err(fv[k], fo[k])
                        assert r <= IMG_TOL, f"{where}: {k}: {r:.2e} of the image's range"
                for k in bounded:
                    v, o = fv[k].detach().double().cpu(), fo[k].double()
                    bound = 2.0 * (1.0 + rec["nc_image"].double()) * EPS * o     # [H, W] broadcasts over the channels
                    err = (v - o).abs()
                    assert bool((o >= 0).all())
                    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
                    worst = max(worst, ratio)
                    assert bool((err <= bound).all()), f"{where}: {k}: a pixel is {ratio:.2f} x the bound 2 (1 + n_contrib) 2^-24 |oracle|"
                images[vname, name] = {k: (None if fv[k] is None else fv[k].cpu()) for k in fs.IMAGE_KEYS}
            for k in fs.IMAGE_KEYS:
                if images[vname, "rect"][k] is not None:
                    assert same_bits(images[vname, "rect"][k], images[vname, "ellipse"][k]), f"{cid}:{vname}: {k} depends on the binning"
            assert np.array_equal(fs.digest(images[vname, "ellipse"]), golden[fs.case_id(tile, F, case, vname)]), \
                f"{cid}:{vname}: images differ in bits from the recorded build"
        for k in fs.IMAGE_KEYS:
            a, b = images["mfma", "ellipse"][k], images["weight", "ellipse"][k]
            if a is not None and bool(torch.isfinite(a).all()):
                assert same_bits(a, b), f"{cid}: {k}: the MFMA and the weight accumulation differ in bits"
        n += 1
    print(f"accumulation variants: {n} cases each, largest |variant - oracle| / (2 (1 + n_contrib) 2^-24 |oracle|) = {worst:.3f}")


def _on_device(sc, dev):
    g = dict(bg=sc.bg.to(dev), means3D=sc.means3D.to(dev), opacities=sc.opacities.to(dev), scales=sc.scales.to(dev),
             rotations=sc.rotations.to(dev), shs=sc.shs.to(dev), language=None if sc.F == 0 else sc.language.to(dev))
    cam = sc.camera
    c = dict(viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
             projmatrix_raw=cam.projection_matrix.to(dev), campos=cam.camera_center.to(dev), tanfovx=cam.tanfovx,
             tanfovy=cam.tanfovy)
    return g, c


def _workspace(sc, tile, capacity, dev, **kw):
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    ws = RasterWorkspace(sc.P, sc.camera.width, sc.camera.height, sc.F, sc.shs.shape[1], capacity, dev, tile=tile, **kw)
    g, c = _on_device(sc, dev)
    ws.set_scene(sh_degree=sc.sh_degree, **c, **g)
    return ws


def _ws_decisions(hip, ws, tile):
    """The decisions a workspace's last forward left (CPU tensors); the lists in sorted order."""
    W, H, P, F = ws.W, ws.H, ws.P, ws.F
    hip.TILE = tile
    nt = ((W + tile - 1) // tile) * ((H + tile - 1) // tile)
    R = ws.rendered()[0]
    d = dict(R=R, radii=ws.out["radii"].cpu(), n_touched=ws.out["n_touched"].cpu(),
             final_T=hip.state_field("image", ws.img, "final_T", W=W, H=H, dtype=torch.float32, count=W * H).cpu(),
             n_contrib=hip.state_field("image", ws.img, "n_contrib", W=W, H=H, dtype=torch.int32, count=W * H).cpu(),
             tile_work=hip.state_field("image", ws.img, "tile_work", W=W, H=H, dtype=torch.int32, count=2 * nt).cpu(),
             ranges=hip.state_field("image", ws.img, "ranges", W=W, H=H, dtype=torch.int32, count=2 * nt).cpu(),
             blended=hip.state_field("geometry", ws.geom, "blended", P=P, F=F, dtype=torch.uint8, count=P).cpu())
    if R > 0:
        src = hip.state_field("binning", ws.binning, "src", R=ws.capacity, F=F, dtype=torch.int32, count=R).long()
        gid = hip.state_field("binning", ws.binning, "inst_gid", R=ws.capacity, F=F, dtype=torch.int32, count=R)
        fl = hip.state_field("binning", ws.binning, "flags", R=ws.capacity, F=F, dtype=torch.uint8, count=R)
        d.update(point_list=gid[src].cpu(), flags=fl[src].cpu())
    return d


def _assert_same_ws_decisions(a, b, where, keys=None):
    for k in (keys or a.keys()):
        same = (a[k] == b[k]) if not torch.is_tensor(a[k]) else (a[k].shape == b[k].shape and torch.equal(a[k], b[k]))
        assert same, f"{where}: {k} differs"


def _expected_raw_cut(case, sc, rec, tile, depths):
    """Per tile: fl32(fl32(1.1f depth[stop]) + 0.01f) for the entry at which the tile's last pixel terminated, +inf when a pixel
    inside the image never did, None where this test has no independent truth.
    stop / edge: every wall reaches every pixel of these images with alpha far above 1/255 (sigma 12 px, opacity 0.999), so a
    pixel whose n_contrib lies in front of the last wall of its tile's list terminated at the wall at list position n_contrib,
    and a pixel that blended the last wall never terminated (nothing behind the walls can saturate anything).
    skips / plain: nothing saturates anywhere.  never: the far corner of tile (0, 0) never terminates; the other tiles see the
    narrow walls at alphas around 1/255 and are left out.  after: five walls saturate quadrant 0 of tile (0, 0) only."""
    W, H = sc.camera.width, sc.camera.height
    gx, gy = (W + tile - 1) // tile, (H + tile - 1) // tile
    inf = float("inf")
    if case.family in ("skips", "plain"):
        return [inf] * (gx * gy)
    if case.family in ("never", "after"):
        return [inf] + [None] * (gx * gy - 1)
    out = []
    pl = rec["point_list"].long()
    for t in range(gx * gy):
        bx, by = t % gx, t // gx
        r0, r1 = int(rec["ranges"][t, 0]), int(rec["ranges"][t, 1])
        gids = pl[r0:r1]
        is_wall = (gids >= case.s) & (gids < case.s + case.n_walls)
        if not bool(is_wall.any()):
            out.append(inf)
            continue
        end = int(is_wall.nonzero().max()) + 1
        nc = rec["nc_image"][by * tile:(by + 1) * tile, bx * tile:(bx + 1) * tile]
        if bool((nc < end).all()):
            d = depths[int(gids[int(nc.max())])]
            out.append(float((d * torch.tensor(1.1, dtype=torch.float32)) + torch.tensor(0.01, dtype=torch.float32)))
        else:
            out.append(inf)
    return out


@pytest.mark.parametrize("F", fs.F_OTHER)
@pytest.mark.parametrize("tile", fs.TILES)
def test_depth_cut_instantiation(hip, oracle, tile, F):
    dev = torch.device(DEV)
    n, finite_first, finite_last = 0, 0, 0
    for case in fs.cases(tile):
        cid = fs.case_id(tile, F, case, "cut")
        sc, _ = fs.make(case, tile, F)
        fo, rec = _oracle_forward(oracle, sc, tile)
        W, H = sc.camera.width, sc.camera.height
        nt = ((W + tile - 1) // tile) * ((H + tile - 1) // tile)
        plain = _workspace(sc, tile, fo["R"] + 16, dev)
        cut = _workspace(sc, tile, fo["R"] + 16, dev, depth_cut=True)
        out_p = {k: v.clone() for k, v in plain.forward().items()}
        dp = _ws_decisions(hip, plain, tile)
        _assert_images_equal(out_p, fo, f"{cid}:plain")     # (the plain workspace renders the oracle's frame)
        assert bool(torch.isinf(cut.depth_cut).all())
        out_c = {k: v.clone() for k, v in cut.forward().items()}
        assert cut.forward_status() == 0, cid
        dc = _ws_decisions(hip, cut, tile)
        cnt = hip.state_field("geometry", cut.geom, "counters", P=sc.P, F=F, dtype=torch.int32, count=16).cpu()
        assert int(cnt[CNT_CUT_MISS]) == 0, cid
        for k in out_p:
            assert torch.equal(out_c[k], out_p[k]), f"{cid}: {k}"
        _assert_same_ws_decisions(dc, dp, cid)
        # the raw cut-off every tile leaves (the second half of the array; the dilation only reads it)
        depths = hip.state_field("geometry", cut.geom, "depths", P=sc.P, F=F, dtype=torch.float32, count=sc.P).cpu()
        raw = cut._depth_cut_buf[nt:].cpu()
        want = _expected_raw_cut(case, sc, rec, tile, depths)
        for t, w in enumerate(want):
            if w is not None:
                assert float(raw[t]) == w, f"{cid}: tile {t} left the cut-off {float(raw[t])!r}, expected {w!r}"
        if case.family in ("stop", "edge"):
            assert want[0] != float("inf"), cid
            stop = int(rec["nc_image"][:tile, :tile].max())
            finite_first += stop % 128 == 0
            finite_last += stop % 128 == 127
        # a second frame of the view, with the cut-offs the first one left now in force
        out_2 = {k: v.clone() for k, v in cut.forward().items()}
        assert cut.forward_status() == 0, cid
        d2 = _ws_decisions(hip, cut, tile)
        cnt = hip.state_field("geometry", cut.geom, "counters", P=sc.P, F=F, dtype=torch.int32, count=16).cpu()
        assert int(cnt[CNT_CUT_MISS]) == 0, cid
        for k in out_p:
            assert torch.equal(out_2[k], out_p[k]), f"{cid}: second frame: {k}"
        _assert_same_ws_decisions(d2, dp, f"{cid}: second frame", keys=("radii", "n_touched", "final_T", "n_contrib"))
        assert d2["R"] <= dp["R"]
        n += 1
    # the tile's stop entry was the first and the last entry of the batch staged last
    assert finite_first > 0 and finite_last > 0, (finite_first, finite_last)
    print(f"depth cut-offs: {n} cases")


def _targets(sc, seed, dev):
    W, H, F = sc.camera.width, sc.camera.height, sc.F
    gen = torch.Generator().manual_seed(seed)
    gt_image = torch.rand(3, H, W, generator=gen)
    gt_image[:, : H // 3] *= 0.001                       # below the rgb boundary threshold
    gt_depth = torch.rand(H, W, generator=gen) * 5
    gt_depth[:, : W // 4] = 0.0                          # invalid depth
    gt_lang = torch.nn.functional.normalize(torch.randn(max(F, 1), 5, 7, generator=gen), dim=0)[:F] if F else None
    grad_mask = (torch.rand(H, W, generator=gen) > 0.3).float()
    exposure = torch.tensor([0.11, -0.03])
    mv = lambda t: None if t is None else t.to(dev).contiguous()   # noqa: E731
    return mv(gt_image), mv(gt_depth), mv(gt_lang), mv(grad_mask), mv(exposure)


def _assert_fused_equals_two_kernels(fu, two, lang, where):
    assert torch.equal(fu["dL_dimage"], two["dL_dimage"]) and torch.equal(fu["dL_ddepth"], two["dL_ddepth"]), where
    if lang:
        assert torch.equal(fu["dL_dlanguage"], two["dL_dlanguage"]), where
    else:
        assert fu["dL_dlanguage"] is None, where
    _close(fu["loss"], two["loss"], f"{where}: loss")
    assert float((fu["dL_dexposure"] - two["dL_dexposure"]).abs().max()) <= FUSED_EXPOSURE_ATOL, where


@pytest.mark.parametrize("F", [0, 15])
@pytest.mark.parametrize("tile", fs.TILES)
def test_fused_loss_epilogues_on_lists_that_saturate_per_wave(hip, tile, F):
    from online_lang_splatting_amd import losses
    dev = torch.device(DEV)
    n = 0
    for ci, case in enumerate(fs.cases(tile, ("stop", "never", "after", "edge"))):
        cid = fs.case_id(tile, F, case, "loss")
        sc, kind = fs.make(case, tile, F)
        ws = _workspace(sc, tile, 4 * len(kind) + 16, dev)
        gt_image, gt_depth, gt_lang, grad_mask, exposure = _targets(sc, 100 + ci, dev)
        img = {k: v.clone() for k, v in ws.forward().items()}
        plain = _ws_decisions(hip, ws, tile)
        # the mapping loss
        two = losses.mapping_loss(img["color"], img["depth"], img["language"] if F else None, gt_image, gt_depth, gt_lang, exposure)
        two = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in two.items()}
        for skip in (False, True):
            fu = ws.forward_loss(gt_image, gt_depth, gt_lang, exposure, skip_images=skip)
            torch.cuda.synchronize()
            _assert_fused_equals_two_kernels(fu, two, F > 0, f"{cid}: mapping, skip_images={skip}")
        # the tracking loss, with and without a mask
        for gm in (grad_mask, None):
            two = losses.tracking_loss(img["color"], img["depth"], img["opacity"], gt_image, gt_depth, gm, exposure)
            two = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in two.items()}
            for skip in (False, True):
                where = f"{cid}: tracking, mask={gm is not None}, skip_images={skip}"
                fu = ws.forward_loss(gt_image, gt_depth, None, exposure, gm, tracking=True, skip_images=skip)
                torch.cuda.synchronize()
                _assert_fused_equals_two_kernels(fu, two, False, where)
                if skip and F == 15:
                    # launch_fwd_f: the F = 0 instantiation on the language scene's state makes the same decisions
                    _assert_same_ws_decisions(_ws_decisions(hip, ws, tile), plain, where,
                                              keys=("n_contrib", "final_T", "n_touched", "flags", "tile_work"))
        n += 1
    print(f"fused loss epilogues: {n} cases")


@pytest.mark.parametrize("F", [0, 15])
@pytest.mark.parametrize("mode", [_abi.BWD_REFERENCE, _abi.BWD_EXACT])
@pytest.mark.parametrize("tile", fs.TILES)
def test_backward_on_lists_that_saturate_per_wave(hip, oracle, tile, mode, F):
    dev = torch.device(DEV)
    n = 0
    for case in fs.cases(tile, ("stop", "never", "after")):
        cid = fs.case_id(tile, F, case, f"m{mode}")
        sc, _ = fs.make(case, tile, F)
        seed = case.s + case.tail
        fo, go = run_backend(oracle, sc, None, seed, tile, mode)
        fg, gg = run_backend(hip, sc, dev, seed, tile, mode)
        torch.cuda.synchronize()
        _assert_images_equal(fg, fo, cid)
        assert_backward_criteria(hip, sc, fg, gg, go, seed, tile, mode, cid)
        oracle.release(fo["geom"])
        n += 1
    print(f"backward: {n} cases")
