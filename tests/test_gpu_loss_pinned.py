"""olsr_mapping_loss, olsr_tracking_loss and the fused epilogue of olsr_forward_async_loss pinned to tests/loss_ref.py, the
float32 restatement of csrc/olsr_loss_device.h + csrc/k_loss.hip (itself held to the reference by tests/test_loss_ref_cpu.py).

COTANGENTS: equal to the restatement bit for bit, the sign of zero included.  The build uses -ffp-contract=off and the header
writes no FMA; the one value that is not IEEE-exact is expf(exposure[0]) from the device's libm, so each call tries the
correctly rounded e^a and its two float32 neighbours, and ONE candidate must make every output of the call match.

SUMS (loss[0..3], dL_dexposure[0..1]): |got - truth| <= (D + 2) 2^-24 S, plus one float32 rounding of the result.  truth = the
restatement's exact float32 terms added in float64 and weighted as loss_final_block weights them; S = the same weighted sum over
the terms' magnitudes (for the exposure gradients too: the sum of magnitudes, not the cancelled result); D = the largest number
of float32 additions a term passes through before the doubles, read from the code:
  stand-alone (mapping_loss_kernel): a thread adds the terms of its VEC pixels one after the other to s[k] — per pixel 3 colour
    terms to s[0], s[3], s[4], 1 depth term to s[1], F language terms to s[2] — so n VEC additions with n = 3, 1, F, 3, 3 (the
    first, 0 + t, is exact: counted all the same); wave_sum is six levels of v += shfl_xor(v, m); thread k then adds the four
    waves' values, v = 0; v += red[0..3]: three that round.  D = n VEC + 6 + 3: 21 / 13 / 4 F + 9 on the 16-byte path,
    12 / 10 / F + 9 on the scalar path.  The partials are then added in double (loss_final_block): below 2^-24 by 2^-29.
  fused epilogue (render_fwd_kernel, LOSS != 0): one pixel per thread, so n additions; the same six-level wave_sum;
    ((w0 + w1) + w2) + w3: three.  D = n + 6 + 3: 12 / 10 / F + 9.
Each addition perturbs the partial sum it forms, which is at most S, by at most 2^-24 relative: D 2^-24 S to first order; the
+ 2 covers the second-order terms and the doubles.  D is not measured.  Each case prints its observed error in units of 2^-24 S.

LANGUAGE SIGN: t64 = the bilinear sum in float64 over the float32 weights.  dL_dlanguage may differ from sign(l - t64) wl only
where |l - t64| <= 5 * 2^-24 * mag, mag the same sum over magnitudes: four roundings on a path of the float32 sum (product,
inner sum, product, outer sum) plus one for second-order terms.  No cap on their number, and none anywhere else.

Shapes are the smallest at which each structural edge exists (the table of each test)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import loss_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
EXPOSURE = np.array([0.11, -0.03], dtype=F32)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def _n(t):
    return None if t is None else t.detach().cpu().numpy()


def _got(o):
    return {k: _n(o.get(k)) for k in ("loss", "dL_dimage", "dL_ddepth", "dL_dlanguage", "dL_dexposure")}


def make_inputs(W, H, F=0, lw=0, lh=0, seed=0):
    """Random images with a quarter of the colour targets under the threshold, a quarter of the depths invalid, opacities
    around 0.95 and a 30 % grad_mask; masks by pixel, so that a 1-row image has them too."""
    g = torch.Generator().manual_seed(1000 * F + 7 * W + H + seed)
    r = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    c = dict(image=r(3, H, W), depth=r(1, H, W) * 5, lang=torch.randn(F, H, W, generator=g) * 0.3 if F else None,
             gt_image=r(3, H, W), gt_depth=r(H, W) * 5,
             gt_lang=torch.randn(F, lh, lw, generator=g) * 0.3 if F and lw else None,
             opacity=r(1, H, W) * 0.2 + 0.85, grad_mask=(r(H, W) > 0.3).float())
    c["gt_image"][:, r(H, W) < 0.25] *= 0.001
    c["gt_depth"][r(H, W) < 0.25] = 0.0
    return {k: (None if v is None else v.numpy()) for k, v in c.items()}


def run_mapping(c, exposure=EXPOSURE, label="", vec4=None, **kw):
    """olsr_mapping_loss through losses.mapping_loss, pinned."""
    from online_lang_splatting_amd import losses
    o = losses.mapping_loss(_t(c["image"]), _t(c["depth"]), _t(c["lang"]), _t(c["gt_image"]), _t(c["gt_depth"]), _t(c["gt_lang"]),
                            _t(exposure), **kw)
    H, W = c["image"].shape[1:]
    Fc = 0 if c["lang"] is None else c["lang"].shape[0]
    rk = dict(alpha=kw.get("alpha", 0.95), thr=kw.get("rgb_boundary_threshold", 0.01), lamda=kw.get("lamda_lang", 1.0),
              initialization=kw.get("initialization", False))
    args = (c["image"], c["depth"], c["lang"], c["gt_image"], c["gt_depth"], c["gt_lang"], exposure)
    got = _got(o)
    if Fc == 0:
        got["dL_dlanguage"] = None
    rep = LR.pin(got, args, rk, LR.adds_standalone(Fc, W % 4 == 0 if vec4 is None else vec4), f"mapping {label}")
    return got, rep


def run_tracking(c, exposure=EXPOSURE, label="", masked=True, vec4=None, **kw):
    """olsr_tracking_loss through losses.tracking_loss, pinned."""
    from online_lang_splatting_amd import losses
    gm = c["grad_mask"] if masked else None
    o = losses.tracking_loss(_t(c["image"]), _t(c["depth"]), _t(c["opacity"]), _t(c["gt_image"]), _t(c["gt_depth"]), _t(gm),
                             _t(exposure), **kw)
    W = c["image"].shape[2]
    rk = dict(alpha=kw.get("alpha", 0.95), thr=kw.get("rgb_boundary_threshold", 0.01), tracking=True, opacity=c["opacity"],
              grad_mask=gm)
    args = (c["image"], c["depth"], None, c["gt_image"], c["gt_depth"], None, exposure)
    got = _got(o)
    got["dL_dlanguage"] = None
    rep = LR.pin(got, args, rk, LR.adds_standalone(0, W % 4 == 0 if vec4 is None else vec4), f"tracking {label}")
    return got, rep


# W x H.  16-byte path (W % 4 == 0, torch's allocations are aligned): one thread; one wave partly empty; 65 threads = a second
# wave with one lane; one full block; 257 threads = a second block with one thread; 258 blocks = a second trip of the final
# block's strided loop.  Scalar path: the same edges with one pixel per thread.
VEC4_SIZES = [(4, 1), (16, 16), (260, 1), (32, 32), (1028, 1), (516, 512)]
SCALAR_SIZES = [(1, 1), (63, 1), (65, 1), (255, 1), (257, 1), (257, 257)]


@pytest.mark.parametrize("W,H", VEC4_SIZES + SCALAR_SIZES)
def test_block_and_wave_edges_of_the_standalone_kernel(hip, W, H):
    from online_lang_splatting_amd._lib import lib
    vec = 4 if W % 4 == 0 else 1
    threads = (W * H + vec - 1) // vec
    blocks = (threads + 255) // 256
    assert blocks <= lib().olsr_mapping_loss_scratch_bytes(W, H) // (5 * 4)      # the partials fit what the entry asked for
    if (W, H) in ((516, 512), (257, 257)):
        assert blocks > 256
    c = make_inputs(W, H)
    run_mapping(c, label=f"{W}x{H}")
    run_mapping(c, exposure=None, label=f"{W}x{H} exposure=None")
    run_tracking(c, label=f"{W}x{H}")
    run_tracking(c, label=f"{W}x{H} no grad_mask", masked=False)


def _abi_call(c, tracking, F, offset):
    """The entry through the C ABI with the named pointer starting 4 bytes into its allocation (None: all aligned)."""
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd._lib import check, lib
    H, W = c["image"].shape[1:]

    def place(name, a=None, shape=None):
        n = int(np.prod(shape if shape is not None else a.shape))
        buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[1:n + 1] if name == offset else buf[:n]
        if a is not None:
            v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).reshape(-1))
        assert (v.data_ptr() % 16 == 4) == (name == offset)
        return v
    t = {k: place(k, c[k]) for k in ("image", "depth", "gt_image", "gt_depth")}
    t["dL_dimage"], t["dL_ddepth"] = place("dL_dimage", shape=(3, H, W)), place("dL_ddepth", shape=(H, W))
    loss, dexp, expo = torch.zeros(4, device=DEV), torch.zeros(2, device=DEV), _t(EXPOSURE)
    L = lib()
    scratch = torch.empty(L.olsr_mapping_loss_scratch_bytes(W, H), dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = _abi.OlsrLossParams(width=W, height=H, F=0 if tracking else F, lang_width=W if F and not tracking else 0,
                            lang_height=H if F and not tracking else 0, initialization=0, alpha=0.95,
                            rgb_boundary_threshold=0.01, lamda_lang=1.0)
    if tracking:
        t["opacity"], t["grad_mask"] = place("opacity", c["opacity"]), place("grad_mask", c["grad_mask"])
        check(L.olsr_tracking_loss(C.byref(p), t["image"].data_ptr(), t["depth"].data_ptr(), t["opacity"].data_ptr(),
                                   t["gt_image"].data_ptr(), t["gt_depth"].data_ptr(), t["grad_mask"].data_ptr(), expo.data_ptr(),
                                   t["dL_dimage"].data_ptr(), t["dL_ddepth"].data_ptr(), loss.data_ptr(), dexp.data_ptr(),
                                   scratch.data_ptr(), st))
    else:
        if F:
            t["lang"], t["gt_lang"] = place("lang", c["lang"]), place("gt_lang", c["gt_lang"])
            t["dL_dlanguage"] = place("dL_dlanguage", shape=(F, H, W))
        ptr = lambda k: t[k].data_ptr() if k in t else None  # noqa: E731
        check(L.olsr_mapping_loss(C.byref(p), t["image"].data_ptr(), t["depth"].data_ptr(), ptr("lang"), t["gt_image"].data_ptr(),
                                  t["gt_depth"].data_ptr(), ptr("gt_lang"), expo.data_ptr(), t["dL_dimage"].data_ptr(),
                                  t["dL_ddepth"].data_ptr(), ptr("dL_dlanguage"), loss.data_ptr(), dexp.data_ptr(),
                                  scratch.data_ptr(), st))
    torch.cuda.synchronize()
    return dict(loss=_n(loss), dL_dexposure=_n(dexp), dL_dimage=_n(t["dL_dimage"]).reshape(3, H, W),
                dL_ddepth=_n(t["dL_ddepth"]).reshape(1, H, W),
                dL_dlanguage=_n(t["dL_dlanguage"]).reshape(F, H, W) if "dL_dlanguage" in t else None)


@pytest.mark.parametrize("W,H", [(16, 16), (32, 32)])
def test_a_misaligned_pointer_takes_the_scalar_path_with_the_same_bits(hip, W, H):
    """Each pointer of the 16-byte test (launch_mapping_loss) in turn 4 bytes into its allocation: the call must fall back to
    one pixel per thread — a 16-byte access there would fault or read the neighbour — and the cotangents have the aligned
    run's bits.  Mapping at F = 0 as the table says, and at F = 3 (identity-size target) so that language and dL_dlanguage are
    pointers too; gt_language is read by scalar loads on both paths and is offset for that reason."""
    for tracking, F in ((False, 0), (False, 3), (True, 0)):
        c = make_inputs(W, H, F, W if F else 0, H if F else 0)
        rk = dict(tracking=True, opacity=c["opacity"], grad_mask=c["grad_mask"]) if tracking else {}
        args = (c["image"], c["depth"], None if tracking else c["lang"], c["gt_image"], c["gt_depth"],
                None if tracking else c["gt_lang"], EXPOSURE)
        who = "tracking" if tracking else f"mapping F={F}"
        rk["depth_weight_from_float"] = True     # _abi_call leaves olsr_loss_params.one_minus_alpha 0: the library's 1.f - alpha
        base = _abi_call(c, tracking, F, None)
        LR.pin(base, args, rk, LR.adds_standalone(F, True), f"{who} {W}x{H} aligned")
        names = ["image", "depth", "gt_image", "gt_depth", "dL_dimage", "dL_ddepth"]
        names += ["opacity", "grad_mask"] if tracking else (["lang", "gt_lang", "dL_dlanguage"] if F else [])
        for name in names:
            o = _abi_call(c, tracking, F, name)
            for k in ("dL_dimage", "dL_ddepth", "dL_dlanguage"):
                assert (o[k] is None and base[k] is None) or LR.same_bits(o[k], base[k]), (who, name, k)
            # gt_language is not part of the 16-byte test: that run stays on the 16-byte path, every other one leaves it
            LR.pin(o, args, rk, LR.adds_standalone(F, name == "gt_lang"), f"{who} {W}x{H} {name} + 4 bytes")


@pytest.mark.parametrize("F", [3, 15, 16, 32])
def test_every_channel_count_and_target_size(hip, F):
    """W x H = 20 x 12 (16-byte path) and 21 x 13 (scalar); targets w x h = 5 x 7 (smaller), 40 x 48 (larger), the image's
    size (every weight 1 or 0) and 1 x 1 (every index clamped); then no target at all, exposure=None, and initialization."""
    for W, H in ((20, 12), (21, 13)):
        for lw, lh in ((5, 7), (40, 48), (W, H), (1, 1)):
            c = make_inputs(W, H, F, lw, lh)
            run_mapping(c, label=f"F={F} {W}x{H} target {lw}x{lh}")
        got, _ = run_mapping(dict(c, gt_lang=None), label=f"F={F} {W}x{H} no target")
        assert got["loss"][3] == 0 and (LR.f32_bits(got["dL_dlanguage"]) == 0).all()
        got, _ = run_mapping(c, exposure=None, label=f"F={F} {W}x{H} exposure=None")
        assert (LR.f32_bits(got["dL_dexposure"]) == 0).all()
        got, _ = run_mapping(c, label=f"F={F} {W}x{H} initialization", initialization=True)
        assert (LR.f32_bits(got["dL_dexposure"]) == 0).all()


EDGE_CASES = LR.load_cases("loss_edges")


def _case_inputs(c, tracking):
    H, W = c["gt_depth"].shape
    d = {k: c.get(k) for k in ("image", "depth", "lang", "gt_image", "gt_depth", "gt_lang", "opacity", "grad_mask")}
    if not tracking:   # a mapping case through the tracking entry as well: an opacity that straddles 0.95, no grad_mask
        d["opacity"] = (0.9 + 0.1 * np.random.default_rng(5).random((1, H, W))).astype(F32)
        d["grad_mask"] = np.ones((H, W), dtype=F32)
    return d


@pytest.mark.parametrize("name,tracking,c", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_planted_decisions_through_both_entries(hip, name, tracking, c):
    """Every case of tests/golden/loss_edges.npz (thresholds met exactly and one ulp either side, ties, a zero grad_mask on a live
    pixel, the four kinds of target, non-finite pixels; counted in tests/test_loss_ref_cpu.py) through olsr_mapping_loss AND
    olsr_tracking_loss, each pinned to the restatement; the entry the case was recorded from is also held to what the
    reference returned: zero pattern and sign exactly.
    Non-finite pixels: exactly the sums that the float64 statement makes non-finite are non-finite (check_sums: a NaN truth
    needs NaN, an infinite one the same infinity, a finite one a finite result within the bound); every other pixel's cotangent
    keeps the bits of the run with those pixels replaced by 0.5; the poisoned pixels' own cotangents are the fixture's — +0
    at a NaN, and at +inf the golden's value within the 2 ulp of the two orders of forming alpha / (3 H W)."""
    d = _case_inputs(c, tracking)
    expo = np.array([c["a"][0], c["b"][0]], dtype=F32)
    kw = dict(alpha=float(c["alpha"]), rgb_boundary_threshold=float(c["thr"]))
    init = (not tracking) and bool(int(c["init"]))
    runs = {}
    runs[False] = run_mapping(d, exposure=expo, label=name, initialization=init, **kw)[0]
    runs[True] = run_tracking(d, exposure=expo, label=name, **kw)[0]
    own = runs[tracking]
    for k, g in (("dL_dimage", "d_image"), ("dL_ddepth", "d_depth")) + (() if tracking else (("dL_dlanguage", "d_lang"),)):
        assert np.array_equal(own[k] == 0, c[g] == 0) and np.array_equal(np.sign(own[k]), np.sign(c[g])), (name, k)
    bad = ~np.isfinite(d["image"])
    bad_lang = None if d["lang"] is None else ~np.isfinite(d["lang"])
    if not bad.any() and (bad_lang is None or not bad_lang.any()):
        assert np.isfinite(own["loss"]).all()
        return
    assert not np.isfinite(own["loss"][0])
    clean = dict(d, image=np.where(bad, F32(0.5), d["image"]))
    if bad_lang is not None:
        clean["lang"] = np.where(bad_lang, F32(0.5), d["lang"])
    cleans = {False: run_mapping(clean, exposure=expo, label=name + " cleaned", initialization=init, **kw)[0],
              True: run_tracking(clean, exposure=expo, label=name + " cleaned", **kw)[0]}
    for tr in (False, True):
        assert np.isfinite(cleans[tr]["loss"]).all()
        assert np.array_equal(LR.f32_bits(runs[tr]["dL_dimage"])[~bad], LR.f32_bits(cleans[tr]["dL_dimage"])[~bad])
        assert LR.same_bits(runs[tr]["dL_ddepth"], cleans[tr]["dL_ddepth"])
        assert (LR.f32_bits(runs[tr]["dL_dimage"])[np.isnan(d["image"])] == 0).all()
    if bad_lang is not None and bad_lang.any():
        assert np.array_equal(LR.f32_bits(runs[False]["dL_dlanguage"])[~bad_lang], LR.f32_bits(cleans[False]["dL_dlanguage"])[~bad_lang])
        assert (LR.f32_bits(own["dL_dlanguage"])[bad_lang] == 0).all() and (c["d_lang"][bad_lang] == 0).all()
    elif not tracking:
        assert LR.same_bits(runs[False]["dL_dlanguage"], cleans[False]["dL_dlanguage"])
    if bad.any():
        gold, mine = c["d_image"][bad], own["dL_dimage"][bad]
        assert np.array_equal(np.sign(mine), np.sign(gold)) and (gold[np.isnan(d["image"][bad])] == 0).all()
        assert (np.abs(mine.astype(np.float64) - gold.astype(np.float64)) <= 2 * np.spacing(np.abs(gold)).astype(np.float64)).all()


# ---- the fused epilogue ---------------------------------------------------------------------------------------------------
def _workspace(F, W, H, tile, seed):
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    from online_lang_splatting_amd.scene import make_scene
    dev = torch.device(DEV)
    # (scale_mult: the generator's default covers every pixel many times over; a quarter of its scales leaves about half of the
    #  pixels under opacity 0.95, so that the tracking loss's depth mask decides both ways)
    sc = make_scene(2000, W, H, F, seed=seed, bg=torch.tensor([0.2, 0.1, 0.3]), scale_mult=0.25)
    cam = sc.camera
    ws = RasterWorkspace(sc.P, W, H, F, sc.shs.shape[1], 400000, dev, tile=tile)
    ws.set_scene(sh_degree=sc.sh_degree, bg=sc.bg.to(dev), means3D=sc.means3D.to(dev), opacities=sc.opacities.to(dev),
                 scales=sc.scales.to(dev), rotations=sc.rotations.to(dev), shs=sc.shs.to(dev),
                 language=None if F == 0 else sc.language.to(dev), viewmatrix=cam.world_view_transform.to(dev),
                 projmatrix=cam.full_proj_transform.to(dev), projmatrix_raw=cam.projection_matrix.to(dev),
                 campos=cam.camera_center.to(dev), tanfovx=cam.tanfovx, tanfovy=cam.tanfovy)
    return ws


# F, W, H, tile, target w x h, the form of the language window.  157 x 101: ragged in both directions.  257 x 257: 324 tiles
# of 15, 289 of 16 — more than 256 partials, the final block's second trip.  Language: a small target enlarged and, at F = 3,
# the image's own size (a tile's window fits the idle feature rows: staged in LDS); 300 x 200 on 64 x 64 (a tile's window is
# about 72 x 49 texels per channel) and the image's own size at F = 32 (17 x 17 texels x 32 channels): gathered; at F = 3 the
# 300 x 200 target's windows fit in the ragged last tiles only: both forms in one launch.
FUSED = [(0, 157, 101, 15, None, None), (0, 157, 101, 16, None, None), (0, 257, 257, 15, None, None),
         (0, 257, 257, 16, None, None), (15, 96, 64, 15, (12, 9), "staged"), (16, 96, 64, 16, (12, 9), "staged"),
         (32, 61, 47, 16, (24, 20), "staged"), (3, 64, 64, 15, (64, 64), "staged"), (3, 64, 64, 15, (300, 200), "both"),
         (15, 64, 64, 16, (300, 200), "gathered"), (32, 61, 47, 16, (61, 47), "gathered")]


def _window_forms(F, W, H, tile, lw, lh):
    """Which form each tile's language window takes: the epilogue's own test (k_render_fwd.hip: the window of texels the
    tile's pixels read, ww * wh * F floats, is staged when it fits the B * FR = 128 * round_up(4 + F, 4) idle floats)."""
    x0, x1, _, _ = LR.bilinear_index(W, lw)
    y0, y1, _, _ = LR.bilinear_index(H, lh)
    room = 128 * ((4 + F + 3) // 4 * 4)
    forms = set()
    for by in range(0, H, tile):
        for bx in range(0, W, tile):
            ww = int(x1[min(bx + tile - 1, W - 1)]) - int(x0[bx]) + 1
            wh = int(y1[min(by + tile - 1, H - 1)]) - int(y0[by]) + 1
            forms.add("staged" if ww * wh * F <= room else "gathered")
    return forms


@pytest.mark.parametrize("F,W,H,tile,target,form", FUSED)
def test_fused_epilogue_is_pinned_on_the_images_the_plain_forward_wrote(hip, F, W, H, tile, target, form):
    if F:
        assert _window_forms(F, W, H, tile, *target) == ({"staged", "gathered"} if form == "both" else {form})
    ws = _workspace(F, W, H, tile, seed=500 + F + W)
    ntiles = ((W + tile - 1) // tile) * ((H + tile - 1) // tile)
    if W == 257:
        assert ntiles == (324 if tile == 15 else 289)
    out = ws.forward()
    torch.cuda.synchronize()
    assert int(ws.num_rendered[1]) == 0                       # no instance was dropped for want of capacity
    img = {k: _n(out[k]).copy() for k in ("color", "depth", "opacity", "language")}
    opaque = int((img["opacity"] > F32(0.95)).sum())
    assert np.isfinite(img["color"]).all() and W * H // 5 < opaque < W * H - W * H // 5       # opacity > 0.95 decides both ways
    c = make_inputs(W, H, F, *(target or (0, 0)), seed=3)
    lang = img["language"] if F else None
    gt_image, gt_depth, gt_lang, gm = _t(c["gt_image"]), _t(c["gt_depth"]), _t(c["gt_lang"]), _t(c["grad_mask"])
    D = LR.adds_epilogue(F)
    for exposure in (EXPOSURE, None):
        for skip in (False, True):
            for k in img:
                ws.out[k].fill_(-7.0)
            fu = ws.forward_loss(gt_image, gt_depth, gt_lang, _t(exposure), skip_images=skip)
            torch.cuda.synchronize()
            for k in img:   # written exactly as by the plain forward, or not at all
                assert LR.same_bits(_n(ws.out[k]), np.full_like(img[k], -7.0) if skip else img[k]), (k, skip)
            got = _got(fu)
            args = (img["color"], img["depth"], lang, c["gt_image"], c["gt_depth"], c["gt_lang"], exposure)
            LR.pin(got, args, {}, D, f"fused mapping F={F} {W}x{H} tile {tile} target {target} "
                                     f"exposure={'on' if exposure is not None else 'None'} skip_images={skip}")
    for masked in (True, False):
        fu = ws.forward_loss(gt_image, gt_depth, None, _t(EXPOSURE), gm if masked else None, tracking=True)
        torch.cuda.synchronize()
        got = _got(fu)
        assert got["dL_dlanguage"] is None
        rk = dict(tracking=True, opacity=img["opacity"], grad_mask=c["grad_mask"] if masked else None)
        args = (img["color"], img["depth"], None, c["gt_image"], c["gt_depth"], None, EXPOSURE)
        LR.pin(got, args, rk, D, f"fused tracking F={F} {W}x{H} tile {tile} grad_mask={masked}")
