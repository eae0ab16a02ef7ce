"""The raw-parameter render path (OLSR_ACT_*: the kernels apply sigmoid / exp / normalize themselves and chain the gradients
back to the raw arrays) held bit for bit, per flag, to the activations = 0 path that the oracle parity tests pin.

olsr_debug_activate returns the activated values A through the very device functions the kernels call, so expf — the one
operation a CPU cannot restate bit for bit — drops out: the un-fused frame renders A with activations = 0, the fused frame
renders the raw arrays with the flags, and everything between them is an equality.  The chained gradients equal
tests/act_ref.py's float32 restatement applied to the un-fused gradients, and lie within its float64 bound
(tests/test_act_ref_cpu.py derives it: 3 / 1 / 18 roundings x 2^-24 for opacity / scale / rotation).

Measured on an MI355X (this file's own print-outs, largest over all cases; bounds in brackets), in units of 2^-24 of the element
(opacity, scale) or of its condition (rotation): opacity chain 2.00 (3), scale chain 0.96 (1), rotation chain 4.27 (18);
the hook's expf 0.85 ulp (1), its sigmoid 0.75 of its bound.  DESIGN.md, "The raw-parameter path, pinned per flag"."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import act_ref as A
from online_lang_splatting_amd import _abi
from online_lang_splatting_amd.scene import arc_cameras, make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, P_SCENE, CAPACITY = 160, 120, 3000, 400000
OP, SC, ROT = _abi.ACT_OPACITY_SIGMOID, _abi.ACT_SCALE_EXP, _abi.ACT_ROTATION_NORMALIZE
IMAGES = ("color", "language", "depth", "opacity", "radii", "n_touched")
UNTOUCHED = ("dL_dmeans2D", "dL_dconic", "dL_dcolors", "dL_dlanguage", "dL_ddepths", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
             "dL_dtau", "dL_dtau_sum")
CHAINED = ((OP, "dL_dopacity"), (SC, "dL_dscales"), (ROT, "dL_drotations"))


def _cam(c, dev):
    return dict(viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev),
                projmatrix_raw=c.projection_matrix.to(dev), campos=c.camera_center.to(dev), tanfovx=c.tanfovx, tanfovy=c.tanfovy)


@functools.lru_cache(maxsize=None)
def _case(F):
    """The suite's small scene with the edge rows of act_ref.edge_rows() planted in rows [0, E), raw parameters for every row
    (un-normalised quaternions of norm 0.3 - 2.3 on the random rows), and their activations by the library's own hook.
    F = 15 carries SH degree 3 (M = 16: the bucket row's 48-float SH slice), F = 0 degree 0."""
    from online_lang_splatting_amd import _lib
    dev = torch.device(DEV)
    sc = make_scene(P_SCENE, W, H, F, seed=29 + F, max_sh_degree=3 if F else 0)
    e = A.edge_rows()
    E = len(e["names"])
    g = torch.Generator().manual_seed(31)
    raw_op = torch.logit(sc.opacities.clamp(1e-4, 1 - 1e-4))
    raw_sc = torch.log(sc.scales)
    raw_rot = sc.rotations * (0.3 + 2 * torch.rand(sc.P, 1, generator=g))
    means = sc.means3D.clone()
    for t, k in ((means, "means3D"), (raw_op, "opacities"), (raw_sc, "scales"), (raw_rot, "rotations")):
        t[:E] = torch.from_numpy(e[k])
    raw = tuple(t.to(dev).contiguous() for t in (raw_op, raw_sc, raw_rot))
    act_all = _lib.debug_activate(_abi.ACT_ALL, *raw)
    cams = [sc.camera] + arc_cameras(W, H, 2)[1:]
    base = dict(bg=sc.bg.to(dev), means3D=means.to(dev).contiguous(), shs=sc.shs.to(dev), sh_degree=sc.sh_degree,
                language=sc.language.to(dev) if F else None)
    cot = [tuple(None if t is None else t.to(dev) for t in sc.cotangents(40 + v)) for v in range(2)]
    return SimpleNamespace(F=F, P=sc.P, M=sc.shs.shape[1], E=E, edge=e, raw=raw, act_all=act_all, base=base, dev=dev,
                           cams=[_cam(c, dev) for c in cams], cot=cot)


def _inputs(s, act):
    """What a caller hands the library for the flag subset `act`: the raw array where the flag is set, the activated one where
    it is not; and A, the hook's activation of exactly those arrays (an unflagged array is copied through)."""
    from online_lang_splatting_amd import _lib
    given = tuple(s.raw[i] if act & bit else s.act_all[i] for i, bit in enumerate((OP, SC, ROT)))
    activated = _lib.debug_activate(act, *given)
    for i, bit in enumerate((OP, SC, ROT)):
        if not act & bit:
            assert torch.equal(activated[i], given[i])     # copied through
        else:
            assert torch.equal(activated[i], s.act_all[i])  # one array's activation does not depend on the other flags
    return given, activated


def _workspace(s, bwd_mode=_abi.BWD_REFERENCE, binning=_abi.BINNING_ELLIPSE):
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    return RasterWorkspace(s.P, W, H, s.F, s.M, CAPACITY, s.dev, bwd_mode=bwd_mode, binning=binning)


def _frame(ws, s, arrays, act, view=0, backward=True):
    """One forward (+ backward) on `ws`: clones of the images, the state fields, R, the sorted list, and the gradients."""
    from online_lang_splatting_amd import _C
    op, sc_, rot = arrays
    ws.set_scene(opacities=op, scales=sc_, rotations=rot, activations=act, **s.cams[view], **s.base)
    out = {k: v.clone() for k, v in ws.forward().items()}
    R, overflow = ws.rendered()
    assert not overflow and R > 0
    out["R"] = R
    out["final_T"] = _C.state_field("image", ws.img, "final_T", W=W, H=H, dtype=torch.float32, count=W * H).clone()
    out["n_contrib"] = _C.state_field("image", ws.img, "n_contrib", W=W, H=H, dtype=torch.int32, count=W * H).clone()
    out["point_list"] = _C.state_field("binning", ws.binning, "point_list", R=ws.capacity, F=ws.F, dtype=torch.int32, count=R).clone()
    if not backward:
        return out, None
    g = {k: v.clone() for k, v in ws.backward(*s.cot[view]).items()}
    assert not ws.backward_status()[1]
    return out, g


def _assert_same_forward(a, b, where):
    assert a["R"] == b["R"], where
    for k in IMAGES + ("final_T", "n_contrib", "point_list"):
        assert torch.equal(a[k], b[k]), (where, k)
    for k in ("color", "language", "depth", "opacity", "final_T"):
        assert bool(torch.isfinite(a[k]).all()), (where, k)


def _assert_chain(s, act, given, activated, gu, gf, where, measured):
    """gf (fused, flags `act`) against gu (un-fused, the activated arrays): untouched gradients equal, flagged ones equal to
    the restated chain of gu and within its float64 bound, and the comparison has teeth."""
    for k in UNTOUCHED:
        assert torch.equal(gf[k], gu[k]), (where, k)
    E = s.E
    A_op, A_sc, A_rot = activated
    for bit, k in CHAINED:
        u, f = gu[k].cpu().numpy(), gf[k].cpu().numpy()
        assert np.isfinite(u).all() and np.isfinite(f).all(), (where, k)
        if not act & bit:
            assert torch.equal(gf[k], gu[k]), (where, k)
            continue
        if bit == OP:
            want = A.opacity_chain(u, A_op).reshape(f.shape)
            truth = A.opacity_truth(u, A_op).reshape(f.shape)
            bound, K, keep = A.opacity_bound(truth), A.K_OPACITY, np.ones(s.P, bool)
        elif bit == SC:
            want = A.scale_chain(u, A_sc)
            truth = A.scale_truth(u, A_sc)
            bound, K, keep = A.scale_bound(truth), A.K_SCALE, np.ones(s.P, bool)
        else:
            q = given[2]
            # the activated rotation the un-fused frame rendered IS the restated h, bit for bit
            assert A.same_bits(A_rot, A.normalize_forward(q)), where
            want = A.rotation_chain(u, q)
            truth = A.rotation_truth(u, q)[1]
            keep = ~A.clamp_active(q)            # the planted zero quaternion: held to the restatement only
            assert int((~keep).sum()) == A.N_CLAMP_PLANTED and not keep[:E].all()
            bound, K = A.rotation_bound(u, q), A.K_ROT_BWD
        assert A.same_bits(f, want), (where, k, int((f != want).sum()))
        err = np.abs(f.astype(np.float64) - truth)
        assert np.isfinite(truth[keep]).all()
        assert (err[keep] <= bound[keep]).all(), (where, k, float((err[keep] / bound[keep]).max()))
        # (in the bound's own unit: 2^-24 of the element or of its condition, plus the underflow term)
        measured[k] = max(measured.get(k, 0.0), float((err[keep] / (bound[keep] / K)).max()))
        # teeth: gradients flow through planted and random rows, and the chain changes them
        rows_u = (u.reshape(s.P, -1) != 0).any(1)
        changed = rows_u & (f.reshape(s.P, -1) != u.reshape(s.P, -1)).any(1)
        assert rows_u[:E].any() and changed[:E].any(), (where, k)
        assert rows_u[E:].mean() >= 0.01 and changed[E:].mean() >= 0.01, (where, k, float(rows_u[E:].mean()))


@pytest.mark.parametrize("F", [0, 15])
@pytest.mark.parametrize("act", range(8))
def test_raw_path_equals_unfused_path_bit_for_bit(hip, act, F):
    """fused (raw arrays, flags) == un-fused (the hook's activations, no flags) on one workspace, in the order fused ->
    un-fused -> fused so that a state the flags might leave behind would show: images, radii, n_touched, final_T, n_contrib,
    R and the sorted list in both binning modes; every untouched gradient; every flagged gradient against act_ref.
    All flags together also run the exact-order backward (BWD_EXACT).
    Measured distance of the chained gradients from the float64 truth, largest over the sixteen cases, in units of 2^-24 of
    the element (opacity, scale) or of its condition (rotation): opacity 2.00 (bound 3), scale 0.96 (bound 1), rotation 4.27
    (bound 18)."""
    s = _case(F)
    given, activated = _inputs(s, act)
    measured = {}
    configs = [(_abi.BWD_REFERENCE, _abi.BINNING_ELLIPSE), (_abi.BWD_REFERENCE, _abi.BINNING_RECT)]
    if act == _abi.ACT_ALL:
        configs.append((_abi.BWD_EXACT, _abi.BINNING_ELLIPSE))
    for mode, binning in configs:
        where = f"act={act} F={F} mode={mode} binning={binning}"
        ws = _workspace(s, mode, binning)
        of1, gf1 = _frame(ws, s, given, act)
        ou, gu = _frame(ws, s, activated, 0)
        of2, gf2 = _frame(ws, s, given, act)
        _assert_same_forward(of1, ou, where)
        _assert_same_forward(of2, of1, where + " (again)")
        for k in gf1:
            assert A.same_bits(gf2[k], gf1[k]), (where, k)
        # the planted scale rows still render (a radius > 0)
        names = s.edge["names"]
        for n in ("scale 0", "scale min", "scale max", "scale axis -8"):
            assert 0 < int(ou["radii"][names.index(n)]) < 2 ** 31 - 1, n
        _assert_chain(s, act, given, activated, gu, gf1, where, measured)
    print(f"act={act} F={F} chained gradients vs float64, max error / (2^-24 x element or condition): "
          + " ".join(f"{k}={v:.3f}" for k, v in measured.items()))
    for k, v in measured.items():
        assert v <= dict(dL_dopacity=A.K_OPACITY, dL_dscales=A.K_SCALE, dL_drotations=A.K_ROT_BWD)[k]


@pytest.mark.parametrize("F", [0, 15])
@pytest.mark.parametrize("act", range(8))
def test_bucket_receives_the_chained_gradients(hip, act, F):
    """backward(bucket=..., first=True) on one view and first=False on a second, with the flags, and the same with
    bucket_only=True: flat, densify and max_radii equal GradientBucket.accumulate of the separately returned (chained) arrays;
    the row masks of the two fused buckets equal each other and the mask of an un-fused bucket, and cover every non-zero row.
    pose_only=True (tracking) gives the un-fused dL_dtau_sum."""
    from online_lang_splatting_amd.frame_shard import GradLayout, GradientBucket
    s = _case(F)
    given, activated = _inputs(s, act)
    ws = _workspace(s)
    lay = GradLayout(s.M, F)
    ref = GradientBucket(s.P, lay, s.dev)
    fused, only, unfused = (GradientBucket(s.P, lay, s.dev, track_rows=True) for _ in range(3))
    for b in (ref, fused, only, unfused):   # stale contents must be overwritten by the first view
        b.flat.fill_(7.0)
        b.densify.fill_(7.0)
        b.max_radii.fill_(7)
    for v in range(2):
        ou, gu = _frame(ws, s, activated, 0, view=v)
        ws.backward(*s.cot[v], bucket=unfused, first=(v == 0), bucket_only=True)
        of, sep = _frame(ws, s, given, act, view=v)
        _assert_same_forward(of, ou, f"view {v}")
        assert torch.equal(sep["dL_dtau_sum"], gu["dL_dtau_sum"])
        ref.accumulate(sep, of["radii"], first=(v == 0))
        g2 = ws.backward(*s.cot[v], bucket=fused, first=(v == 0))
        for k in sep:  # the separate arrays are still written, identically
            assert A.same_bits(g2[k], sep[k]), k
        g3 = ws.backward(*s.cot[v], bucket=only, first=(v == 0), bucket_only=True)
        assert torch.equal(g3["dL_dtau_sum"], gu["dL_dtau_sum"]) and g3["dL_dopacity"] is None
        g4 = ws.backward(*s.cot[v], pose_only=True)
        assert torch.equal(g4["dL_dtau_sum"], gu["dL_dtau_sum"]) and g4["dL_dmeans3D"] is None
        assert not ws.backward_status()[1]
    for name, b in (("fused", fused), ("bucket_only", only)):
        assert torch.equal(b.flat, ref.flat), name
        assert torch.equal(b.densify, ref.densify), name
        assert torch.equal(b.max_radii, ref.max_radii), name
        assert torch.equal(b.row_mask, unfused.row_mask), name
    nonzero = (ref.flat != 0).any(1).cpu().numpy()
    bits = np.unpackbits(fused.row_mask.cpu().numpy().view(np.uint8), bitorder="little")[: s.P].astype(bool)
    assert nonzero.sum() > 0.01 * s.P and not (nonzero & ~bits).any()
    sl = lay.slices()
    for bit, k in (("opacity", OP), ("scales", SC), ("rotations", ROT)):
        col = ref.flat[:, sl[bit]]
        assert float(col.abs().max()) > 0
        if act & k:   # the bucket holds the chained gradient, not the un-fused one
            assert not torch.equal(col, unfused.flat[:, sl[bit]]), bit
        else:
            assert torch.equal(col, unfused.flat[:, sl[bit]]), bit
    assert int((ref.densify[:, 1] == 2).sum()) > 0


def test_activation_hook_against_float64(hip):
    """olsr_debug_activate against exp / sigmoid in double, on the scene's raw rows (edge rows included) and on dense sweeps of
    the arguments the parameters take (log-scales -87 ... 16, logits -30 ... 30).
    exp: OCML documents expf as accurate to 1 ulp: |s - exp(x)| <= ulp(exp(x)).
    sigmoid: act_sigmoid is 1 / (1 + expf(-x)).  With e' = e (1 + eps), |eps| <= 2^-23 (1 ulp, relative), the correctly rounded
    addition t = (1 + e')(1 + d1) and division o = (1 / t)(1 + d2), |d| <= 2^-24, to first order
        o / sigma - 1 = -eps e / (1 + e) - d1 + d2,    e / (1 + e) = 1 - sigma,
    so |o - sigma| <= (2 (1 - sigma) + 2) x 2^-24 x sigma: between 2 and 4 units of 2^-24, relative.  Where expf(-x) overflows
    (x < -88.72) the result is exactly 0 (the truth is below 2^-128).
    Measured on an MI355X: expf 0.85 ulp; sigmoid 0.75 of its bound, 2.54 x 2^-24 relative (caller side)."""
    from online_lang_splatting_amd import _lib
    s = _case(0)
    dev = s.dev
    n = 200001
    x_op = torch.cat([s.raw[0].reshape(-1), torch.linspace(-30.0, 30.0, n, device=dev)]).contiguous()
    x_sc = torch.cat([s.raw[1].reshape(-1), torch.linspace(-87.0, 16.0, 3 * n, device=dev)]).reshape(-1, 3).contiguous()
    # (the two arrays need one P: the shorter sweep is padded with zeros)
    Pn = max(x_op.numel(), x_sc.shape[0])
    xo = torch.zeros(Pn, device=dev)
    xo[: x_op.numel()] = x_op
    xs = torch.zeros(Pn, 3, device=dev)
    xs[: x_sc.shape[0]] = x_sc
    o, sc_, _ = _lib.debug_activate(OP | SC, xo, xs, None)
    o, sc_, xo, xs = (t.cpu().numpy() for t in (o, sc_, xo, xs))
    x64 = xs.astype(np.float64)
    ulps = A.ulp_error(sc_, np.exp(x64))
    print(f"expf vs float64: max {ulps.max():.4f} ulp over {ulps.size} arguments")
    assert ulps.max() <= 1.0
    overflow = xo.astype(np.float64) < -math.log(float(np.finfo(np.float32).max))
    assert overflow.sum() == 1 and (o[overflow] == 0).all()         # the planted -90
    xk = xo[~overflow].astype(np.float64)
    sig = 1.0 / (1.0 + np.exp(-xk))
    bound = (2.0 * (1.0 - sig) + 2.0) * A.U * sig + A.TINY
    err = np.abs(o[~overflow].astype(np.float64) - sig)
    print(f"sigmoid vs float64: max {float((err / bound).max()):.4f} of the bound, {float((err / (A.U * sig)).max()):.4f} x 2^-24 "
          f"relative, over {err.size} arguments")
    assert (err <= bound).all()
    assert ((o >= 0) & (o <= 1)).all()
    # an unflagged array and a NULL pair: copied through / left out
    c_op, c_sc, c_rot = _lib.debug_activate(0, s.raw[0], s.raw[1], s.raw[2])
    assert torch.equal(c_op, s.raw[0]) and torch.equal(c_sc, s.raw[1]) and torch.equal(c_rot, s.raw[2])
    assert _lib.debug_activate(ROT, None, None, s.raw[2])[:2] == (None, None)


@pytest.mark.parametrize("fused_loss", [True, False])
def test_mapping_step_buckets_hold_the_restated_chain(hip, fused_loss):
    """MappingStep (one lane, two views, 160 x 120, ACT_ALL, all learning rates 0) with the loss in the composite's epilogue
    and with the stand-alone loss kernel: after iteration(), summed_gradients() equals, bit for bit, the bucket accumulated
    from un-fused frames of the hook's activations — same cameras and targets, cotangents from losses.mapping_loss on the
    un-fused images (the same bits, by the forward equality), gradients chained by act_ref."""
    from online_lang_splatting_amd import losses
    from online_lang_splatting_amd.frame_shard import FrameLanes, GradLayout, GradientBucket
    from online_lang_splatting_amd.slam_iterations import MappingStep
    F = 15
    s = _case(F)
    dev = s.dev
    g = torch.Generator().manual_seed(5)
    targets = [(torch.rand(3, H, W, generator=g).to(dev), (torch.rand(H, W, generator=g) * 4).to(dev),
                (torch.randn(F, 48, 48, generator=g) * 0.3).to(dev)) for _ in range(2)]
    params = dict(means3D=s.base["means3D"], shs=s.base["shs"], language=s.base["language"],
                  opacities=s.raw[0].clone(), scales=s.raw[1].clone(), rotations=s.raw[2].clone())
    lrs = dict(xyz=0.0, sh_dc=0.0, sh_rest=0.0, opacity=0.0, scale=0.0, rotation=0.0, language=0.0)
    lanes = FrameLanes(1, s.P, W, H, F, s.M, CAPACITY, dev)
    step = MappingStep(lanes, params, s.base["bg"], s.base["sh_degree"], s.cams, targets, lrs, activations=_abi.ACT_ALL,
                       fused_loss=fused_loss)
    step.iteration()
    got = step.summed_gradients()
    for k, raw in zip(("opacities", "scales", "rotations"), s.raw):
        assert torch.equal(params[k], raw), k                       # (rate 0: the parameters did not move)
    ws = _workspace(s)
    ref = GradientBucket(s.P, GradLayout(s.M, F), dev)
    ref.flat.fill_(7.0)
    for v in range(2):
        ws.set_scene(opacities=s.act_all[0], scales=s.act_all[1], rotations=s.act_all[2], activations=0, **s.cams[v], **s.base)
        out = ws.forward()
        lo = losses.mapping_loss(out["color"], out["depth"], out["language"], *targets[v])
        gu = ws.backward(lo["dL_dimage"], lo["dL_dlanguage"], lo["dL_ddepth"])
        to = lambda a, like: torch.from_numpy(np.ascontiguousarray(a)).reshape(like.shape).to(dev)  # noqa: E731
        chained = dict(gu)
        chained["dL_dopacity"] = to(A.opacity_chain(gu["dL_dopacity"], s.act_all[0]), gu["dL_dopacity"])
        chained["dL_dscales"] = to(A.scale_chain(gu["dL_dscales"], s.act_all[1]), gu["dL_dscales"])
        chained["dL_drotations"] = to(A.rotation_chain(gu["dL_drotations"], s.raw[2]), gu["dL_drotations"])
        ref.accumulate(chained, out["radii"], first=(v == 0))
    assert torch.equal(got, ref.flat)
    sl = GradLayout(s.M, F).slices()
    for k in ("opacity", "scales", "rotations", "sh", "language"):
        assert float(got[:, sl[k]].abs().max()) > 0, k


def test_activation_argument_errors(hip):
    """The checks the raw path's callers rely on: a raw opacity must reach the backward too, scale / rotation activations
    exclude a precomputed covariance, unknown bits are refused — by the frame entries and by the hook."""
    from online_lang_splatting_amd import _lib
    s = _case(0)
    ws = _workspace(s)
    kw = dict(**s.cams[0], **s.base)
    op, sc_, rot = s.raw
    ws.set_scene(opacities=op, scales=sc_, rotations=rot, activations=_abi.ACT_ALL, **kw)
    ws.forward()
    ws.set_scene(opacities=None, scales=sc_, rotations=rot, activations=OP, **kw)
    with pytest.raises(_lib.OlsrError, match=r"a raw \(pre-sigmoid\) opacity is needed by backward as well"):
        ws.backward(*s.cot[0])
    cov = torch.zeros(s.P, 6, device=s.dev)
    for bit in (SC, ROT, SC | ROT):
        ws.set_scene(opacities=s.act_all[0], scales=None, rotations=None, cov3D_precomp=cov, activations=bit, **kw)
        with pytest.raises(_lib.OlsrError, match="scale / rotation activations make no sense with a precomputed 3D covariance"):
            ws.forward()
    for bits in (8, 16 | OP, -1):
        ws.set_scene(opacities=op, scales=sc_, rotations=rot, activations=bits, **kw)
        with pytest.raises(_lib.OlsrError, match=r"activations holds unknown OLSR_ACT_\* bits"):
            ws.forward()
        with pytest.raises(_lib.OlsrError, match=r"activations holds unknown OLSR_ACT_\* bits"):
            _lib.debug_activate(bits, op, sc_, rot)
    L = _lib.lib()
    assert L.olsr_debug_activate(-1, 0, None, None, None, None, None, None, None) == _abi.OLSR_ERR_ARG
    assert L.olsr_debug_activate(0, _abi.ACT_ALL, None, None, None, None, None, None, None) == _abi.OLSR_OK
    # the workspace is as usable as before
    ws.set_scene(opacities=op, scales=sc_, rotations=rot, activations=_abi.ACT_ALL, **kw)
    ws.forward()
    assert not ws.rendered()[1]
