"""The mapping / tracking loss of csrc/olsr_loss_device.h + csrc/k_loss.hip restated in numpy, one rounding per operation, in
the header's order.  TEST INFRASTRUCTURE ONLY — the product never imports this module; no torch, no autograd.

The build uses -ffp-contract=off and the header writes no FMA, so with dtype=float32 every per-pixel value below is the value
the kernel holds, bit for bit: the three cotangent images, and the five unweighted terms each pixel adds to s[0..4] (|rgb|,
|depth|, |language|, dL/da, dL/db).  The one operation that is not IEEE-exact is expf(exposure[0]), which comes from the device's
libm: e^a is therefore an ARGUMENT (`ea`), and ea_candidates() lists the correctly rounded value and its two float32 neighbours —
one of them must make every output of a call match.

What the kernels do with the terms afterwards (thread, wave and block sums in float32, then doubles) depends on the launch
shape; the truth for the sums is the terms added in float64 (math.fsum: exact), weighted as loss_final_block weights them, and
the kernels are held to it by a derived bound (sum_bound()).

The depth term's weight is a parameter of its own, olsr_loss_params.one_minus_alpha: see loss_ref().

dtype=float64 evaluates the same statement in double (same decisions, same float32 bilinear weights): that form is what
tests/test_loss_ref_cpu.py holds to oracle/loss_oracle.py run in float64, to 1e-12.

The language target: t = ly0 (lx0 g00 + lx1 g01) + ly1 (lx0 g10 + lx1 g11) with the float32 weights of ATen's
area_pixel_compute_source_index.  `t64` is that sum in float64 over the SAME float32 weights and `mag` the same sum over
magnitudes: float32 t is within 4 roundings of t64 on every path (product, inner sum, product, outer sum), so the sign of
l - t can differ from the sign of l - t64 only where |l - t64| <= 5 * 2^-24 * mag (one more for the second-order terms).
"""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -24          # unit roundoff of float32
LANG_ROUNDINGS = 5      # 4 roundings on a path of the bilinear sum + 1 for second-order terms (derived above, not measured)


def bilinear_index(n_out, n_in):
    """bilinear_index of the header for dst = 0 .. n_out - 1: (i0, i1, l0, l1), indices int32, weights float32."""
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=F32)
    src = scale * (dst + F32(0.5)) - F32(0.5)
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int32), np.int32(n_in - 1))
    i1 = (i0 + (i0 < n_in - 1)).astype(np.int32)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def _sgn(v):
    """loss_sgn: 1, -1, or +0 (NaN -> 0)."""
    one = v.dtype.type(1)
    return np.where(v > 0, one, np.where(v < 0, -one, v.dtype.type(0))).astype(v.dtype)


def ea_candidates(exposure, initialization=False):
    """The float32 values expf(a) may be: the correctly rounded e^a and its two neighbours; 1.0 alone where it is exact."""
    if exposure is None or initialization:
        return [F32(1)]
    a = F32(np.asarray(exposure, dtype=F32).reshape(-1)[0])
    if a == 0:
        return [F32(1)]
    c = F32(np.exp(np.float64(a)))
    return [c, np.nextafter(c, F32(0)), np.nextafter(c, F32(np.inf))]


def _fsum(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if x.size and not np.isfinite(x).all():
        with np.errstate(all="ignore"):
            return float(np.sum(x))      # inf / NaN propagate as IEEE addition propagates them
    if x.size > (1 << 20):               # pairwise in float64: off by a few 2^-53 of the magnitudes, nothing beside 2^-24
        return float(np.sum(x))
    return math.fsum(x.tolist())


def loss_ref(image, depth, language, gt_image, gt_depth, gt_language=None, exposure=None, *, ea=None, tracking=False,
             opacity=None, grad_mask=None, alpha=0.95, thr=0.01, lamda=1.0, initialization=False, dtype=F32,
             depth_weight_from_float=False):
    """image [3,H,W], depth [1,H,W], language [F,H,W] or None, gt_image [3,H,W], gt_depth [H,W], gt_language [F,h,w] or None,
    exposure [2] or None (float32 arrays); tracking: opacity [1,H,W], grad_mask [H,W] or None, no language term.
    alpha: the caller's Python double.  The depth weight 1 - alpha is olsr_loss_params.one_minus_alpha = float32(1.0 - alpha)
    formed in double, as the Python wrappers (and the reference) form it; depth_weight_from_float: the field left 0 by a caller
    of the C ABI, for whom the library uses 1.f - float32(alpha).
    Returns a dict:
      d_image, d_depth, d_lang   the cotangents (dtype)
      terms                      list of the five per-pixel unweighted terms
      sums, mags                 float64[5]: the terms, and their magnitudes, added exactly
      loss, dexp                 float64[4], float64[2]: what loss_final_block forms from `sums`
      loss_mag, dexp_mag         the same weighted sums over magnitudes (S of sum_bound; loss_mag[0] is not used: the total's
                                 bound is the sum of its three terms' bounds)
      m, md                      the colour and depth masks, [H,W]
      t64, mag                   the language target in float64 over the float32 weights, and its magnitude sum (or None)."""
    T = np.dtype(dtype).type
    cv = lambda t: np.ascontiguousarray(np.asarray(t, dtype=F32)).astype(T)  # noqa: E731
    x, gt = cv(image), cv(gt_image)
    _, H, W = x.shape
    HW = H * W
    dz, gd = cv(depth).reshape(H, W), cv(gt_depth).reshape(H, W)
    use = exposure is not None and not initialization
    if use:
        e = np.asarray(exposure, dtype=F32).reshape(-1)
        ea_ = T(ea) if ea is not None else T(ea_candidates(exposure)[0])
        eb = T(e[1])
    else:
        ea_, eb = T(1), T(0)
    al, th, lam = T(F32(alpha)), T(F32(thr)), T(F32(lamda))
    oma32 = F32(F32(1) - F32(alpha)) if depth_weight_from_float else F32(1.0 - float(alpha))
    if oma32 == 0:   # loss_depth_weight(): a zero field means "derive"
        oma32 = F32(F32(1) - F32(alpha))
    out = {}
    with np.errstate(all="ignore"):
        # ---- RGB (loss_rgb_term; m, op and wrgb as k_loss.hip forms them)
        m = (((gt[0] + gt[1]) + gt[2]) > th).astype(T)
        op = np.ones((H, W), dtype=T)
        if tracking:
            op = cv(opacity).reshape(H, W)
            if grad_mask is not None:
                m = m * cv(grad_mask).reshape(H, W)
        wrgb = al / (T(3) * T(HW))
        ab = (ea_ * x + eb) if use else x
        v = ab * m - gt * m
        t0 = op * np.abs(v) if tracking else np.abs(v)
        dab = op * (_sgn(v) * m) if tracking else _sgn(v) * m
        t3 = dab * (ea_ * x)
        t4 = dab
        out["d_image"] = ((wrgb * dab) * ea_).astype(T)
        # ---- depth (loss_depth_term)
        md = (gd > T(F32(0.01))).astype(T)
        if tracking:
            md = md * (op > T(F32(0.95))).astype(T)
        wd = T(oma32) / T(HW)
        vd = dz * md - gd * md
        t1 = np.abs(vd)
        out["d_depth"] = ((wd * _sgn(vd)) * md).astype(T).reshape(1, H, W)
        # ---- language (bilinear_index, loss_lang_term)
        Fc = 0 if (language is None or tracking) else int(np.asarray(language).shape[0])
        t2 = np.zeros((Fc, H, W), dtype=T)
        out["d_lang"] = np.zeros((Fc, H, W), dtype=T)
        out["t64"] = out["mag"] = None
        has_lang = Fc > 0 and gt_language is not None
        if has_lang:
            lg, g = cv(language), cv(gt_language)
            lh, lw = g.shape[1], g.shape[2]
            y0, y1, ly0, ly1 = bilinear_index(H, lh)
            x0, x1, lx0, lx1 = bilinear_index(W, lw)
            g00, g01 = g[:, y0][:, :, x0], g[:, y0][:, :, x1]
            g10, g11 = g[:, y1][:, :, x0], g[:, y1][:, :, x1]
            wy0, wy1 = ly0.astype(T)[None, :, None], ly1.astype(T)[None, :, None]
            wx0, wx1 = lx0.astype(T)[None, None, :], lx1.astype(T)[None, None, :]
            t = wy0 * (wx0 * g00 + wx1 * g01) + wy1 * (wx0 * g10 + wx1 * g11)
            vl = lg - t
            t2 = np.abs(vl)
            wl = lam / (T(Fc) * T(HW))
            out["d_lang"] = (wl * _sgn(vl)).astype(T)
            out["wl"] = wl
            D = np.float64
            Y0, Y1, X0, X1 = (w.astype(D) for w in (wy0, wy1, wx0, wx1))
            A, B, C_, D_ = (q.astype(D) for q in (g00, g01, g10, g11))
            out["t64"] = Y0 * (X0 * A + X1 * B) + Y1 * (X0 * C_ + X1 * D_)
            out["mag"] = Y0 * (np.abs(X0 * A) + np.abs(X1 * B)) + Y1 * (np.abs(X0 * C_) + np.abs(X1 * D_))
        terms = [t0, t1, t2, t3, t4]
        out["m"], out["md"] = m, md
        out["terms"] = terms
        sums = np.array([_fsum(t) for t in terms])
        mags = np.array([_fsum(np.abs(t)) for t in terms])
        a64, l64, hw = float(F32(alpha)), float(F32(lamda)), float(H) * float(W)

        def weigh(s):
            l_rgb = a64 * s[0] / (3.0 * hw)
            l_depth = float(oma32) * s[1] / hw
            l_lang = l64 * s[2] / (float(Fc) * hw) if has_lang else 0.0
            dexp = [a64 * s[3] / (3.0 * hw), a64 * s[4] / (3.0 * hw)] if use else [0.0, 0.0]
            return np.array([l_rgb + l_depth + l_lang, l_rgb, l_depth, l_lang]), np.array(dexp)
        out["sums"], out["mags"] = sums, mags
        out["loss"], out["dexp"] = weigh(sums)
        out["loss_mag"], out["dexp_mag"] = weigh(mags)
    out["use_exposure"], out["has_lang"], out["F"], out["one_minus_alpha"] = use, has_lang, Fc, oma32
    return out


def f32_bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32)


def same_bits(a, b):
    """Bit equality of two float32 arrays, the sign of zero included; any NaN equals any NaN."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(f32_bits(a)[~na], f32_bits(b)[~nb]))


def sum_bound(D, S, truth):
    """|got - truth| for a float32 result whose terms (magnitude sum S, already weighted) pass through at most D float32
    additions before the doubles: each addition perturbs the partial sum it forms by at most 2^-24 relative, so the sum is off
    by at most ((1 + u)^D - 1) S <= (D + 2) u S (the 2 covers the second-order terms, for D <= 2^10, and the doubles), and the
    result is rounded to float32 once."""
    b = (D + 2) * U * S
    return b + U * (abs(truth) + b)


def rounding_units(got, truth, S):
    """|got - truth| in units of 2^-24 S (what sum_bound's D + 2 bounds, before the result's own rounding)."""
    return abs(float(got) - float(truth)) / (U * S) if S > 0 else 0.0


def adds_standalone(F, vec4):
    """D of mapping_loss_kernel per sum s[0..4]: a thread adds its pixels' terms one after the other to s[k] (3 colour terms,
    1 depth term, F language terms, 3 and 3 exposure terms per pixel, VEC pixels), wave_sum is six levels of v += shfl_xor,
    and thread k adds the four waves' values: v = 0; v += red[0..3] — the first of those is exact, three round."""
    vec = 4 if vec4 else 1
    return [n * vec + 6 + 3 for n in (3, 1, max(F, 1), 3, 3)]


def adds_epilogue(F):
    """D of the fused epilogue (k_render_fwd.hip): one pixel per thread, so 3 / 1 / F / 3 / 3 sequential adds, the same
    six-level wave_sum, and ((w0 + w1) + w2) + w3: three adds."""
    return [n + 6 + 3 for n in (3, 1, max(F, 1), 3, 3)]


def check_sums(got_loss, got_dexp, ref, D, label="", only=None):
    """Holds loss[0..3] and dL_dexposure[0..1] to `ref` (a loss_ref() result) by sum_bound with the per-sum depths D[0..4].
    Non-finite truths must be met exactly (inf by the same inf, NaN by NaN).  only: the names to hold, of rgb, depth, lang,
    d_a, d_b, total (default: all).  Returns the observed errors in rounding units
    {name: units}; raises AssertionError with the figures otherwise."""
    got_loss = np.asarray(got_loss, dtype=np.float64).reshape(-1)
    got_dexp = np.asarray(got_dexp, dtype=np.float64).reshape(-1)
    lm, dm = ref["loss_mag"], ref["dexp_mag"]
    rows = [("rgb", got_loss[1], ref["loss"][1], lm[1], D[0]), ("depth", got_loss[2], ref["loss"][2], lm[2], D[1]),
            ("lang", got_loss[3], ref["loss"][3], lm[3], D[2]), ("d_a", got_dexp[0], ref["dexp"][0], dm[0], D[3]),
            ("d_b", got_dexp[1], ref["dexp"][1], dm[1], D[4])]
    units, total_bound = {}, 0.0
    for name, got, truth, S, d in rows:
        if only is not None and name not in only:
            continue
        if not np.isfinite(truth):
            assert (np.isnan(got) and np.isnan(truth)) or got == truth, f"{label} {name}: {got} for {truth}"
            units[name] = float("nan")
            continue
        assert np.isfinite(got), f"{label} {name}: {got} for the finite {truth}"
        b = sum_bound(d, S, truth)
        units[name] = rounding_units(got, truth, S)
        assert abs(got - truth) <= b, f"{label} {name}: |{got!r} - {truth!r}| > {b:.3e} ({units[name]:.2f} units, D + 2 = {d + 2})"
        if name in ("rgb", "depth", "lang"):
            total_bound += (d + 2) * U * S
    truth = ref["loss"][0]
    if only is not None and "total" not in only:
        return units
    if not np.isfinite(truth):
        assert (np.isnan(got_loss[0]) and np.isnan(truth)) or got_loss[0] == truth, f"{label} total: {got_loss[0]} for {truth}"
        units["total"] = float("nan")
    else:
        assert np.isfinite(got_loss[0]), f"{label} total: {got_loss[0]} for the finite {truth}"
        b = total_bound + U * (abs(truth) + total_bound)
        units["total"] = abs(got_loss[0] - truth) / (U * float(lm[0])) if lm[0] > 0 else 0.0
        assert abs(got_loss[0] - truth) <= b, f"{label} total: |{got_loss[0]!r} - {truth!r}| > {b:.3e}"
    return units


def located_lang_flips(d_lang, language, ref):
    """The language cotangent against sign(l - t64) * wl: returns the number of elements that differ, after asserting that
    every one of them lies where |l - t64| <= LANG_ROUNDINGS * 2^-24 * mag (no cap on their number, none anywhere else)."""
    d = np.asarray(d_lang, dtype=F32)
    if not ref["has_lang"]:
        assert not d.size or (f32_bits(d) == 0).all(), "language cotangent must be +0 without a target"
        return 0
    l64 =np.asarray(language, dtype=F32).astype(np.float64)
    diff = l64 - ref["t64"]
    want_sign = np.sign(diff)
    got_sign = np.sign(d.astype(np.float64))
    assert np.isin(np.abs(d), [F32(0), F32(ref["wl"])]).all(), "a language cotangent is neither 0 nor +-wl"
    nan = np.isnan(diff)                                  # loss_sgn(NaN) = 0: a poisoned element's cotangent is +0
    assert (f32_bits(d)[nan] == 0).all(), "a NaN language element must have the cotangent +0"
    differ = (got_sign != want_sign) & ~nan
    near =np.abs(diff) <= LANG_ROUNDINGS * U * ref["mag"]
    assert not (differ & ~near).any(), (
        f"{int((differ & ~near).sum())} language cotangents differ from sign(l - t64) away from a rounding tie")
    return int(differ.sum())


def load_cases(name):
    """The cases of tests/golden/<name>.npz as (id, tracking, {key: array}), mapping cases first."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    out = []
    for tag, n in (("c", int(z["n_cases"])), ("t", int(z["n_tracking_cases"]))):
        for i in range(n):
            pre = f"{tag}{i}_"
            out.append((f"{name}-{tag}{i}", tag == "t", {k[len(pre):]: np.asarray(z[k]) for k in z.files if k.startswith(pre)}))
    return out


def ref_for_case(c, tracking, ea=None, dtype=F32, exposure=True, depth_weight_from_float=False):
    """loss_ref() on a golden case (load_cases()); exposure=False: the entry called with exposure=None."""
    expo = np.array([c["a"].reshape(-1)[0], c["b"].reshape(-1)[0]], dtype=F32) if exposure else None
    kw = dict(ea=ea, alpha=float(c["alpha"]), thr=float(c["thr"]), dtype=dtype, depth_weight_from_float=depth_weight_from_float)
    if tracking:
        return loss_ref(c["image"], c["depth"], None, c["gt_image"], c["gt_depth"], None, expo, tracking=True,
                        opacity=c["opacity"], grad_mask=c["grad_mask"], **kw)
    return loss_ref(c["image"], c["depth"], c["lang"], c["gt_image"], c["gt_depth"], c["gt_lang"], expo, lamda=1.0,
                    initialization=bool(int(c["init"])), **kw)


def pin(got, args, kw, D, label="", only=None):
    """One call of a loss entry held to the restatement.  got: dict(loss, dL_dimage, dL_ddepth, dL_dlanguage or None,
    dL_dexposure) as numpy arrays; args, kw: the positional and keyword arguments of loss_ref() for the same inputs (without
    `ea`); D: the per-sum addition depths (adds_standalone / adds_epilogue); only: as check_sums takes it.
    Tries the e^a candidates in turn: one must make all three cotangents equal to the restatement bit for bit (the sign of zero
    included) AND put every sum within sum_bound; then locates the language flips against t64.
    Returns dict(candidate index, ea, units, flips) and prints it as one line."""
    exposure, init = args[6] if len(args) > 6 else None, kw.get("initialization", False)
    cands = ea_candidates(exposure, init)
    d_lang = got.get("dL_dlanguage")
    report, why = None, []
    for i, ea in enumerate(cands):
        ref = loss_ref(*args, ea=ea, **kw)
        pairs = [("dL_dimage", "d_image"), ("dL_ddepth", "d_depth")] + ([("dL_dlanguage", "d_lang")] if d_lang is not None else [])
        bad = {}
        for g, r in pairs:   # {output: number of elements whose bits differ}
            a = np.asarray(got[g], dtype=F32)
            assert a.size == ref[r].size, f"{label}: {g} has {a.size} elements, expected {ref[r].size}"
            if not same_bits(a.reshape(ref[r].shape), ref[r]):
                bad[g] = int((f32_bits(a).reshape(-1) != f32_bits(ref[r]).reshape(-1)).sum())
        if bad:
            why.append((float(ea), bad))
            continue
        try:
            units = check_sums(got["loss"], got["dL_dexposure"], ref, D, label, only)
        except AssertionError as e:
            why.append((float(ea), str(e)))
            continue
        flips = located_lang_flips(d_lang, args[2], ref) if d_lang is not None else 0
        report = dict(candidate=i, ea=float(ea), units=units, flips=flips, ref=ref)
        break
    assert report is not None, f"{label}: no e^a candidate makes every output match: {why}"
    worst = {k: round(float(v), 2) for k, v in report["units"].items()}
    print(f"[loss pinned] {label}: e^a candidate {report['candidate']} of {len(cands)} ({report['ea']!r}); sum errors in 2^-24 S "
          f"{worst} against D + 2 = {[d + 2 for d in D]}; located language flips {report['flips']}")
    return report
