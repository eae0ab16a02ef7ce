"""olsr_ss_encoder_encode / olsr_ss_query_sims (HIP) and lang_single_stage's SingleStageEncoder, SingleStageQuery and
SingleStageTargets on the GPU: the language side of a `single_stage_ae: True` configuration.

Yardstick: the suite's rule for these nets, imported unchanged (tests/test_gpu_lang_codec._ratio_rule, the encoder test's
helper, and lang_query_ref.tolerance for discrete decisions).  With `truth` the float64 and `ref32` the float32 evaluation of
the reference's statements (tests/golden/lang_single_stage.npz, recorded from the reference's module;
tests/lang_single_stage_ref.py, which tests/test_lang_single_stage_ref_golden.py pins to that file, for the other sizes):
    max and rms of |hip - truth| <= max(4 x the same of ref32, 4 * 2^-24 max|truth|)
Everything else is exact: the two input layouts, the two code layouts, tiles of a call against calls on the tiles, repeated
runs, relevancy against localise(similarities), add_keyframe_hr against encode agree bit for bit, and a NaN row or pixel
leaves every other row's bits as they were.  The references of a size are computed once (REFS) and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import lang_query_ref as RQ
import lang_single_stage_ref as R
from test_gpu_lang_codec import _ratio_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
THRESH = 0.5
REFS = {}


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _state():
    if "state" not in REFS:
        REFS["state"] = R.module_state(SEED)
    return REFS["state"]


def _rows130():
    """(features [130,768], truth [130,15], ref32), computed once."""
    if "rows130" not in REFS:
        x = R.make_features(130, SEED)
        REFS["rows130"] = (x, R.encode(_state()[0], x, torch.float64), R.encode(_state()[0], x, torch.float32))
    return REFS["rows130"]


def _encoder(state=None):
    from online_lang_splatting_amd.lang_single_stage import SingleStageEncoder
    state = _state()[0] if state is None else state
    enc = SingleStageEncoder(DEV, state)
    assert torch.equal(enc.flat.cpu(), R.flatten_encoder(state)) and enc.eps == R.BN_EPS
    return enc


def _decoder(state=None):
    from online_lang_splatting_amd.lang_single_stage import SingleStageDecoder
    state = _state()[1] if state is None else state
    dec = SingleStageDecoder(DEV, state)
    assert torch.equal(dec.flat.cpu(), R.flatten_decoder(state))
    return dec


def _planes(rows, pad=0):
    """[N,768] on the CPU -> the same data as a channel-major [768,1,N] tensor on the device whose planes are N + pad apart."""
    N = rows.shape[0]
    buf = torch.full((768, N + pad), float("nan"), device=DEV)
    buf[:, :N] = rows.t().to(DEV)
    return buf.as_strided((768, 1, N), (N + pad, N, 1))


def _query(case):
    from online_lang_splatting_amd.lang_single_stage import SingleStageQuery
    q = SingleStageQuery(_decoder(case["dec_state"]))
    assert q.thresh == THRESH
    q.set_phrases(case["pos"].to(DEV), case["neg"].to(DEV))
    q.set_labels(None if case["labels"] is None else case["labels"].to(DEV))
    return q


def _raw_sims(dec, codes, phrases, decode_hw=None):
    """olsr_ss_query_sims itself (any K from 1): codes [15,h,w] and phrases [K,768] on the device -> [K,h',w']."""
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd._lib import check, lib
    h, w = codes.shape[1:]
    dh, dw = (h, w) if decode_hw is None else decode_hw
    K = phrases.shape[0]
    p = _abi.OlsrLangQueryParams(n_widths=len(_abi.SS_DECODER_WIDTHS), K=K, n_pos=0, n_labels=0, in_width=w, in_height=h,
                                 dec_width=dw, dec_height=dh, out_width=dw, out_height=dh, thresh=THRESH, flags=0)
    for k, v in enumerate(_abi.SS_DECODER_WIDTHS):
        p.widths[k] = v
    sims = torch.empty(K, dh, dw, device=DEV)
    check(lib().olsr_ss_query_sims(C.byref(p), codes.data_ptr(), dec.flat.data_ptr(), phrases.data_ptr(), sims.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return sims


def _map_case(h, w):
    """(codes [15,h,w], decoder state, 64 unit phrase rows, {K: (truth, ref32)}) of a map size, computed once."""
    key = ("map", h, w)
    if key not in REFS:
        codes, _ = RQ.make_codes(h, w, SEED + h)
        dec_state, phrases = _state()[1], RQ.unit_rows(64, SEED + h)
        t = [R.similarities(codes, dec_state, phrases, dt) for dt in (torch.float64, torch.float32)]
        REFS[key] = (codes, dec_state, phrases, t)
    return REFS[key]


# ---- the golden cases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(R.ENCODE_CASES))
def test_golden_encode(hip, key):
    z = R.golden()
    state, _ = R.make_encode_case(key)
    x = torch.from_numpy(z[f"{key}_features"])
    out = _encoder(state).encode(x.to(DEV), layout="rows").cpu()
    assert tuple(out.shape) == z[f"{key}_out_f64"].shape
    _ratio_rule(f"golden {key}", out, torch.from_numpy(z[f"{key}_out_f64"]), torch.from_numpy(z[f"{key}_out_f32"]))


def test_golden_decode(hip):
    z = R.golden()
    dec_state, _, _ = R.make_decode_case()
    rows, phrases = torch.from_numpy(z["decode_codes"]), torch.from_numpy(z["decode_phrases"])
    dec = _decoder(dec_state)
    sims = _raw_sims(dec, rows.t().contiguous().view(15, 1, -1).to(DEV), phrases.to(DEV)).cpu()[:, 0]
    _ratio_rule("golden similarities", sims, torch.from_numpy(z["decode_sims_f64"]), torch.from_numpy(z["decode_sims_f32"]))
    # the recorded 768-wide rows, through the products with the unit vectors of their own directions: <decode(c), f / |f|> = 1
    kept = [int(k) for k in z["decode_kept"]]
    f64 = torch.from_numpy(z["decode_features_f64"])
    own = _raw_sims(dec, rows[kept].t().contiguous().view(15, 1, -1).to(DEV), f64.float().contiguous().to(DEV)).cpu()[:, 0]
    truth = torch.mm(f64, f64.float().double().T).T
    ref32 = torch.mm(torch.from_numpy(z["decode_features_f32"]), f64.float().T).T
    _ratio_rule("golden features against themselves", own, truth, ref32)


# ---- the encoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
def test_encoder_sizes_in_both_layouts(hip, N):
    x, t64, t32 = _rows130()
    enc = _encoder()
    rows = enc.encode(x[:N].to(DEV), layout="rows").cpu().clone()
    assert tuple(rows.shape) == (N, 15)
    _ratio_rule(f"N = {N} rows", rows, t64[:N], t32[:N])
    chan = enc.encode(_planes(x[:N]), layout="rows").cpu().clone()
    _ratio_rule(f"N = {N} channels", chan, t64[:N], t32[:N])
    assert torch.equal(rows, chan)   # the layouts fill the same LDS image: the same bits
    assert float((rows.double().norm(dim=1) - 1).abs().max()) <= 2.0 ** -23
    # [15,N] and [N,15] are bitwise transposes
    assert torch.equal(enc.encode(x[:N].to(DEV), layout="channels").cpu(), rows.t())
    assert torch.equal(enc.encode(x[:N].to(DEV)).cpu(), rows.t())   # "channels" is the default: the target's layout


def test_unaligned_planes(hip):
    """N = 117, plane_stride = 121, and a map that starts one float into its allocation: no plane is 16-byte aligned."""
    N, stride = 117, 121
    x, t64, t32 = _rows130()
    enc = _encoder()
    want = enc.encode(x[:N].to(DEV), layout="rows").cpu().clone()
    buf = torch.full((1 + 768 * stride,), float("nan"), device=DEV)
    off = buf[1:].view(768, stride)
    off[:, :N] = x[:N].t().to(DEV)
    assert off.data_ptr() % 16 == 4
    got = enc.encode(off.as_strided((768, 1, N), (stride, N, 1), 1), layout="rows").cpu()
    _ratio_rule(f"N = {N}, plane stride {stride}, base + 4 bytes", got, t64[:N], t32[:N])
    assert torch.equal(got, want)


def test_batch_of_two(hip):
    x, t64, t32 = _rows130()
    xb = x[:70].view(2, 5, 7, 768).permute(0, 3, 1, 2).contiguous()
    assert tuple(xb.shape) == (2, 768, 5, 7)
    enc = _encoder()
    out = enc.encode(xb.to(DEV), layout="rows").cpu().clone()
    assert tuple(out.shape) == (2, 35, 15)
    _ratio_rule("[2,768,5,7]", out.reshape(70, 15), t64[:70], t32[:70])
    chan = enc.encode(xb.to(DEV)).cpu().clone()
    assert tuple(chan.shape) == (2, 15, 35) and torch.equal(chan.transpose(1, 2), out)
    for b in range(2):
        assert torch.equal(enc.encode(xb[b].to(DEV), layout="rows").cpu(), out[b])
        assert torch.equal(enc.encode(xb[b:b + 1].to(DEV), layout="rows").cpu(), out[b])


def test_rows_do_not_depend_on_their_tile_and_runs_repeat(hip):
    x, _, _ = _rows130()
    enc = _encoder()
    xd = x.to(DEV)
    whole = enc.encode(xd, layout="rows").clone()
    assert torch.equal(enc.encode(xd, layout="rows"), whole)                          # repeatability
    assert torch.equal(enc.encode(xd[:64].contiguous(), layout="rows"), whole[:64])
    assert torch.equal(enc.encode(xd[64:].contiguous(), layout="rows"), whole[64:])   # the same pixels at another offset of a tile
    assert torch.equal(enc.encode(xd[3:70].contiguous(), layout="rows"), whole[3:70])
    chan = _planes(x)
    assert torch.equal(enc.encode(chan).clone(), enc.encode(chan))
    mine = torch.empty(130, 15, device=DEV)   # a caller's buffer is written in place and returned
    assert enc.encode(xd, layout="rows", out=mine) is mine and torch.equal(mine, whole)


def test_nan_row_stays_in_its_row(hip):
    x, _, _ = _rows130()
    enc = _encoder()
    clean = enc.encode(x.to(DEV), layout="rows").clone()
    for bad_row, bad_col in ((5, 0), (64, 767), (129, 100)):
        xb = x.clone()
        xb[bad_row, bad_col] = float("nan")
        for feats in (xb.to(DEV), _planes(xb)):
            out = enc.encode(feats, layout="rows")
            assert bool(torch.isnan(out[bad_row]).all())
            keep = torch.arange(130, device=DEV) != bad_row
            assert torch.equal(out[keep], clean[keep])


# ---- the query -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 7, 17, 64])
@pytest.mark.parametrize("h,w", [(24, 40), (33, 31)])
def test_query_sims(hip, h, w, K):
    """960 pixels = 15 tiles of 64 and 1023 = 16 tiles less one pixel; K = 1, 7 (one phrase tile), 17 (two), 64 (four)."""
    codes, dec_state, phrases, (t64, t32) = _map_case(h, w)
    dec = _decoder(dec_state)
    sims = _raw_sims(dec, codes.to(DEV), phrases[:K].contiguous().to(DEV))
    assert tuple(sims.shape) == (K, h, w)
    _ratio_rule(f"{w} x {h}, K = {K}", sims.cpu(), t64[:K], t32[:K])
    assert torch.equal(_raw_sims(dec, codes.to(DEV), phrases[:K].contiguous().to(DEV)), sims)


def test_query_resampled_codes(hip):
    """Codes 9 x 13 decoded at 11 x 7 (F.interpolate bilinear, align_corners=False, up along one axis and down the other)."""
    codes, _ = RQ.make_codes(9, 13, SEED + 2)
    dec_state, phrases = _state()[1], RQ.unit_rows(7, SEED + 2)
    sims = _raw_sims(_decoder(dec_state), codes.to(DEV), phrases.to(DEV), decode_hw=(11, 7)).cpu()
    t64, t32 = (R.similarities(codes, dec_state, phrases, dt, decode_hw=(11, 7)) for dt in (torch.float64, torch.float32))
    assert tuple(sims.shape) == tuple(t64.shape) == (7, 11, 7)
    _ratio_rule("9 x 13 decoded at 11 x 7", sims, t64, t32)
    case = R.make_query_case(9, 13, 5, 2, 0)
    q = _query(case)
    via = q.similarities(case["codes"].to(DEV), decode_hw=(11, 7))
    phr = torch.cat([case["pos"], case["neg"]]).contiguous().to(DEV)
    assert torch.equal(via, _raw_sims(q.decoder, case["codes"].to(DEV), phr, decode_hw=(11, 7)))


def test_nan_code_pixel_stays_in_its_pixel(hip):
    codes, dec_state, phrases, _ = _map_case(33, 31)
    dec = _decoder(dec_state)
    ph = phrases[:7].contiguous().to(DEV)
    clean = _raw_sims(dec, codes.to(DEV), ph).reshape(7, -1).clone()
    for pixel, channel in ((5, 0), (64, 14), (1022, 7)):
        cb = codes.clone()
        cb.view(15, -1)[channel, pixel] = float("nan")
        out = _raw_sims(dec, cb.to(DEV), ph).reshape(7, -1)
        assert bool(torch.isnan(out[:, pixel]).all())
        keep = torch.arange(33 * 31, device=DEV) != pixel
        assert torch.equal(out[:, keep], clean[:, keep])


def _check_query(label, case, q, out):
    """relevancy()'s outputs against the reference's statements: the continuous ones by the ratio rule, the mask and the labels
    wherever the truth's deciding value is further than the tolerance from its decision."""
    t64, t32 = (R.query(case, dt, THRESH) for dt in (torch.float64, torch.float32))
    hip = {k: v.cpu() for k, v in out.items()}
    for name in ("similarities", "relevancy", "smoothed", "blended"):
        ref = "sims" if name == "similarities" else name
        _ratio_rule(f"{label} {name}", hip[name], t64[ref], t32[ref])
    P, H, W = hip["relevancy"].shape
    tol = RQ.tolerance(t64["normed"], t32["normed"])
    for p in range(P):
        differs = hip["mask"][p] != t64["mask"][p]
        near = (t64["normed"][p] - THRESH).abs() <= tol
        print(f"{label} mask[{p}]: {int(differs.sum())} pixels differ, {int(near.sum())} of {H * W} lie within {tol:.3e} of the threshold")
        assert int((differs & ~near).sum()) == 0
        x, y = int(hip["coord"][p, 0]), int(hip["coord"][p, 1])
        assert 0.0 <= float(t64["score"][p] - t64["smoothed"][p, y, x]) <= RQ.tolerance(t64["smoothed"], t32["smoothed"])
    if case["labels"] is not None:
        differs = hip["labels"].long() != t64["labels"]
        near = t64["label_margin"].abs() <= RQ.tolerance(t64["sims"], t32["sims"])
        assert int((differs & ~near).sum()) == 0
    return hip


def test_relevancy_is_localise_of_similarities(hip):
    case = R.make_query_case(24, 40, 3, 3, 2)
    q = _query(case)
    codes = case["codes"].to(DEV)
    a = {k: v.clone() for k, v in q.relevancy(codes).items()}
    _check_query("40 x 24", case, q, a)
    sims = q.similarities(codes).clone()
    assert torch.equal(sims, a["similarities"])
    b = q.localise(sims)
    assert set(a) == set(b) and "labels" in a
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # up-sampled outputs: stage B at its own size from the same similarities
    c = {k: v.clone() for k, v in q.relevancy(codes, out_hw=(37, 53)).items()}
    d = q.localise(sims, out_hw=(37, 53))
    assert tuple(c["mask"].shape) == (3, 37, 53)
    for k in c:
        assert torch.equal(c[k], d[k]), k


def test_round_trip(hip):
    """768 -> 15 on the device, then the query's 15 -> 768 and the products with phrases made by decoding three of the codes,
    against the same chain restated in float64 and float32 (as test_gpu_lang_encoder.test_round_trip_through_the_query)."""
    from online_lang_splatting_amd.lang_single_stage import SingleStageQuery
    N = 70
    enc_state, dec_state = _state()
    x = R.make_features(N, SEED + 5)
    enc, dec = _encoder(), _decoder()
    codes = enc.encode(x.to(DEV)).clone()                       # [15,N]
    ref = [R.encode(enc_state, x, dt) for dt in (torch.float64, torch.float32)]
    _ratio_rule("round trip: codes", codes.cpu().t(), ref[0], ref[1])
    raw, _ = R.object_phrases(dec_state, ref[0][[3, 30, 64]].float(), 0)
    neg = RQ.unit_rows(4, SEED)
    q = SingleStageQuery(dec)
    q.set_phrases(raw.to(DEV), neg.to(DEV))
    sims = q.similarities(codes.view(15, 1, N)).cpu()
    t = [R.similarities(c.t().reshape(15, 1, N), dec_state, torch.cat([raw, neg]), dt) for c, dt in zip(ref, (torch.float64, torch.float32))]
    assert tuple(sims.shape) == tuple(t[0].shape) == (7, 1, N)
    _ratio_rule("round trip: similarities", sims, t[0], t[1])


def test_object_phrases_score_highest_on_their_own_pixels(hip):
    """Phrases made by decoding the three object codes of a 40 x 24 map (lang_query_ref.make_codes: a disc of one code each,
    5 % noise) score higher on every pixel of their own disc than on any other pixel.  With default initialisation the decoder
    sends all codes to nearly one direction, so the gap is small; the float64 evaluation's gap is asserted to be wider than
    twice the tolerance first, so that the claim is one float32 arithmetic can be held to (here: 3e-5 against 2.7e-6)."""
    from online_lang_splatting_amd.lang_single_stage import SingleStageQuery
    h, w = 24, 40
    dec_state = _state()[1]
    codes, obj = RQ.make_codes(h, w, SEED + 7)
    raw, _ = R.object_phrases(dec_state, obj[:3], 0)
    neg = RQ.unit_rows(4, SEED)
    q = SingleStageQuery(_decoder())
    q.set_phrases(raw.to(DEV), neg.to(DEV))
    sims = q.similarities(codes.to(DEV)).cpu().reshape(7, -1)
    t64, t32 = (R.similarities(codes, dec_state, torch.cat([raw, neg]), dt).reshape(7, -1) for dt in (torch.float64, torch.float32))
    _ratio_rule("object phrases: similarities", sims, t64, t32)
    tol = RQ.tolerance(t64, t32)
    for k in range(3):
        inside = (obj[k].double() @ codes.view(15, -1).double()) > 0.9      # the disc's pixels: the object's code and 5 % noise
        gap = float(t64[k, inside].min() - t64[k, ~inside].max())
        print(f"object {k}: {int(inside.sum())} pixels, the truth's gap to every other pixel {gap:.3e}, tolerance {tol:.3e}")
        assert 20 <= int(inside.sum()) <= 200 and gap > 2 * tol
        assert float(sims[k, inside].min()) > float(sims[k, ~inside].max())
        assert bool(inside[int(sims[k].argmax())])


# ---- consumers -------------------------------------------------------------------------------------------------------------
def test_query_evaluator_takes_a_single_stage_query(hip):
    import query_eval_ref as QE
    from online_lang_splatting_amd.query_eval import QueryEvaluator
    H, W = 33, 31
    case = R.make_query_case(H, W, 4, 3, 0)
    q = _query(case)
    codes = case["codes"].to(DEV)
    n_pos = 3
    gt = np.zeros((n_pos, H, W), np.uint8)
    for p in range(n_pos):
        gt[p, 4 + 5 * p:16 + 5 * p, 3 + 6 * p:15 + 6 * p] = 1
    boxes = np.float32([[0, 0, W - 1, H - 1], [0, 0, 3, 3], [W, H, W + 5, H + 5]])
    off = np.arange(n_pos + 1, dtype=np.int32)
    ev = QueryEvaluator(q)
    got = ev.evaluate(codes, torch.from_numpy(gt).to(DEV), torch.from_numpy(boxes).to(DEV), off)
    r = q.relevancy(codes)
    _check_query("31 x 33", case, q, r)
    want = QE.score_image(r["mask"].cpu().numpy(), r["smoothed"].cpu().numpy(), gt, boxes, off)
    for k in ("intersection", "union", "n_max", "hit"):
        assert got[k].tolist() == want[k].tolist(), k
    assert np.array_equal(got["mask_smoothed"].cpu().numpy(), want["mask_smoothed"])
    assert ev.summary()["images"] == 1 and got["hit"][0] == 1


def test_label_points_takes_a_single_stage_query(hip):
    from online_lang_splatting_amd.tsdf import label_points
    n = 130
    case = R.make_query_case(24, 40, 6, 3, 3)
    q = _query(case)
    feats = case["codes"].reshape(15, -1)[:, 200:200 + n].t().contiguous()   # [n,15] rows, as surface_points returns them
    got = label_points(q, feats.to(DEV))
    assert got.dtype == torch.int64 and tuple(got.shape) == (n,)
    sims = {dt: R.similarities(feats.t().reshape(15, 1, n), case["dec_state"], case["labels"], dt)[:, 0, :]
            for dt in (torch.float64, torch.float32)}
    want = torch.argmax(sims[torch.float64], dim=0)
    top = sims[torch.float64].T.topk(2, dim=-1).values
    margin = top[:, 0] - top[:, 1]
    tol = RQ.tolerance(sims[torch.float64], sims[torch.float32])
    differs = got.cpu() != want
    print(f"label_points n = {n}: {int(differs.sum())} labels differ from the float64 argmax; tolerance {tol:.3e}, smallest margin "
          f"{float(margin.min()):.3e}; labels used {sorted(set(want.tolist()))}")
    assert int((differs & (margin > tol)).sum()) == 0
    assert int((margin <= tol).sum()) <= max(1, n // 100)
    assert len(set(want.tolist())) > 1


def test_targets(hip):
    from online_lang_splatting_amd.lang_single_stage import SingleStageTargets
    h, w = 9, 13
    hr = R.make_features(h * w, SEED + 3).t().contiguous().view(1, 768, h, w).to(DEV)
    enc = _encoder()
    t = SingleStageTargets(enc, hw=(h, w))
    a = t.add_keyframe_hr("kf", hr)
    want = enc.encode(hr).clone()
    assert tuple(a.shape) == (15, h, w) and a.is_contiguous() and torch.equal(a, want.view(15, h, w))
    # the stored target is the object's own: the encoder's reusable buffer may be overwritten
    enc.encode(R.make_features(h * w, SEED + 4).to(DEV))
    assert torch.equal(t.targets["kf"], want.view(15, h, w))
    assert torch.equal(t.add_keyframe_hr("rows", hr[0].permute(1, 2, 0).reshape(-1, 768).contiguous()), a)
    b = t.add_keyframe("file", want)                     # labels from file: [15,h*w] or [15,h,w]
    assert torch.equal(b, a) and b.data_ptr() != want.data_ptr()
    t.rehearse(["kf", "file"])
    assert [x.data_ptr() for x in t.targets_for(["file", "kf"])] == [b.data_ptr(), a.data_ptr()]
    with pytest.raises(KeyError, match="never added"):
        t.rehearse(["kf", "missing"])
    with pytest.raises(RuntimeError, match="add_keyframe_hr"):
        t.add_keyframe_hr("bad", hr[:, :, :5].contiguous())
    with pytest.raises(RuntimeError, match="add_keyframe"):
        t.add_keyframe("bad", want[:14])
    assert "bad" not in t.targets


def test_add_keyframe_backbone_is_forward_then_add_keyframe_hr(hip):
    """The keyframe chain from the backbone's three maps: hr_net -> SingleStageEncoder -> the stored [15,h,w] target."""
    import hr_net_ref as RH
    from online_lang_splatting_amd.lang_single_stage import SingleStageTargets
    from test_gpu_hr_net import _dev, _net
    x = _dev(RH.make_inputs(((2, 3), (4, 6), (8, 12)), 22))
    net, enc = _net(), _encoder()
    a, b = SingleStageTargets(enc, hw=(16, 24)), SingleStageTargets(enc, hw=(16, 24))
    ta = a.add_keyframe_backbone("kf", *x, net)
    tb = b.add_keyframe_hr("kf", net.forward(*x))
    assert tuple(ta.shape) == (15, 16, 24) and torch.equal(ta, tb) and bool(torch.isfinite(ta).all())
    assert float((ta.double().norm(dim=0) - 1).abs().max()) <= 2.0 ** -23


def test_targets_at_the_keyframe_size(hip):
    """192 x 192 as the back end has it, [1,768,192,192] -> the [15,192,192] target, once."""
    from online_lang_splatting_amd.lang_single_stage import SingleStageTargets
    x = R.make_features(192 * 192, SEED + 2).t().contiguous().view(1, 768, 192, 192)
    t64, t32 = (R.encode(_state()[0], x, dt) for dt in (torch.float64, torch.float32))
    target = SingleStageTargets(_encoder()).add_keyframe_hr(0, x.to(DEV))
    assert tuple(target.shape) == (15, 192, 192)
    _ratio_rule("192 x 192", target.cpu().view(15, -1).t(), t64, t32)


def test_errors_are_raised_not_copied(hip):
    x, _, _ = _rows130()
    enc = _encoder()
    xd = x[:70].to(DEV)
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        enc.encode(x[:70])
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        enc.encode(xd.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        enc.encode(xd.t().contiguous().t())
    with pytest.raises(RuntimeError, match="plane must be contiguous"):
        enc.encode(xd.view(7, 10, 768).permute(2, 0, 1))           # [768,7,10] with the channel fastest
    with pytest.raises(RuntimeError, match="expected"):
        enc.encode(xd[:, :512].contiguous())
    with pytest.raises(RuntimeError, match="out must be"):
        enc.encode(xd, out=torch.empty(70, 15, device=DEV))         # the default layout is [15,70]
    with pytest.raises(RuntimeError, match="layout must be"):
        enc.encode(xd, layout="planes")
    case = R.make_query_case(9, 13, 5, 2, 0)
    q = _query(case)
    codes = case["codes"].to(DEV)
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        q.relevancy(case["codes"])
    with pytest.raises(RuntimeError, match=r"expected \[15,h,w\]"):
        q.similarities(codes[:14])
    from online_lang_splatting_amd.lang_single_stage import SingleStageQuery
    with pytest.raises(RuntimeError, match="set_phrases first"):
        SingleStageQuery(q.decoder).similarities(codes)
