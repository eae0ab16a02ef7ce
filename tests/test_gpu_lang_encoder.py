"""olsr_lang_encoder_encode (HIP), lang_encoder.LanguageEncoder and OnlineLanguageTargets.add_keyframe_hr on the GPU.

Yardstick: the project's own, imported unchanged from tests/test_gpu_lang_codec.py.  With `truth` the float64 and `ref32`
the float32 evaluation of the reference's statements (tests/golden/lang_encoder.npz, recorded from the reference's module;
tests/lang_encoder_ref.py, which tests/test_lang_encoder_ref_golden.py pins to that file, for the other sizes):
    max and rms of |hip - truth| <= max(4 x the same of ref32, 4 * 2^-24 max|truth|)
Why 4x fits was measured on the CPU when the cases were designed: with this BatchNorm state, BatchNorm as alpha h + beta and
every layer accumulated in k chunks of 4, 16 and 64, at N = 4096 and N = 70, the max error was 6.0e-8 .. 1.08e-7 against
ref32's 1.17e-7 .. 1.25e-7 and the rms 1.5e-8 .. 2.0e-8 against 2.2e-8: ratios 0.48 - 0.93.  Every figure is printed.

Everything else is exact: the two input layouts, tiles of a call against calls on the tiles, repeated runs, the fused codes
against OnlineLanguageCodec.encode, and add_keyframe_hr against encode followed by add_keyframe agree bit for bit.
The float64 / float32 references of a size are computed once (REFS) and shared.
"""
import ctypes as C

import pytest
import torch

import lang_codec_ref as RC
import lang_encoder_ref as R
import lang_query_ref as RQ
from test_gpu_lang_codec import _raises_exactly, _ratio_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 11
GUARD = -7.5          # fills the guard words around an output
REFS = {}


def _state():
    if "state" not in REFS:
        REFS["state"] = R.encoder_state(SEED)
    return REFS["state"]


def _reference(key, make):
    """(features, truth, ref32) of a case, computed once."""
    if key not in REFS:
        x = make()
        REFS[key] = (x, R.encode(_state(), x, torch.float64), R.encode(_state(), x, torch.float32))
    return REFS[key]


def _rows257():
    return _reference("rows257", lambda: R.make_features(257, SEED))


def _encoder(state=None):
    from online_lang_splatting_amd.lang_encoder import LanguageEncoder
    state = _state() if state is None else state
    enc = LanguageEncoder(DEV, state)
    assert torch.equal(enc.flat.cpu(), R.flatten(state)) and enc.eps == R.BN_EPS
    return enc


def _codec(seed=0):
    from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec
    c = OnlineLanguageCodec(DEV, seed=0)
    c.load_state_dict(RC.unflatten(RC.initial_params(seed)))
    return c


def _planes(rows, pad=0):
    """[N,768] on the CPU -> the same data as a channel-major [768,1,N] tensor on the device whose planes are N + pad apart."""
    N = rows.shape[0]
    buf = torch.full((768, N + pad), float("nan"), device=DEV)
    buf[:, :N] = rows.t().to(DEV)
    return buf.as_strided((768, 1, N), (N + pad, N, 1))


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_golden(hip, key):
    z = R.golden()
    state, _ = R.make_case(key)
    x = torch.from_numpy(z[f"{key}_features"])
    out = _encoder(state).encode(x.to(DEV)).cpu()
    assert tuple(out.shape) == z[f"{key}_out_f64"].shape
    _ratio_rule(f"golden {key}", out, torch.from_numpy(z[f"{key}_out_f64"]), torch.from_numpy(z[f"{key}_out_f32"]))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 70, 257])
def test_sizes_in_both_layouts(hip, N):
    x, t64, t32 = _rows257()
    enc = _encoder()
    rows = enc.encode(x[:N].to(DEV)).cpu().clone()
    assert tuple(rows.shape) == (N, 32)
    _ratio_rule(f"N = {N} rows", rows, t64[:N], t32[:N])
    chan = enc.encode(_planes(x[:N])).cpu().clone()
    _ratio_rule(f"N = {N} channels", chan, t64[:N], t32[:N])
    # the layouts fill the same LDS image: the same bits
    assert torch.equal(rows, chan)
    assert float((rows.double().norm(dim=1) - 1).abs().max()) <= 2.0 ** -23


@pytest.mark.parametrize("N", [1, 65, 257])
def test_unaligned_planes(hip, N):
    """plane_stride = N + 3, and a map that starts one float into its allocation: no plane is 16-byte aligned."""
    x, t64, t32 = _rows257()
    enc = _encoder()
    want = enc.encode(x[:N].to(DEV)).cpu().clone()
    padded = _planes(x[:N], pad=3)
    assert padded.stride(0) == N + 3
    got = enc.encode(padded).cpu().clone()
    _ratio_rule(f"N = {N}, plane stride N + 3", got, t64[:N], t32[:N])
    assert torch.equal(got, want)
    buf = torch.full((1 + 768 * (N + 3),), float("nan"), device=DEV)
    off = buf[1:].view(768, N + 3)
    off[:, :N] = x[:N].t().to(DEV)
    assert off.data_ptr() % 16 == 4
    assert torch.equal(enc.encode(off.as_strided((768, 1, N), (N + 3, N, 1), 1)).cpu(), want)


def test_batch(hip):
    x, t64, t32 = _reference("batch", lambda: R.make_features(70, SEED + 1).view(2, 5, 7, 768).permute(0, 3, 1, 2).contiguous())
    assert tuple(x.shape) == (2, 768, 5, 7)
    enc = _encoder()
    out = enc.encode(x.to(DEV)).cpu().clone()
    assert tuple(out.shape) == (70, 32)
    _ratio_rule("[2,768,5,7]", out, t64, t32)
    for b in range(2):
        assert torch.equal(enc.encode(x[b].to(DEV)).cpu(), out[35 * b:35 * (b + 1)])
        assert torch.equal(enc.encode(x[b:b + 1].to(DEV)).cpu(), out[35 * b:35 * (b + 1)])


def test_keyframe_size(hip):
    """192 x 192 as the back end has it, [1,768,192,192], once."""
    x, t64, t32 = _reference("192", lambda: R.make_features(192 * 192, SEED + 2).t().contiguous().view(1, 768, 192, 192))
    out = _encoder().encode(x.to(DEV)).cpu()
    assert tuple(out.shape) == (192 * 192, 32)
    _ratio_rule("192 x 192", out, t64, t32)


def test_rows_do_not_depend_on_their_tile_and_runs_repeat(hip):
    x, _, _ = _rows257()
    enc = _encoder()
    xd = x[:130].to(DEV)
    whole = enc.encode(xd).clone()
    assert torch.equal(enc.encode(xd), whole)                          # repeatability
    assert torch.equal(enc.encode(xd[:64].contiguous()), whole[:64])
    assert torch.equal(enc.encode(xd[64:].contiguous()), whole[64:])
    chan = _planes(x[:130])
    assert torch.equal(enc.encode(chan).clone(), enc.encode(chan))
    # a caller's buffer is written in place and returned
    mine = torch.empty(130, 32, device=DEV)
    assert enc.encode(xd, out=mine) is mine and torch.equal(mine, whole)


def _raw(enc, N, x, layout, stride, online, feat, codes, code_layout):
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd._lib import check, lib
    p = _abi.OlsrLangEncoderParams(n_widths=6, in_layout=layout, code_layout=code_layout, plane_stride=stride, bn_eps=enc.eps)
    for k, v in enumerate(_abi.LANG_ENCODER_WIDTHS):
        p.widths[k] = v
    check(lib().olsr_lang_encoder_encode(C.byref(p), N, x.data_ptr(), enc.flat.data_ptr(), online, feat, codes,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))


@pytest.mark.parametrize("N", [1, 65, 130])
@pytest.mark.parametrize("code_layout", [0, 1])
def test_nothing_is_written_outside_the_outputs(hip, N, code_layout):
    from online_lang_splatting_amd import _abi
    x, _, _ = _rows257()
    enc, codec = _encoder(), _codec()
    xd = x[:N].to(DEV)
    pad = 1024
    f_all = torch.full((pad + N * 32 + pad,), GUARD, device=DEV)
    c_all = torch.full((pad + N * 15 + pad,), GUARD, device=DEV)
    f, c = f_all[pad:pad + N * 32], c_all[pad:pad + N * 15]
    _raw(enc, N, xd, _abi.LANG_ENCODER_IN_ROWS, 0, codec.flat.data_ptr(), f.data_ptr(), c.data_ptr(), code_layout)
    for buf, n in ((f_all, N * 32), (c_all, N * 15)):
        assert bool((buf[:pad] == GUARD).all()) and bool((buf[pad + n:] == GUARD).all())
        assert not bool((buf[pad:pad + n] == GUARD).any())
    want = enc.encode(xd)
    assert torch.equal(f.view(N, 32), want)
    # either output alone gives the same bits and leaves the other untouched
    f2, c2 = torch.full_like(f_all, GUARD), torch.full_like(c_all, GUARD)
    _raw(enc, N, xd, _abi.LANG_ENCODER_IN_ROWS, 0, None, f2[pad:].data_ptr(), None, code_layout)
    _raw(enc, N, xd, _abi.LANG_ENCODER_IN_ROWS, 0, codec.flat.data_ptr(), None, c2[pad:].data_ptr(), code_layout)
    assert torch.equal(f2, f_all) and torch.equal(c2, c_all)


@pytest.mark.parametrize("layout", ["rows", "channels"])
def test_fused_codes_equal_the_codec(hip, layout):
    x, _, _ = _rows257()
    enc, codec = _encoder(), _codec(2)
    for feats in (x[:130].to(DEV), _planes(x[:130], pad=3)):
        f32, codes = enc.encode_codes(feats, codec, layout=layout)
        assert tuple(codes.shape) == ((130, 15) if layout == "rows" else (15, 130))
        assert torch.equal(f32, enc.encode(x[:130].to(DEV), out=torch.empty(130, 32, device=DEV)))
        assert torch.equal(codes, codec.encode(f32, layout))
    # a batch: one code map per item
    xb = R.make_features(70, SEED + 1).view(2, 5, 7, 768).permute(0, 3, 1, 2).contiguous().to(DEV)
    f32, codes = enc.encode_codes(xb, codec, layout=layout)
    assert tuple(codes.shape) == ((2, 35, 15) if layout == "rows" else (2, 15, 35))
    for b in range(2):
        assert torch.equal(codes[b], codec.encode(f32[35 * b:35 * (b + 1)], layout))


def test_add_keyframe_hr_is_encode_then_add_keyframe(hip):
    from online_lang_splatting_amd.slam_iterations import OnlineLanguageTargets
    h, w = 9, 13
    hr = R.make_features(h * w, SEED + 3).t().contiguous().view(1, 768, h, w).to(DEV)
    enc = _encoder()
    a, b = OnlineLanguageTargets(_codec(1), lr=1e-3, hw=(h, w)), OnlineLanguageTargets(_codec(1), lr=1e-3, hw=(h, w))
    ta = a.add_keyframe_hr("kf", hr, enc)
    tb = b.add_keyframe("kf", enc.encode(hr))
    assert tuple(ta.shape) == (15, h, w) and torch.equal(ta, tb)
    assert torch.equal(a.features["kf"], b.features["kf"]) and tuple(a.features["kf"].shape) == (h * w, 32)
    assert torch.equal(a.codec.flat, b.codec.flat) and torch.equal(a.last_loss, b.last_loss) and a.steps == b.steps == 1
    # the stored rows are the object's own: the encoder's reusable buffer may be overwritten
    kept = a.features["kf"].clone()
    enc.encode(R.make_features(h * w, SEED + 4).to(DEV))
    assert torch.equal(a.features["kf"], kept)
    a.rehearse(["kf"])
    b.rehearse(["kf"])
    assert torch.equal(a.codec.flat, b.codec.flat)
    with pytest.raises(RuntimeError, match="add_keyframe_hr"):
        a.add_keyframe_hr("bad", hr[:, :, :5].contiguous(), enc)


def test_nan_row_stays_in_its_row(hip):
    x, _, _ = _rows257()
    enc = _encoder()
    clean = enc.encode(x[:130].to(DEV)).clone()
    for bad_row, bad_col in ((5, 0), (64, 767), (129, 100)):
        xb = x[:130].clone()
        xb[bad_row, bad_col] = float("nan")
        for feats in (xb.to(DEV), _planes(xb)):
            out = enc.encode(feats)
            assert bool(torch.isnan(out[bad_row]).all())
            keep = torch.arange(130, device=DEV) != bad_row
            assert torch.equal(out[keep], clean[keep])


def test_errors_are_raised_not_copied(hip):
    x, _, _ = _rows257()
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
        enc.encode(xd, out=torch.empty(69, 32, device=DEV))
    with pytest.raises(RuntimeError, match="OnlineLanguageCodec"):
        enc.encode_codes(xd, None)


def test_round_trip_through_the_query(hip):
    """768 -> 32 -> 15 on the device, then the query's 15 -> 32 -> 768 and the products with some of the input rows as phrases,
    against the same chain restated in float64 and float32."""
    from online_lang_splatting_amd.lang_query import LanguageDecoder, LanguageQuery
    N = 70
    x = R.make_features(N, SEED + 5)
    online, dec_state = RC.initial_params(4), RQ.decoder_state(104)
    pos, neg = x[:3].contiguous(), x[3:7].contiguous()
    enc, codec = _encoder(), _codec(4)
    q = LanguageQuery(LanguageDecoder(DEV, dec_state), codec)
    q.set_phrases(pos.to(DEV), neg.to(DEV))
    f32, codes = enc.encode_codes(x.to(DEV), codec, layout="channels")
    sims = q.similarities(codes.view(15, 1, N)).cpu()
    ref = []
    for dt in (torch.float64, torch.float32):
        with torch.no_grad():
            c = RC.codec_from(online, dt).encode(R.encode(_state(), x, dt))
        ref.append((c, RQ.similarities(c.t().reshape(15, 1, N), online, dec_state, torch.cat([pos, neg]), dt)))
    assert tuple(sims.shape) == tuple(ref[0][1].shape) == (7, 1, N)
    _ratio_rule("round trip: features32", f32.cpu(), R.encode(_state(), x, torch.float64), R.encode(_state(), x, torch.float32))
    _ratio_rule("round trip: codes", codes.cpu().t(), ref[0][0], ref[1][0])
    _ratio_rule("round trip: similarities", sims, ref[0][1], ref[1][1])


def test_validator_sentences(hip):
    """The shared input and output checks' sentences, word for word, on the smallest inputs that reach them."""
    from online_lang_splatting_amd.lang_encoder import LanguageEncoder
    enc, m = _encoder(), torch.rand(1, 768, 2, 2, device=DEV)
    with _raises_exactly("LanguageEncoder: a GPU device is required (there is no torch fallback)"):
        LanguageEncoder("cpu")
    with _raises_exactly("encode: features must be a float32 tensor on the GPU"):
        enc.encode(m.double())
    with _raises_exactly("encode_codes: features must be a float32 tensor on the GPU"):
        enc.encode_codes(m.cpu(), _codec())
    with _raises_exactly("encode: features has shape (1, 767, 2, 2), expected [N,768], [768,h,w] or [B,768,h,w]"):
        enc.encode(m[:, :767].contiguous())
    with _raises_exactly("encode: every channel plane must be contiguous and the planes must not overlap "
                         "(strides (3072, 4, 1, 2) for shape (1, 768, 2, 2))"):
        enc.encode(m.transpose(2, 3))
    with _raises_exactly("encode: features has shape (2, 31), expected [N,768] with N >= 1"):
        enc.encode(torch.rand(2, 31, device=DEV))
    with _raises_exactly("encode: [N,768] rows must be contiguous"):
        enc.encode(torch.rand(768, 2, device=DEV).t())
    with _raises_exactly("encode: out must be a contiguous float32 [4,32] tensor on cuda:0"):
        enc.encode(m, out=torch.empty(3, 32, device=DEV))
