"""The single-stage chain's C-ABI (include/olsr_single_stage.h) and host helpers without a GPU: both symbols load from
libolsr.so, _abi carries the sizes and the state lists, every argument error returns OLSR_ERR_ARG before anything touches the
device, the checkpoint loaders accept what they should and name what they reject, and every declared function has an
extents row in tests/test_gpu_single_stage_extents.py."""
import ctypes as C
import os
import re

import pytest
import torch

import lang_single_stage_ref as R
from online_lang_splatting_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


def _declared():
    src = open(os.path.join(ROOT, "include", "olsr_single_stage.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(olsr_[a-z0-9_]+)\s*\(", src)))


def test_symbols_and_abi(L):
    from online_lang_splatting_amd import _lib
    assert _declared() == sorted(_lib.EXPORTS_SINGLE_STAGE) == ["olsr_ss_encoder_encode", "olsr_ss_query_sims"]
    assert not set(_lib.EXPORTS_SINGLE_STAGE) & set(_lib.EXPORTS)
    for name in _lib.EXPORTS_SINGLE_STAGE:
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "olsr_single_stage.h")).read()
    assert int(re.search(r"#define OLSR_SS_ENCODER_PARAMS (\d+)", header).group(1)) == _abi.SS_ENCODER_PARAMS == 396927 == R.N_ENCODER
    assert int(re.search(r"#define OLSR_SS_DECODER_PARAMS (\d+)", header).group(1)) == _abi.SS_DECODER_PARAMS == 542544 == R.N_DECODER
    assert tuple(_abi.SS_ENCODER_WIDTHS) == tuple(R.ENCODER_WIDTHS) == (768, 384, 192, 96, 48, 24, 15)
    assert tuple(_abi.SS_DECODER_WIDTHS) == tuple(R.DECODER_WIDTHS) == (15, 24, 48, 96, 192, 384, 384, 768)
    assert tuple(_abi.SS_ENCODER_STATE) == tuple(R.ENCODER_STATE) and tuple(_abi.SS_DECODER_STATE) == tuple(R.DECODER_STATE)
    assert sum(int(torch.Size(s).numel()) for _, s in _abi.SS_ENCODER_STATE) == _abi.SS_ENCODER_PARAMS
    assert sum(int(torch.Size(s).numel()) for _, s in _abi.SS_DECODER_STATE) == _abi.SS_DECODER_PARAMS
    # every weight matrix and bias of the encoder starts on a 16-byte boundary of an aligned array
    off = 0
    for name, shape in _abi.SS_ENCODER_STATE:
        if int(name.split(".")[1]) % 3 == 0:
            assert off % 4 == 0, name
        off += int(torch.Size(shape).numel())
    # int32 n_widths, widths[8], in_layout, code_layout | 4 bytes of padding | int64 plane_stride | double bn_eps
    assert C.sizeof(_abi.OlsrSsEncoderParams) == 64
    assert _abi.OlsrSsEncoderParams.in_layout.offset == 36 and _abi.OlsrSsEncoderParams.code_layout.offset == 40
    assert _abi.OlsrSsEncoderParams.plane_stride.offset == 48 and _abi.OlsrSsEncoderParams.bn_eps.offset == 56
    import online_lang_splatting_amd as pkg
    for name in ("SingleStageEncoder", "SingleStageDecoder", "SingleStageQuery", "SingleStageTargets"):
        assert getattr(pkg, name) is not None and name in pkg.__all__


def test_every_declared_function_has_an_extents_row():
    import test_gpu_single_stage_extents as T
    assert sorted(T.COVERED) == _declared()


# Addresses that are never dereferenced: every row below must be rejected before a launch.
PTR = 0x1000
N = 36864


def _enc_params(**kw):
    p = dict(n_widths=7, in_layout=_abi.LANG_ENCODER_IN_CHANNELS, code_layout=_abi.LANG_AE_CODES_CHANNELS, plane_stride=N,
             bn_eps=1e-5)
    widths = kw.pop("widths", _abi.SS_ENCODER_WIDTHS)
    p.update(kw)
    s = _abi.OlsrSsEncoderParams(**p)
    for k, v in enumerate(widths):
        s.widths[k] = v
    return s


BAD_ENCODER = [("n_widths", dict(n_widths=6)), ("n_widths", dict(n_widths=8)),
               ("the two-stage chain", dict(n_widths=6, widths=_abi.LANG_ENCODER_WIDTHS)),
               ("a width", dict(widths=(768, 384, 192, 96, 48, 24, 16))), ("a width", dict(widths=(768, 512, 192, 96, 48, 24, 15))),
               ("the decoder's list", dict(n_widths=8, widths=_abi.SS_DECODER_WIDTHS)),
               ("plane_stride < N", dict(plane_stride=N - 1)), ("plane_stride < 0", dict(plane_stride=-N)),
               ("in_layout", dict(in_layout=2)), ("in_layout", dict(in_layout=-1)), ("code_layout", dict(code_layout=2)),
               ("code_layout", dict(code_layout=-1)),
               ("bn_eps = 0", dict(bn_eps=0.0)), ("bn_eps < 0", dict(bn_eps=-1e-5)), ("bn_eps NaN", dict(bn_eps=float("nan")))]


def test_encoder_argument_errors(L):
    # params, N, features768, encoder_params, codes, stream
    ok = [_enc_params(), N, PTR, PTR, PTR, None]
    rows = [("params struct", {0: None}), ("N = 0", {1: 0}), ("N < 0", {1: -5}), ("features768", {2: None}),
            ("encoder_params", {3: None}), ("codes", {4: None}), ("encoder_params alignment", {3: PTR + 4}),
            ("encoder_params alignment", {3: PTR + 8})]
    rows += [(what, {0: _enc_params(**kw)}) for what, kw in BAD_ENCODER]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        a0 = None if args[0] is None else C.byref(args[0])
        assert L.olsr_ss_encoder_encode(a0, *args[1:]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error()
    assert L.olsr_ss_encoder_encode(C.byref(_enc_params(n_widths=6)), *ok[1:]) == _abi.OLSR_ERR_ARG
    assert b"layer widths {768, 384, 192, 96, 48, 24, 15} only" in L.olsr_last_error()
    # the row layout does not read plane_stride: the width list is what is wrong here
    assert L.olsr_ss_encoder_encode(C.byref(_enc_params(in_layout=_abi.LANG_ENCODER_IN_ROWS, plane_stride=0, n_widths=6)),
                                    *ok[1:]) == _abi.OLSR_ERR_ARG
    assert b"layer widths" in L.olsr_last_error()


def _query_params(**kw):
    p = dict(n_widths=8, K=7, n_pos=3, n_labels=0, in_width=40, in_height=24, dec_width=40, dec_height=24, out_width=40,
             out_height=24, thresh=0.5, flags=0)
    widths = kw.pop("widths", _abi.SS_DECODER_WIDTHS)
    p.update(kw)
    s = _abi.OlsrLangQueryParams(**p)
    for k, v in enumerate(widths):
        s.widths[k] = v
    return s


BAD_QUERY = [("n_widths", dict(n_widths=7)), ("n_widths", dict(n_widths=6)),
             ("the two-stage chain", dict(n_widths=6, widths=_abi.LANG_QUERY_WIDTHS)),
             ("a width", dict(widths=(15, 24, 48, 96, 192, 384, 512, 768))), ("a width", dict(widths=(32, 24, 48, 96, 192, 384, 384, 768))),
             ("the encoder's list", dict(n_widths=7, widths=_abi.SS_ENCODER_WIDTHS)),
             ("K = 0", dict(K=0, n_pos=0)), ("K = 65", dict(K=65)), ("K < 0", dict(K=-1, n_pos=0)),
             ("n_pos + n_labels > K", dict(n_pos=5, n_labels=3)), ("n_pos < 0", dict(n_pos=-1)),
             ("a zero extent", dict(in_width=0)), ("a zero extent", dict(dec_height=0)), ("a negative extent", dict(out_width=-3)),
             ("too many pixels", dict(dec_width=1 << 15, dec_height=1 << 14)), ("unknown flags", dict(flags=4))]


def test_query_argument_errors(L):
    # params, codes, decoder_params, phrases, sims, stream
    ok = [_query_params(), PTR, PTR, PTR, PTR, None]
    rows = [("params struct", {0: None}), ("codes", {1: None}), ("decoder_params", {2: None}), ("phrases", {3: None}),
            ("sims", {4: None}), ("decoder_params alignment", {2: PTR + 4}), ("phrases alignment", {3: PTR + 8})]
    rows += [(what, {0: _query_params(**kw)}) for what, kw in BAD_QUERY]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        a0 = None if args[0] is None else C.byref(args[0])
        assert L.olsr_ss_query_sims(a0, *args[1:]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error()
    assert L.olsr_ss_query_sims(C.byref(_query_params(n_widths=6, widths=_abi.LANG_QUERY_WIDTHS)), *ok[1:]) == _abi.OLSR_ERR_ARG
    assert b"layer widths {15, 24, 48, 96, 192, 384, 384, 768} only" in L.olsr_last_error()
    # and the two-stage entries keep rejecting the single-stage lists
    assert L.olsr_lang_query_sims(C.byref(_query_params()), PTR, PTR, PTR, PTR, PTR, None) == _abi.OLSR_ERR_ARG
    assert b"layer widths {32, 192, 256, 384, 512, 768} only" in L.olsr_last_error()


def test_checkpoint_loaders():
    from online_lang_splatting_amd import lang_single_stage as S
    enc, dec = R.module_state(3)
    full = R.module_from(dict(enc, **dec), torch.float32).state_dict()
    assert any(k.endswith("num_batches_tracked") for k in full)
    lightning = {"epoch": 3, "state_dict": {"model." + k: v for k, v in full.items()}}
    for load, views, state, flatten, n in ((S.load_encoder_state, S.encoder_views, enc, R.flatten_encoder, R.N_ENCODER),
                                           (S.load_decoder_state, S.decoder_views, dec, R.flatten_decoder, R.N_DECODER)):
        flat = torch.zeros(n)
        load(flat, state)
        assert torch.equal(flat, flatten(state))
        v = views(flat)
        assert list(v) == list(state) and [tuple(t.shape) for t in v.values()] == [tuple(t.shape) for t in state.values()]
        # a plain AutoencoderMLP state dict (the other half and num_batches_tracked are ignored), and a Lightning checkpoint
        for other in (full, lightning):
            back = torch.zeros(n)
            load(back, other)
            assert torch.equal(back, flat)
        with pytest.raises(RuntimeError, match="checkpoint or state dict"):
            load(flat, [1, 2])
        with pytest.raises(RuntimeError, match=str(n)):
            views(torch.zeros(n - 1))
    back = torch.zeros(R.N_ENCODER)
    with pytest.raises(RuntimeError, match=r"missing keys \['encoder.13.running_var'\]"):
        S.load_encoder_state(back, {k: v for k, v in enc.items() if k != "encoder.13.running_var"})
    with pytest.raises(RuntimeError, match=r"unexpected keys \['encoder.16.weight'\]"):
        S.load_encoder_state(back, dict(enc, **{"encoder.16.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match=r"encoder.0.weight has shape \(512, 768\).*compiled into"):
        S.load_encoder_state(back, dict(enc, **{"encoder.0.weight": torch.zeros(512, 768)}))
    with pytest.raises(RuntimeError, match="missing keys"):
        S.load_encoder_state(back, {"state_dict": {"model.decoder.0.weight": torch.zeros(24, 15)}})
    back = torch.zeros(R.N_DECODER)
    with pytest.raises(RuntimeError, match=r"missing keys \['decoder.12.bias'\]"):
        S.load_decoder_state(back, {k: v for k, v in dec.items() if k != "decoder.12.bias"})
    with pytest.raises(RuntimeError, match=r"unexpected keys \['decoder.14.weight'\]"):
        S.load_decoder_state(back, dict(dec, **{"decoder.14.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match=r"decoder.0.weight has shape \(192, 32\).*compiled into"):
        S.load_decoder_state(back, dict(dec, **{"decoder.0.weight": torch.zeros(192, 32)}))


def test_a_gpu_is_required_and_the_types_are_checked():
    from online_lang_splatting_amd import lang_single_stage as S
    with pytest.raises(RuntimeError, match="GPU"):
        S.SingleStageEncoder("cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        S.SingleStageDecoder("cpu")
    with pytest.raises(RuntimeError, match="SingleStageDecoder is expected"):
        S.SingleStageQuery(None)
    with pytest.raises(RuntimeError, match="SingleStageEncoder is expected"):
        S.SingleStageTargets(None)
    from online_lang_splatting_amd.lang_query import LanguageQuery
    assert issubclass(S.SingleStageQuery, LanguageQuery)
