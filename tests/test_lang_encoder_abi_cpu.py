"""The language encoder's C-ABI and host helpers without a GPU: the symbol loads, _abi carries the sizes and the state list,
every argument error returns OLSR_ERR_ARG before anything touches the device, and the checkpoint loader accepts what it
should and names what it rejects."""
import ctypes as C

import pytest
import torch

import lang_encoder_ref as R
from online_lang_splatting_amd import _abi


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


def _params(**kw):
    p = dict(n_widths=6, in_layout=_abi.LANG_ENCODER_IN_CHANNELS, code_layout=_abi.LANG_AE_CODES_CHANNELS, plane_stride=36864,
             bn_eps=1e-5)
    widths = kw.pop("widths", _abi.LANG_ENCODER_WIDTHS)
    p.update(kw)
    s = _abi.OlsrLangEncoderParams(**p)
    for k, v in enumerate(widths):
        s.widths[k] = v
    return s


def test_symbol_and_abi(L):
    assert hasattr(L, "olsr_lang_encoder_encode")
    from online_lang_splatting_amd import _lib
    assert "olsr_lang_encoder_encode" in _lib.EXPORTS
    assert _abi.LANG_ENCODER_PARAMS == 572128 == R.N_ENCODER
    assert (_abi.LANG_ENCODER_IN_ROWS, _abi.LANG_ENCODER_IN_CHANNELS) == (0, 1)
    assert tuple(_abi.LANG_ENCODER_WIDTHS) == tuple(R.WIDTHS)
    assert tuple(_abi.LANG_ENCODER_STATE) == tuple(R.STATE)
    assert sum(int(torch.Size(s).numel()) for _, s in _abi.LANG_ENCODER_STATE) == _abi.LANG_ENCODER_PARAMS
    # int32 n_widths, widths[8], in_layout, code_layout | 4 bytes of padding | int64 plane_stride | double bn_eps
    assert C.sizeof(_abi.OlsrLangEncoderParams) == 64
    assert _abi.OlsrLangEncoderParams.plane_stride.offset == 48 and _abi.OlsrLangEncoderParams.bn_eps.offset == 56
    import online_lang_splatting_amd as pkg
    assert pkg.LanguageEncoder is not None and "LanguageEncoder" in pkg.__all__


# Addresses that are never dereferenced: every row below must be rejected before a launch.
PTR = 0x1000
N = 36864

BAD_PARAMS = [("n_widths", dict(n_widths=5)), ("n_widths", dict(n_widths=7)),
              ("the single-stage chain", dict(n_widths=7, widths=(768, 384, 192, 96, 48, 24, 15))),
              ("a width", dict(widths=(768, 384, 256, 128, 64, 32))), ("a width", dict(widths=(768, 512, 256, 128, 64, 15))),
              ("the decoder's list", dict(widths=_abi.LANG_QUERY_WIDTHS)),
              ("plane_stride < N", dict(plane_stride=N - 1)), ("plane_stride < 0", dict(plane_stride=-N)),
              ("in_layout", dict(in_layout=2)), ("in_layout", dict(in_layout=-1)), ("code_layout", dict(code_layout=2)),
              ("bn_eps = 0", dict(bn_eps=0.0)), ("bn_eps < 0", dict(bn_eps=-1e-5)), ("bn_eps NaN", dict(bn_eps=float("nan")))]


def test_argument_errors(L):
    # params, N, features768, encoder_params, online_params, features32, codes, stream
    ok = [_params(), N, PTR, PTR, PTR, PTR, PTR, None]
    rows = [("params struct", {0: None}), ("N = 0", {1: 0}), ("N < 0", {1: -5}), ("features768", {2: None}),
            ("encoder_params", {3: None}), ("both outputs NULL", {5: None, 6: None}), ("both outputs NULL", {4: None, 5: None, 6: None}),
            ("codes without online_params", {4: None}), ("encoder_params alignment", {3: PTR + 4}),
            ("encoder_params alignment", {3: PTR + 8})]
    rows += [(what, {0: _params(**kw)}) for what, kw in BAD_PARAMS]
    for what, change in rows:
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        a0 = None if args[0] is None else C.byref(args[0])
        assert L.olsr_lang_encoder_encode(a0, *args[1:]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error()
    # the width list is reported with the words of the query's entry
    assert L.olsr_lang_encoder_encode(C.byref(_params(n_widths=5)), *ok[1:]) == _abi.OLSR_ERR_ARG
    assert b"layer widths {768, 512, 256, 128, 64, 32} only" in L.olsr_last_error()
    # the row layout does not read plane_stride
    assert L.olsr_lang_encoder_encode(C.byref(_params(in_layout=_abi.LANG_ENCODER_IN_ROWS, plane_stride=0, n_widths=5)),
                                      *ok[1:]) == _abi.OLSR_ERR_ARG


def test_checkpoint_loader():
    from online_lang_splatting_amd import lang_encoder
    state = R.encoder_state(3)
    flat = torch.zeros(R.N_ENCODER)
    lang_encoder.load_encoder_state(flat, state)
    assert torch.equal(flat, R.flatten(state))
    views = lang_encoder.encoder_views(flat)
    assert list(views) == [k for k, _ in R.STATE] and [tuple(v.shape) for v in views.values()] == [tuple(s) for _, s in R.STATE]
    # a plain AutoencoderMLP state dict: decoder entries and num_batches_tracked are ignored
    full = R.encoder_from(state, torch.float32).state_dict()
    assert any(k.startswith("decoder.") for k in full) and any(k.endswith("num_batches_tracked") for k in full)
    back = torch.zeros(R.N_ENCODER)
    lang_encoder.load_encoder_state(back, full)
    assert torch.equal(back, flat)
    # a Lightning checkpoint: {"state_dict": {"model.encoder.0.weight": ...}}
    back.zero_()
    lang_encoder.load_encoder_state(back, {"epoch": 3, "state_dict": {"model." + k: v for k, v in full.items()}})
    assert torch.equal(back, flat)
    with pytest.raises(RuntimeError, match=r"missing keys \['encoder.4.running_var'\]"):
        lang_encoder.load_encoder_state(back, {k: v for k, v in state.items() if k != "encoder.4.running_var"})
    with pytest.raises(RuntimeError, match=r"unexpected keys \['encoder.13.weight'\]"):
        lang_encoder.load_encoder_state(back, dict(state, **{"encoder.13.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match=r"encoder.0.weight has shape \(384, 768\).*compiled into"):
        lang_encoder.load_encoder_state(back, dict(state, **{"encoder.0.weight": torch.zeros(384, 768)}))
    with pytest.raises(RuntimeError, match="missing keys"):
        lang_encoder.load_encoder_state(back, {"state_dict": {"model.decoder.0.weight": torch.zeros(192, 32)}})
    with pytest.raises(RuntimeError, match="checkpoint or state dict"):
        lang_encoder.load_encoder_state(back, [1, 2])
    with pytest.raises(RuntimeError, match="572128"):
        lang_encoder.encoder_views(torch.zeros(572127))


def test_encoder_needs_a_gpu():
    from online_lang_splatting_amd import lang_encoder
    with pytest.raises(RuntimeError, match="GPU"):
        lang_encoder.LanguageEncoder("cpu")
