"""The language query's C-ABI and host helpers without a GPU: the symbols load, every argument error returns OLSR_ERR_ARG
before anything touches the device, the scratch size is monotone and far below a 768-wide image, and the checkpoint loader
accepts what it should and names what it rejects."""
import ctypes as C

import pytest
import torch

import lang_query_ref as R
from online_lang_splatting_amd import _abi


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


def _params(**kw):
    p = dict(n_widths=6, K=7, n_pos=3, n_labels=0, in_width=160, in_height=120, dec_width=160, dec_height=120, out_width=160,
             out_height=120, thresh=0.4, flags=_abi.LANG_QUERY_WANT_MASK)
    widths = kw.pop("widths", _abi.LANG_QUERY_WIDTHS)
    p.update(kw)
    s = _abi.OlsrLangQueryParams(**p)
    for k, v in enumerate(widths):
        s.widths[k] = v
    return s


def test_symbols_load(L):
    for name in ("olsr_lang_query_scratch_bytes", "olsr_lang_query_sims", "olsr_lang_query_relevancy"):
        assert hasattr(L, name), name
    assert C.sizeof(_abi.OlsrLangQueryParams) == 4 * (1 + 8 + 9 + 2)
    assert sum(int(torch.Size(s).numel()) for _, s in _abi.LANG_QUERY_STATE) == _abi.LANG_QUERY_DECODER_PARAMS == R.N_DECODER
    assert tuple(_abi.LANG_QUERY_STATE) == tuple(R.STATE)
    import online_lang_splatting_amd as pkg
    assert pkg.LanguageQuery is not None and pkg.LanguageDecoder is not None


def test_scratch_bytes_is_monotone_and_small(L):
    sizes = [L.olsr_lang_query_scratch_bytes(C.byref(_params(out_width=w, out_height=h)))
             for w, h in ((1, 1), (32, 32), (33, 32), (157, 101), (640, 480), (1200, 680), (2400, 1360))]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    more = [L.olsr_lang_query_scratch_bytes(C.byref(_params(out_width=1200, out_height=680, n_pos=p, K=p + 4))) for p in (1, 3, 8)]
    assert more[0] < more[1] < more[2]
    N = 1200 * 680
    assert 0 < sizes[5] < 64 * N and sizes[5] < 768 * 4 * N // 1000          # no 768-wide image, by three orders of magnitude
    # the decode size and K do not enter: nothing of stage A goes through scratch
    assert L.olsr_lang_query_scratch_bytes(C.byref(_params(out_width=1200, out_height=680, dec_width=9, dec_height=9))) == sizes[5]
    assert L.olsr_lang_query_scratch_bytes(None) > 0
    assert L.olsr_lang_query_scratch_bytes(C.byref(_params(out_width=0))) > 0


# Addresses that are never dereferenced: every row below must be rejected before a launch.
PTR = 0x1000

BAD_PARAMS = [("n_widths", dict(n_widths=5)), ("n_widths", dict(n_widths=8)),
              ("the single-stage chain", dict(n_widths=8, widths=(15, 24, 48, 96, 192, 384, 384, 768))),
              ("a width", dict(widths=(32, 192, 256, 384, 512, 512))), ("a width", dict(widths=(16, 192, 256, 384, 512, 768))),
              ("K = 0", dict(K=0, n_pos=0)), ("K < 0", dict(K=-1, n_pos=0)), ("K > 64", dict(K=65)), ("n_pos < 0", dict(n_pos=-1)),
              ("n_labels < 0", dict(n_labels=-1)), ("n_pos + n_labels > K", dict(n_pos=5, n_labels=3)),
              ("in_width", dict(in_width=0)), ("in_height", dict(in_height=-3)), ("dec_width", dict(dec_width=0)),
              ("dec_height", dict(dec_height=0)), ("out_width", dict(out_width=0)), ("out_height", dict(out_height=-1)),
              ("too many pixels", dict(dec_width=1 << 15, dec_height=1 << 14)), ("flags", dict(flags=4))]


def test_sims_argument_errors(L):
    ok = [_params()] + [PTR] * 5 + [None]      # params, codes, online, decoder, phrases, sims, stream
    rows = [("params struct", 0, None), ("codes", 1, None), ("online_params", 2, None), ("decoder_params", 3, None),
            ("phrases", 4, None), ("sims", 5, None), ("decoder alignment", 3, PTR + 4), ("phrases alignment", 4, PTR + 8)]
    rows += [(what, 0, _params(**kw)) for what, kw in BAD_PARAMS]
    for what, k, bad in rows:
        args = list(ok)
        args[k] = bad
        a0 = None if args[0] is None else C.byref(args[0])
        assert L.olsr_lang_query_sims(a0, *args[1:]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error()


def test_relevancy_argument_errors(L):
    both = _abi.LANG_QUERY_WANT_MASK | _abi.LANG_QUERY_WANT_LABELS
    # params, sims, relevancy, smoothed, blended, score, coord, minmax, mask, labels, scratch, stream
    ok = [_params(n_labels=2, K=9, flags=both)] + [PTR] * 10 + [None]
    rows = [("params struct", 0, None), ("sims", 1, None), ("relevancy", 2, None), ("smoothed", 3, None), ("blended", 4, None),
            ("score", 5, None), ("coord", 6, None), ("minmax", 7, None), ("mask wanted", 8, None), ("labels wanted", 9, None),
            ("scratch", 10, None), ("no negative", 0, _params(K=3)), ("no negative", 0, _params(K=5, n_labels=2)),
            ("labels without label rows", 0, _params(flags=both)), ("thresh", 0, _params(thresh=float("nan"))),
            ("nothing to do", 0, _params(n_pos=0, flags=0)), ("mask without positives", 0, _params(n_pos=0, n_labels=2, flags=both))]
    rows += [(what, 0, _params(**kw)) for what, kw in BAD_PARAMS]
    for what, k, bad in rows:
        args = list(ok)
        args[k] = bad
        a0 = None if args[0] is None else C.byref(args[0])
        assert L.olsr_lang_query_relevancy(a0, *args[1:]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error()


def test_checkpoint_loader():
    from online_lang_splatting_amd import lang_query
    state = R.decoder_state(3)
    flat = torch.zeros(R.N_DECODER)
    lang_query.load_decoder_state(flat, state)
    assert torch.equal(flat, R.flatten(state))
    views = lang_query.decoder_views(flat)
    assert list(views) == [k for k, _ in R.STATE] and [tuple(v.shape) for v in views.values()] == [tuple(s) for _, s in R.STATE]
    # a plain AutoencoderMLP state dict: encoder and BatchNorm entries are ignored
    torch.manual_seed(3)
    full = R.GeneralAutoencoder().state_dict()
    assert any(k.startswith("encoder.") and "running_mean" in k for k in full)
    back = torch.zeros(R.N_DECODER)
    lang_query.load_decoder_state(back, full)
    assert torch.equal(back, flat)
    # a Lightning checkpoint: {"state_dict": {"model.decoder.0.weight": ...}}
    back.zero_()
    lang_query.load_decoder_state(back, {"epoch": 3, "state_dict": {"model." + k: v for k, v in full.items()}})
    assert torch.equal(back, flat)
    with pytest.raises(RuntimeError, match=r"missing keys \['decoder.4.bias'\]"):
        lang_query.load_decoder_state(back, {k: v for k, v in state.items() if k != "decoder.4.bias"})
    with pytest.raises(RuntimeError, match=r"unexpected keys \['decoder.10.weight'\]"):
        lang_query.load_decoder_state(back, dict(state, **{"decoder.10.weight": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="compiled into"):
        lang_query.load_decoder_state(back, dict(state, **{"decoder.8.weight": torch.zeros(512, 512)}))
    with pytest.raises(RuntimeError, match="missing keys"):
        lang_query.load_decoder_state(back, {"state_dict": {"model.encoder.0.weight": torch.zeros(512, 768)}})
    with pytest.raises(RuntimeError, match="checkpoint or state dict"):
        lang_query.load_decoder_state(back, [1, 2])
    with pytest.raises(RuntimeError, match="745536"):
        lang_query.decoder_views(torch.zeros(745535))


def test_query_needs_a_gpu():
    from online_lang_splatting_amd import lang_query
    with pytest.raises(RuntimeError, match="GPU"):
        lang_query.LanguageDecoder("cpu")
    with pytest.raises(RuntimeError, match="LanguageDecoder and an OnlineLanguageCodec"):
        lang_query.LanguageQuery(None, None)
