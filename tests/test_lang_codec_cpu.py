"""The online language autoencoder's C-ABI and host helpers without a GPU: the symbols load, every argument error returns
OLSR_ERR_ARG before anything touches the device, the scratch size grows with N, and the state_dict layout is the reference
module's (names and shapes recorded in tests/golden/lang_codec.npz)."""
import ctypes as C

import pytest
import torch

import lang_codec_ref as R
from online_lang_splatting_amd import _abi


@pytest.fixture(scope="module")
def L():
    from online_lang_splatting_amd import _lib, build
    build.build()
    return _lib.lib()


def _params(**kw):
    p = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1, code_layout=_abi.LANG_AE_CODES_ROWS, in_dim=32, hidden_dim=24,
             code_dim=15)
    p.update(kw)
    return _abi.OlsrLangAeParams(**p)


def test_symbols_load(L):
    for name in ("olsr_lang_ae_scratch_bytes", "olsr_lang_ae_train_step", "olsr_lang_ae_encode", "olsr_lang_ae_decode"):
        assert hasattr(L, name), name
    assert C.sizeof(_abi.OlsrLangAeParams) == 4 * 8 + 6 * 4
    assert (_abi.LANG_AE_IN, _abi.LANG_AE_HIDDEN, _abi.LANG_AE_CODE, _abi.LANG_AE_PARAMS) == (32, 24, 15, 2351)


def test_scratch_bytes_is_monotone(L):
    sizes = [L.olsr_lang_ae_scratch_bytes(n) for n in (1, 255, 256, 257, 1000, 36864, 36865, 1 << 20)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert sizes[0] >= 2351 * 4 and L.olsr_lang_ae_scratch_bytes(0) > 0 and L.olsr_lang_ae_scratch_bytes(-5) > 0
    assert sizes[5] >= (36864 // 256) * 2351 * 4                                # one partial gradient per 256 rows


# Addresses that are never dereferenced: every row below must be rejected before a launch.
PTR = 0x1000


def test_train_step_argument_errors(L):
    ok = [_params(), 100] + [PTR] * 10     # params, N, features, params, exp_avg, exp_avg_sq, step_dev, loss, codes, grad_out, scratch, stream
    rows = [("params struct", 0, None), ("N = 0", 1, 0), ("N < 0", 1, -7), ("features", 2, None), ("params", 3, None),
            ("exp_avg", 4, None), ("exp_avg_sq", 5, None), ("loss", 7, None), ("scratch", 10, None),
            ("layout", 0, _params(code_layout=2)), ("layout", 0, _params(code_layout=-1)), ("in_dim", 0, _params(in_dim=64)),
            ("hidden_dim", 0, _params(hidden_dim=12)), ("code_dim", 0, _params(code_dim=16)),
            ("device step without a counter", None, None)]
    for what, k, bad in rows:
        args = list(ok)
        if k is None:
            args[0], args[6] = _params(step=0), None
        else:
            args[k] = bad
        a0 = None if args[0] is None else C.byref(args[0])
        assert L.olsr_lang_ae_train_step(a0, *args[1:]) == _abi.OLSR_ERR_ARG, what
        assert L.olsr_last_error()


def test_encode_decode_argument_errors(L):
    for fn in (L.olsr_lang_ae_encode, L.olsr_lang_ae_decode):
        ok = [100, PTR, PTR, _abi.LANG_AE_CODES_CHANNELS, PTR, None]
        for what, k, bad in (("N = 0", 0, 0), ("N < 0", 0, -1), ("input", 1, None), ("params", 2, None), ("layout", 3, 2),
                             ("layout", 3, -1), ("output", 4, None)):
            args = list(ok)
            args[k] = bad
            assert fn(*args) == _abi.OLSR_ERR_ARG, (fn.__name__, what)


def test_state_dict_layout_round_trips():
    from online_lang_splatting_amd import lang_codec
    z = R.golden()
    names = [str(k) for k in z["state_names"]]
    shapes = [tuple(int(d) for d in s if d) for s in z["state_shapes"]]
    assert [k for k, _ in _abi.LANG_AE_STATE] == names and [tuple(s) for _, s in _abi.LANG_AE_STATE] == shapes
    flat = torch.from_numpy(z["n257_s0_params"]).clone()
    views = lang_codec.state_views(flat)
    assert list(views) == names and [tuple(v.shape) for v in views.values()] == shapes
    # the flat order is the reference module's: a torch module of that structure loads the views and gives them back
    m = R.Codec()
    m.load_state_dict(views)
    assert list(m.state_dict()) == names
    back = torch.zeros(2351)
    lang_codec.load_state(back, m.state_dict())
    assert torch.equal(back, flat) and torch.equal(R.flatten(m.state_dict()), flat)
    with pytest.raises(RuntimeError, match="missing keys"):
        lang_codec.load_state(back, {k: v for k, v in views.items() if k != "decoder.2.bias"})
    with pytest.raises(RuntimeError, match="unexpected keys"):
        lang_codec.load_state(back, dict(views, extra=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="compiled into"):
        lang_codec.load_state(back, dict(views, **{"encoder.2.weight": torch.zeros(6, 24)}))
    with pytest.raises(RuntimeError, match="2351"):
        lang_codec.state_views(torch.zeros(2350))


def test_codec_needs_a_gpu():
    from online_lang_splatting_amd import lang_codec
    with pytest.raises(RuntimeError, match="GPU"):
        lang_codec.OnlineLanguageCodec("cpu")
