"""No entry of include/olsr_single_stage.h writes outside the bytes it asked for: the extents rows of the two entries, the
way tests/test_gpu_extents.py holds them for include/olsr.h, on tests/extent_harness.py as it is.

| entry                  | shapes                                  | why these                                         | scratch |
| olsr_ss_encoder_encode | N 1, 63, 64, 65; both code layouts      | 64 rows per block                                 | none    |
| olsr_ss_query_sims     | 24x40, 33x31                            | 64 pixels per tile (960 = 15 tiles, 1023 = 16 - 1)| none    |

Each entry runs three ways: plain buffers, guarded outputs (64 KiB of a known byte on either side, the output pre-filled with
a pattern no kernel writes), and guarded outputs that start 4 bytes past a 256-byte boundary (neither entry assumes anything
about its output's alignment).  Checked: the guards are intact, every word of the output was written, and the guarded runs
give the plain run's bits.  The values themselves are held to the float64 restatement by the rule of
tests/test_gpu_lang_single_stage.py."""
import ctypes as C

import pytest
import torch

import extent_harness as H
import lang_query_ref as RQ
import lang_single_stage_ref as R
from online_lang_splatting_amd import _abi
from test_gpu_lang_codec import _ratio_rule

pytestmark = pytest.mark.gpu
DEV = H.DEV
F32 = torch.float32
VP = C.c_void_p
SEED = 21

COVERED = ("olsr_ss_encoder_encode", "olsr_ss_query_sims")


def _L():
    from online_lang_splatting_amd._lib import lib
    return lib()


def _check_rc(rc):
    from online_lang_splatting_amd._lib import check
    check(rc)


def _stream():
    return VP(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


@pytest.fixture(autouse=True)
def _forget_buffers():
    yield
    H.reset()


def three_ways(entry, shape):
    """entry(out) runs the entry into the float32 tensor `out` of `shape`.  -> the plain run's output, after the guarded and the
    misaligned guarded runs passed H.check and gave the same bits."""
    plain = torch.empty(shape, dtype=F32, device=DEV)
    entry(plain)
    torch.cuda.synchronize()
    for misalign in (0, 4):
        H.reset()
        out = H.guarded_tensor(shape, F32, misalign)
        assert out.data_ptr() % 256 == misalign
        entry(out)
        H.check([out], (), [out])
        assert H.same_bits(out, plain), f"the guarded run (base + {misalign}) differs from the plain run"
    H.reset()
    return plain


_REFS = {}


def _encoder_case():
    if "enc" not in _REFS:
        state, x = R.encoder_state(SEED), R.make_features(65, SEED)
        _REFS["enc"] = (state, x, R.encode(state, x, torch.float64), R.encode(state, x, torch.float32))
    return _REFS["enc"]


@pytest.mark.parametrize("code_layout", [0, 1])
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_ss_encoder_encode(hip, N, code_layout):
    from online_lang_splatting_amd.lang_single_stage import SingleStageEncoder
    L = _L()
    state, x, t64, t32 = _encoder_case()
    enc = SingleStageEncoder(DEV, state)
    p = _abi.OlsrSsEncoderParams(n_widths=len(_abi.SS_ENCODER_WIDTHS), in_layout=_abi.LANG_ENCODER_IN_ROWS, code_layout=code_layout,
                                 plane_stride=0, bn_eps=enc.eps)
    for k, v in enumerate(_abi.SS_ENCODER_WIDTHS):
        p.widths[k] = v
    xd = x[:N].to(DEV).contiguous()

    def entry(out):
        _check_rc(L.olsr_ss_encoder_encode(C.byref(p), N, xd.data_ptr(), enc.flat.data_ptr(), out.data_ptr(), _stream()))
    out = three_ways(entry, (N, 15) if code_layout == _abi.LANG_AE_CODES_ROWS else (15, N)).cpu()
    _ratio_rule(f"N = {N}, code layout {code_layout}", out if code_layout == _abi.LANG_AE_CODES_ROWS else out.t(), t64[:N], t32[:N])


@pytest.mark.parametrize("h,w,K", [(24, 40, 7), (33, 31, 17)])
def test_ss_query_sims(hip, h, w, K):
    from online_lang_splatting_amd.lang_single_stage import SingleStageDecoder
    L = _L()
    dec_state = R.decoder_state(SEED + K)
    codes, _ = RQ.make_codes(h, w, SEED + K)
    phrases = RQ.unit_rows(K, SEED + K)
    dec = SingleStageDecoder(DEV, dec_state)
    p = _abi.OlsrLangQueryParams(n_widths=len(_abi.SS_DECODER_WIDTHS), K=K, n_pos=1, n_labels=0, in_width=w, in_height=h,
                                 dec_width=w, dec_height=h, out_width=w, out_height=h, thresh=0.5, flags=0)
    for k, v in enumerate(_abi.SS_DECODER_WIDTHS):
        p.widths[k] = v
    cd, pd = codes.to(DEV).contiguous(), phrases.to(DEV).contiguous()

    def entry(out):
        _check_rc(L.olsr_ss_query_sims(C.byref(p), cd.data_ptr(), dec.flat.data_ptr(), pd.data_ptr(), out.data_ptr(), _stream()))
    out = three_ways(entry, (K, h, w)).cpu()
    t64, t32 = (R.similarities(codes, dec_state, phrases, dt) for dt in (torch.float64, torch.float32))
    _ratio_rule(f"{w} x {h}, K = {K}", out, t64, t32)
