"""tests/lang_single_stage_ref.py against tests/golden/lang_single_stage.npz: arrays recorded from the reference's own
AutoencoderMLP([384,192,96,48,24,15], [24,48,96,192,384,384,768]) in eval(): encode in float64 and float32 on 70 rows and on
a 9 x 13 channel-major map, decode of 70 unit code rows against 7 phrase rows.  The restatement must reproduce every float64
array to 1e-12 and rebuild the inputs bit for bit.  Its float32 run is identical where the file was made; torch's CPU GEMM
may block another way with another thread count or build, so the bound on |restated float32 - recorded float32| is the
recorded float32 run's own largest error against float64, and the test prints what it found."""
import numpy as np
import pytest
import torch

import lang_single_stage_ref as R


@pytest.fixture(scope="module")
def Z():
    return R.golden()


def test_state_layout_is_the_modules(Z):
    sd = R.SingleStageAutoencoder().state_dict()
    assert [k for k in sd if k.startswith("encoder.") and not k.endswith("num_batches_tracked")] == [k for k, _ in R.ENCODER_STATE]
    assert [k for k in sd if k.startswith("decoder.")] == [k for k, _ in R.DECODER_STATE]
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in R.ENCODER_STATE + R.DECODER_STATE)
    assert sum(int(np.prod(s)) for _, s in R.ENCODER_STATE) == R.N_ENCODER == 393951 + 2976
    assert sum(int(np.prod(s)) for _, s in R.DECODER_STATE) == R.N_DECODER == 542544
    assert R.ENCODER_STATE[0] == ("encoder.0.weight", (384, 768)) and R.ENCODER_STATE[-1] == ("encoder.15.bias", (15,))
    assert R.DECODER_STATE[0] == ("decoder.0.weight", (24, 15)) and R.DECODER_STATE[-1] == ("decoder.12.bias", (768,))
    assert float(Z["bn_eps"]) == R.BN_EPS


def test_batchnorm_state_is_not_the_identity():
    st = R.encoder_state(7)
    seen = 0
    for k, v in st.items():
        if int(k.split(".")[1]) % 3 == 1:
            lo, hi = dict(running_mean=(-0.2, 0.2), running_var=(0.05, 1.5), weight=(0.5, 1.5), bias=(-0.3, 0.3))[k.split(".")[2]]
            assert float(v.min()) >= lo and float(v.max()) <= hi and float(v.std()) > 0.05 * (hi - lo), k
            seen += 1
    assert seen == 4 * 5


def _f32_rule(label, o64, o32, g64, g32, recorded):
    e64 = np.abs(o64.numpy() - g64).max()
    d32 = np.abs(o32.numpy().astype(np.float64) - g32.astype(np.float64)).max()
    e32 = np.abs(o32.numpy().astype(np.float64) - g64).max()
    print(f"{label}: float64 {e64:.3e}; float32 {'identical to' if d32 == 0 else f'within {d32:.3e} of'} the recorded run "
          f"(its error against float64: {e32:.3e} here, {recorded:.3e} recorded)")
    assert e64 <= 1e-12
    assert d32 <= recorded


@pytest.mark.parametrize("key", list(R.ENCODE_CASES))
def test_encode_inputs_are_rebuilt_bit_for_bit(Z, key):
    shape, seed = R.ENCODE_CASES[key]
    _, features = R.make_encode_case(key)
    assert int(Z[f"{key}_seed"]) == seed and tuple(features.shape) == tuple(shape)
    assert np.array_equal(features.numpy(), Z[f"{key}_features"])
    assert float(Z[f"{key}_min_h6_norm"]) >= 0.1


@pytest.mark.parametrize("key", list(R.ENCODE_CASES))
def test_encode_reproduces_the_reference(Z, key):
    state, _ = R.make_encode_case(key)
    features = torch.from_numpy(Z[f"{key}_features"])
    o64, o32 = R.encode(state, features, torch.float64), R.encode(state, features, torch.float32)
    g64, g32 = Z[f"{key}_out_f64"], Z[f"{key}_out_f32"]
    assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and tuple(o64.shape) == g64.shape == g32.shape
    assert g64.shape[1] == 15
    _f32_rule(key, o64, o32, g64, g32, float(Z[f"{key}_out_f32_maxerr"]))
    assert float((o64.norm(dim=1) - 1).abs().max()) <= 1e-14


def test_decode_reproduces_the_reference(Z):
    dec_state, rows, phrases = R.make_decode_case()
    assert np.array_equal(rows.numpy(), Z["decode_codes"]) and np.array_equal(phrases.numpy(), Z["decode_phrases"])
    assert tuple(int(k) for k in Z["decode_kept"]) == R.DECODE_KEPT and float(Z["decode_min_y_norm"]) >= 0.1
    assert Z["decode_sims_f64"].shape == (R.DECODE_PHRASES, R.DECODE_ROWS) and Z["decode_features_f64"].shape == (10, 768)
    codes = rows.t().reshape(15, 1, -1)
    s64, s32 = (R.similarities(codes, dec_state, phrases, dt)[:, 0] for dt in (torch.float64, torch.float32))
    g64, g32 = Z["decode_sims_f64"], Z["decode_sims_f32"]
    _f32_rule("similarities", s64, s32, g64, g32, float(np.abs(g32.astype(np.float64) - g64).max()))
    kept = list(R.DECODE_KEPT)
    f64, f32 = R.decode(dec_state, rows, torch.float64)[kept], R.decode(dec_state, rows, torch.float32)[kept]   # as recorded
    g64, g32 = Z["decode_features_f64"], Z["decode_features_f32"]
    _f32_rule("features", f64, f32, g64, g32, float(np.abs(g32.astype(np.float64) - g64).max()))
    assert float((f64.norm(dim=1) - 1).abs().max()) <= 1e-14


def test_chunked_rows_equal_one_pass_and_the_cases_are_clear_of_zero_rows():
    state, features = R.make_encode_case("rows70")
    a, b = R.encode(state, features, torch.float64), R.encode(state, features, torch.float64, chunk=16)
    assert float((a - b).abs().max()) <= 1e-15
    dec_state, rows, _ = R.make_decode_case()
    h6, y = R.least_norms(state, features, dec_state, rows)
    assert h6 >= 0.1 and y >= 0.1
