"""tests/lang_encoder_ref.py against tests/golden/lang_encoder.npz: arrays recorded from the reference's own AutoencoderMLP
(language/autoencoder/model.py) in eval(), encode in float64 and float32 on 70 rows and on a 9 x 13 channel-major map.  The
restatement must reproduce the float64 output to 1e-12 and rebuild the inputs bit for bit.  The float32 output: identical
where the file was made (the same torch, the same thread count); torch's CPU GEMM may block another way with another
thread count or build, so the bound is 2 ulp per element, and the test prints which of the two it found."""
import numpy as np
import pytest
import torch

import lang_encoder_ref as R


@pytest.fixture(scope="module")
def Z():
    return R.golden()


def test_state_layout_is_the_encoders(Z):
    names = [str(k) for k in Z["state_names"]]
    shapes = [tuple(int(d) for d in s if d) for s in Z["state_shapes"]]
    assert [k for k, _ in R.STATE] == names and [tuple(s) for _, s in R.STATE] == shapes
    assert sum(int(np.prod(s)) for s in shapes) == R.N_ENCODER == 568288 + 3840
    assert float(Z["bn_eps"]) == R.BN_EPS
    # state_dict order of the module itself, num_batches_tracked left out
    sd = R.GeneralAutoencoder().state_dict()
    assert [k for k in sd if k.startswith("encoder.") and not k.endswith("num_batches_tracked")] == names


def test_batchnorm_state_is_not_the_identity():
    st = R.encoder_state(7)
    for k, v in st.items():
        if int(k.split(".")[1]) % 3 == 1:
            lo, hi = dict(running_mean=(-0.2, 0.2), running_var=(0.05, 1.5), weight=(0.5, 1.5), bias=(-0.3, 0.3))[k.split(".")[2]]
            assert float(v.min()) >= lo and float(v.max()) <= hi and float(v.std()) > 0.05 * (hi - lo), k


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_inputs_are_rebuilt_bit_for_bit(Z, key):
    shape, seed = R.GOLDEN_CASES[key]
    _, features = R.make_case(key)
    assert int(Z[f"{key}_seed"]) == seed and tuple(features.shape) == tuple(shape)
    assert np.array_equal(features.numpy(), Z[f"{key}_features"])
    rows = R.rows_of(features).double()
    assert float((rows.norm(dim=1) - 1).abs().max()) <= 2.0 ** -23
    assert float(Z[f"{key}_min_h5_norm"]) >= 0.1


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_restatement_reproduces_the_reference(Z, key):
    state, _ = R.make_case(key)
    features = torch.from_numpy(Z[f"{key}_features"])
    o64, o32 = R.encode(state, features, torch.float64), R.encode(state, features, torch.float32)
    g64, g32 = Z[f"{key}_out_f64"], Z[f"{key}_out_f32"]
    assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and tuple(o64.shape) == g64.shape == g32.shape
    e64 = np.abs(o64.numpy() - g64).max()
    d32 = np.abs(o32.numpy().astype(np.float64) - g32.astype(np.float64))
    ulps = (d32 / np.spacing(np.maximum(np.abs(o32.numpy()), np.abs(g32)))).max()
    e32 = np.abs(o32.numpy().astype(np.float64) - g64).max()
    print(f"{key}: float64 {e64:.3e}; float32 {'identical to' if d32.max() == 0 else f'within {ulps:.2f} ulp of'} the recorded run "
          f"(its error against float64: {e32:.3e} here, {float(Z[f'{key}_out_f32_maxerr']):.3e} recorded)")
    assert e64 <= 1e-12
    assert ulps <= 2.0
    # rows of a unit output
    assert float((o64.norm(dim=1) - 1).abs().max()) <= 1e-14


def test_chunked_rows_equal_one_pass():
    state, features = R.make_case("rows70")
    a, b = R.encode(state, features, torch.float64), R.encode(state, features, torch.float64, chunk=16)
    assert float((a - b).abs().max()) <= 1e-15
    assert R.least_h5_norm(state, features) >= 0.1
