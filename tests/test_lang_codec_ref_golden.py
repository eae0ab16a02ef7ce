"""tests/lang_codec_ref.py (the yardstick of tests/test_gpu_lang_codec.py) against arrays recorded from the reference's own
EncoderDecoderOnline driven through train_online_autoencoder's statements (tests/golden/make_golden_lang_codec.py ->
lang_codec.npz), on the CPU.

Tolerance of the float64 comparison: 1e-9 of the recorded array's largest magnitude.  The restatement runs the same torch
modules on the same inputs, so it is normally the same bits; float64 rounding (1.1e-16) through ~100 operations per row and
30 Adam steps (whose m / sqrt(v) is scale-free) stays below 1e-12, and a wrong layer, norm or loss weight shows at 1e-3."""
import numpy as np
import pytest
import torch

import lang_codec_ref as R

CASES = R.golden_cases()
SUB = slice(None, None, R.CODE_ROW_STRIDE)


def test_golden_covers_the_cases():
    z = R.golden()
    assert [(n, s) for _, n, s in CASES] == [(n, s) for n in (1000, 257) for s in (0, 1, 2, 3)]
    assert float(z["lr"]) == 1e-3 and int(z["steps"]) == 30 and float(z["tau"]) == R.TAU == 1e-5
    assert [str(k) for k in z["state_names"]] == [k for k, _ in R.STATE]
    assert [tuple(int(d) for d in s if d) for s in z["state_shapes"]] == [tuple(s) for _, s in R.STATE]
    for key, N, _ in CASES:
        assert z[f"{key}_params"].shape == (R.N_PARAMS,) and z[f"{key}_params"].dtype == np.float32
        assert z[f"{key}_q"].shape == (N, 32) and z[f"{key}_q"].dtype == np.int16
        assert z[f"{key}_grad0_f64"].dtype == np.float64 and z[f"{key}_grad0_f32"].dtype == np.float32
        assert z[f"{key}_loss_f64"].shape == (30, 4)
        assert z[f"{key}_loss_f64"][-1, 0] < z[f"{key}_loss_f64"][0, 0]          # 30 steps at 1e-3 do train


@pytest.mark.parametrize("key,N,seed", CASES)
def test_features_and_tie_filter(key, N, seed):
    z = R.golden()
    x = R.unit(z[f"{key}_q"])
    assert x.dtype == torch.float32 and float((x.double().norm(dim=1) - 1).abs().max()) <= 2.0 ** -22
    # rank-6 mixture + 10 % noise: six singular values carry the rows, the rest is the noise floor
    sv = torch.linalg.svdvals(x.double())
    assert float((sv[:6] ** 2).sum() / (sv ** 2).sum()) > 0.97 and float(sv[6] / sv[0]) > 0.01
    flat = torch.from_numpy(z[f"{key}_params"])
    assert int(R.tie_rows(flat, x).sum()) == 0                                  # no tie rows are left ...
    assert int(z[f"{key}_redrawn"]) <= 0.01 * N                                 # ... and at most 1 % were redrawn
    # default nn.Linear initialisation: uniform in +-1/sqrt(fan_in)
    for (name, shape), v in zip(R.STATE, R.unflatten(flat).values()):
        fan_in = {"encoder.0": 32, "encoder.2": 24, "decoder.0": 15, "decoder.2": 24}[name.rsplit(".", 1)[0]]
        assert float(v.abs().max()) <= fan_in ** -0.5, name


@pytest.mark.parametrize("key,N,seed", CASES)
def test_ref_equals_reference_in_float64(key, N, seed):
    z = R.golden()
    flat, x = torch.from_numpy(z[f"{key}_params"]), R.unit(z[f"{key}_q"])
    t = R.train(flat, x, float(z["lr"]), int(z["steps"]), torch.float64)
    for name, got in (("loss", t["loss"]), ("grad0", t["grad0"]), ("codes_pre0", t["codes_pre0"][SUB]),
                      ("codes_post0", t["codes_post0"][SUB]), ("params30", t["params"]), ("codes_post30", t["codes_post"][SUB])):
        want = z[f"{key}_{name}_f64"]
        scale, err = np.abs(want).max(), np.abs(got.numpy() - want).max()
        print(f"{key} {name}: max error {err:.3e} on a largest magnitude of {scale:.3e}")
        assert err <= 1e-9 * scale, (name, err, scale)


@pytest.mark.parametrize("key,N,seed", CASES)
def test_ref_in_float32_is_the_reference_in_float32(key, N, seed):
    """lang_codec_ref evaluated in float32 is the `ref32` of the full-size GPU cases: its error against the truth must be of
    the size of the reference's own float32 error (the rule of tests/test_gpu_lang_codec.py)."""
    z = R.golden()
    flat, x = torch.from_numpy(z[f"{key}_params"]), R.unit(z[f"{key}_q"])
    t = R.train(flat, x, float(z["lr"]), int(z["steps"]), torch.float32)
    assert t["grad0"].dtype == torch.float32
    truth, ref32 = z[f"{key}_grad0_f64"], z[f"{key}_grad0_f32"].astype(np.float64)
    e_got, e_ref = np.abs(t["grad0"].double().numpy() - truth), np.abs(ref32 - truth)
    rms = lambda e: float(np.sqrt((e ** 2).mean()))  # noqa: E731
    print(f"{key}: gradient max {e_got.max():.3e} / {e_ref.max():.3e}, rms {rms(e_got):.3e} / {rms(e_ref):.3e}")
    assert e_got.max() <= 4.0 * e_ref.max() and rms(e_got) <= 4.0 * rms(e_ref)
    lt, l32 = z[f"{key}_loss_f64"], z[f"{key}_loss_f32"].astype(np.float64)
    for i in range(lt.shape[0]):
        for k in range(4):
            assert abs(float(t["loss"][i, k]) - lt[i, k]) <= max(4.0 * abs(l32[i, k] - lt[i, k]), 4.0 * 2.0 ** -24), (i, k)
    for name, got in (("codes_pre0", t["codes_pre0"][SUB]), ("codes_post0", t["codes_post0"][SUB]), ("params30", t["params"]),
                      ("codes_post30", t["codes_post"][SUB])):
        err = np.abs(got.double().numpy() - z[f"{key}_{name}_f64"]).max()
        assert err <= max(4.0 * float(z[f"{key}_{name}_f32_maxerr"]), 4.0 * 2.0 ** -24), (name, err)
