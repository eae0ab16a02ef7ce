"""tests/hr_net_ref.py against tests/golden/hr_net.npz: arrays recorded from the reference's own HighResLanguageFeatureNet
(tests/golden/make_golden_hr_net.py) on 32 output channels, in float64 and float32, with the float32 run's error over the whole
output.  Pins the restatement the GPU tests measure against, and the tap table of the ConvTranspose2d phases, without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hr_net_ref as R


@pytest.fixture(scope="module")
def z():
    return R.golden()


def test_the_file_holds_what_the_cases_say(z):
    assert float(z["bn_eps"]) == R.BN_EPS and tuple(int(c) for c in z["channels"]) == R.GOLDEN_CHANNELS
    assert [str(k) for k in z["state_names"]] == [k for k, _ in R.STATE]
    assert sum(int(np.prod(s)) for _, s in R.STATE) == R.N_PACKED
    for key, (sizes, seed) in R.GOLDEN_CASES.items():
        assert int(z[f"{key}_seed"]) == seed
        for name, c, (h, w) in zip(("fv", "f3", "f2"), (R.C_FV, R.C_F3, R.C_F2), sizes):
            assert z[f"{key}_{name}"].shape == (c, h, w) and z[f"{key}_{name}"].dtype == np.float32
        shape = (32, 8 * sizes[0][0], 8 * sizes[0][1])
        assert z[f"{key}_out_f64"].shape == shape and z[f"{key}_out_f64"].dtype == np.float64
        assert z[f"{key}_out_f32"].shape == shape and z[f"{key}_out_f32"].dtype == np.float32
        # the recorded error of the whole float32 output bounds the error on the subset
        d = np.abs(z[f"{key}_out_f32"].astype(np.float64) - z[f"{key}_out_f64"])
        assert 0 < d.max() <= float(z[f"{key}_out_f32_maxerr"]) < 1e-6 * max(1.0, float(z[f"{key}_out_absmax"]))


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_restatement_against_the_reference_module(z, key):
    state, inputs = R.make_case(key)
    for name, x in zip(("fv", "f3", "f2"), inputs):
        assert torch.equal(x, torch.from_numpy(z[f"{key}_{name}"])), name
    ch = list(R.GOLDEN_CHANNELS)
    t64 = torch.from_numpy(z[f"{key}_out_f64"])
    mine64 = R.forward(state, *inputs, torch.float64)
    assert float((mine64[ch] - t64).abs().max()) <= 1e-12
    # float32: within the reference's own float32 error, on the subset and (against the float64 restatement) everywhere
    mine32 = R.forward(state, *inputs, torch.float32)
    emax, erms = float(z[f"{key}_out_f32_maxerr"]), float(z[f"{key}_out_f32_rmserr"])
    assert R.err(mine32[ch], t64)[0] <= emax
    got = R.err(mine32, mine64)
    assert got[0] <= emax and got[1] <= erms * (1 + 1e-9)
    # the kernel-order evaluation is a float32 evaluation of the same function: the GPU tests' rule has room for it
    ko = R.err(R.forward_kernel_order(state, *inputs), mine64)
    print(f"{key}: ref32 max {emax:.3e} rms {erms:.3e}; kernel order max {ko[0]:.3e} rms {ko[1]:.3e}")
    assert ko[0] < 2 * emax and ko[1] < 2 * erms


def test_phase_taps_are_pytorch_s():
    """oy = 2 iy - 1 + ky: every (output row, kernel row) pair of ConvTranspose2d(4, 2, 1) appears in exactly one phase."""
    assert R.phase_taps(0) == ((-1, 3), (0, 1)) and R.phase_taps(1) == ((0, 2), (1, 0))
    for parity in (0, 1):
        for d, k in R.phase_taps(parity):
            m = 5
            assert 2 * (m + d) - 1 + k == 2 * m + parity
    assert sorted(k for p in (0, 1) for _, k in R.phase_taps(p)) == [0, 1, 2, 3]


@pytest.mark.parametrize("shape", [(1, 1), (1, 4), (3, 1), (3, 5), (8, 9)])
def test_phase_decomposition_equals_conv_transpose2d(shape):
    g = torch.Generator().manual_seed(31 + shape[0] * 16 + shape[1])
    x = torch.randn(1, 6, *shape, generator=g, dtype=torch.float64)
    w = torch.randn(6, 5, 4, 4, generator=g, dtype=torch.float64)
    b = torch.randn(5, generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    got = R.conv_transpose_phases(x, w, b)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("size", [((5, 7), (10, 14)), ((5, 7), (5, 7)), ((9, 11), (4, 7)), ((1, 1), (2, 2)), ((6, 3), (6, 5))])
def test_bilinear_restatement(size):
    """The kernel's sampling rule against F.interpolate in float64 (float32 rounding of the coordinates only), and a NaN stays
    where F.interpolate keeps it when a dimension keeps its size."""
    (h, w), (H, W) = size
    g = torch.Generator().manual_seed(h * 100 + W)
    x = torch.randn(1, 3, h, w, generator=g, dtype=torch.float64).float()
    want = F.interpolate(x.double(), size=(H, W), mode="bilinear", align_corners=False)
    assert float((R.bilinear32(x, H, W).double() - want).abs().max()) <= 8 * 2.0 ** -24 * float(x.abs().max())
    x[0, 1, h // 2, w // 2] = float("nan")
    assert torch.equal(torch.isnan(R.bilinear32(x, H, W)), torch.isnan(F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False)))
