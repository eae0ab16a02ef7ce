"""tests/lang_query_ref.py against tests/golden/lang_query.npz: arrays recorded from the reference's own decoders
(language/autoencoder/model.py), OpenCLIPNetwork.get_relevancy / get_max_across / get_semantic_map
(eval/openclip_encoder.py) and torch's F.interpolate for evaluate_onlinelangslam.py:270-274, in float64 and float32.  The
restatement must reproduce the float64 arrays to float64 rounding, the float32 relevancy to float32 rounding, and rebuild the
cases' inputs bit for bit.  The 30 x 30 mean is compared with what scipy.ndimage.correlate(mode="mirror") gave when the file
was made: cv2 was not available there, so that part is pinned by restatement, not by running the reference's call."""
import numpy as np
import pytest
import torch

import lang_query_ref as R


@pytest.fixture(scope="module")
def Z():
    return R.golden()


def _case(Z, key):
    h, w, decode_hw, out_hw, seed, n_pos, n_lab = R.GOLDEN_CASES[key]
    case = R.make_case(h, w, seed, n_pos, n_lab)
    return case, decode_hw, out_hw, n_pos, n_lab


def test_state_layout_is_the_decoders(Z):
    names = [str(k) for k in Z["state_names"]]
    shapes = [tuple(int(d) for d in s if d) for s in Z["state_shapes"]]
    assert [k for k, _ in R.STATE] == names and [tuple(s) for _, s in R.STATE] == shapes
    assert sum(int(np.prod(s)) for s in shapes) == R.N_DECODER


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_inputs_are_rebuilt_bit_for_bit(Z, key):
    case, *_ = _case(Z, key)
    assert int(Z[f"{key}_seed"]) == R.GOLDEN_CASES[key][4]
    assert np.array_equal(case["neg"].numpy(), Z[f"{key}_neg"])
    # the codes go through a bicubic resize and the phrases through a float64 decode: the recorded arrays are the inputs of the
    # GPU tests; a rebuild must agree to rounding
    assert np.abs(case["codes"].numpy() - Z[f"{key}_codes"]).max() <= 2e-7
    assert np.abs(case["pos"].numpy() - Z[f"{key}_pos"]).max() <= 2e-7


def golden_case(Z, key):
    """The case with its recorded inputs."""
    case, decode_hw, out_hw, n_pos, n_lab = _case(Z, key)
    case["codes"], case["pos"], case["neg"] = (torch.from_numpy(Z[f"{key}_{n}"]) for n in ("codes", "pos", "neg"))
    if n_lab:
        case["labels"] = torch.from_numpy(Z[f"{key}_label_embeds"])
    return case, decode_hw, out_hw


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_restatement_reproduces_the_reference(Z, key):
    case, decode_hw, out_hw = golden_case(Z, key)
    q64 = R.query(case["codes"], case["online"], case["dec_state"], case["pos"], case["neg"], case["labels"], torch.float64,
                  thresh=float(Z["thresh"]), decode_hw=decode_hw, out_hw=out_hw)
    q32 = R.query(case["codes"], case["online"], case["dec_state"], case["pos"], case["neg"], case["labels"], torch.float32,
                  thresh=float(Z["thresh"]), decode_hw=decode_hw, out_hw=out_hw)
    e = np.abs(q64["relevancy"].numpy() - Z[f"{key}_relevancy_f64"]).max()
    e32 = np.abs(q32["relevancy"].numpy() - Z[f"{key}_relevancy_f32"]).max()
    es = np.abs(q64["smoothed"].numpy() - Z[f"{key}_smoothed_f64"]).max()
    print(f"{key}: relevancy float64 {e:.3e}, float32 {e32:.3e}; smoothed against scipy {es:.3e}")
    assert e <= 1e-13 and es <= 1e-13
    assert e32 <= 4 * 2.0 ** -24        # the row-block products may round otherwise than one torch.mm: two ulp at 0.5
    if case["labels"] is not None:
        assert np.array_equal(q64["labels"].numpy(), Z[f"{key}_labels_f64"])
        differ = int((q32["labels"].numpy() != Z[f"{key}_labels_f32"]).sum())
        assert differ <= R.EXCLUDED_CAP * q32["labels"].numel(), differ


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_features_and_interpolation(Z, key):
    """The 768-channel rows (every 97th) and the resized codes: model.decode(model_online.decode(.)) and both F.interpolate
    statements; resize_rows, which writes the feature interpolation out for row blocks, is held to F.interpolate's result."""
    from lang_codec_ref import codec_from
    case, decode_hw, out_hw = golden_case(Z, key)
    codec, dec = codec_from(case["online"], torch.float64), R.decoder_from(case["dec_state"], torch.float64)
    with torch.no_grad():
        c = case["codes"].double()
        if decode_hw is not None:
            c = R.resize(c, decode_hw)
        assert np.abs(c.numpy() - Z[f"{key}_codes_resized_f64"]).max() <= 1e-15
        h, w = c.shape[1:]
        feat = R.features(c.permute(1, 2, 0).reshape(-1, 15), codec, dec).view(h, w, -1)
        if out_hw is not None and tuple(out_hw) != (h, w):
            up = R.resize_rows(feat, R.taps(h, out_hw[0], torch.float64), R.taps(w, out_hw[1], torch.float64))
            lit = R.resize(feat.permute(2, 0, 1), out_hw).permute(1, 2, 0)
            assert float((up - lit).abs().max()) <= 1e-15
            feat = up
    rows = feat.reshape(-1, 768)[::int(Z["feat_row_stride"])].numpy()
    e = np.abs(rows - Z[f"{key}_feat_f64"]).max()
    print(f"{key}: features float64 {e:.3e} (the float32 run of the reference: {float(Z[f'{key}_feat_f32_maxerr']):.3e})")
    assert e <= 1e-14


def test_ref32_stays_inside_the_discrete_cap(Z):
    for key in R.GOLDEN_CASES:
        h, w, _, out_hw, *_ = R.GOLDEN_CASES[key]
        H, W = (h, w) if out_hw is None else out_hw
        assert int(Z[f"{key}_excluded_ref32"].max()) <= R.EXCLUDED_CAP * H * W


def test_reflect101_is_opencvs_table():
    # gfedcb|abcdefgh|gfedcba, and the periodic continuation for a window wider than the axis
    assert list(R.reflect101(np.arange(-6, 8 + 7), 8)) == [6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1, 0]
    assert list(R.reflect101(np.arange(-5, 6), 1)) == [0] * 11
    assert list(R.reflect101(np.arange(-4, 6), 2)) == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert list(R.reflect101(np.arange(-4, 7), 3)) == [0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2]
