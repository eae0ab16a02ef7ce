"""olsr_lang_query_sims / olsr_lang_query_relevancy (HIP) and lang_query.LanguageQuery on the GPU.

Yardstick for the continuous outputs (similarities, relevancy, smoothed and blended maps, score, min / max): the one of
tests/test_gpu_lang_codec.py, imported from there unchanged.  With `truth` the float64 and `ref32` the float32 evaluation of
the reference's statements (tests/golden/lang_query.npz for the golden cases' relevancy; tests/lang_query_ref.py, which
tests/test_lang_query_ref_golden.py pins to that file, for everything else and for the full sizes):
    max and rms of |hip - truth| <= max(4 x the same of ref32, 4 * 2^-24 max|truth|);  scalars alike.
Design-time evidence that 4x fits another summation order (CPU, N = 4096, default initialisation, every layer accumulated in
K-chunks of 4 and of 64): feature errors 4.0e-8 / 2.9e-8 max against ref32's 4.2e-8, relevancy errors 1.43e-7 / 1.24e-7 against
1.46e-7: ratios 0.7 - 1.0.  Every figure is printed.

Discrete outputs (mask, label map, coordinate).  A pixel may differ from the truth's only where the truth's deciding value
lies within the continuous tolerance of that value (the normalised map of evaluate_onlinelangslam.py:146-150 against thresh,
with the tolerance max(4 max|ref32 - truth|, 4 * 2^-24 max|truth|) of that map; the best against the second-best similarity
with the tolerance of the similarities); such pixels may be at most 0.1 % of a map.  The coordinate passes if the truth's
averaged map at the returned point is within the averaged map's tolerance of the truth's maximum.
"""
import ctypes as C

import pytest
import torch

import lang_codec_ref as RC
import lang_query_ref as R
from test_gpu_lang_codec import _raises_exactly, _ratio_rule, _scalar_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


_tolerance = R.tolerance


def _query(case):
    from online_lang_splatting_amd.lang_codec import OnlineLanguageCodec
    from online_lang_splatting_amd.lang_query import LanguageDecoder, LanguageQuery
    codec = OnlineLanguageCodec(DEV, seed=0)
    codec.load_state_dict(RC.unflatten(case["online"]))
    dec = LanguageDecoder(DEV, case["dec_state"])
    assert torch.equal(dec.flat.cpu(), R.flatten(case["dec_state"]))
    q = LanguageQuery(dec, codec)
    q.thresh = R.THRESH
    q.set_phrases(case["pos"].to(DEV), case["neg"].to(DEV))
    q.set_labels(None if case["labels"] is None else case["labels"].to(DEV))
    return q


def _reference(case, decode_hw, out_hw):
    args = (case["codes"], case["online"], case["dec_state"], case["pos"], case["neg"], case["labels"])
    return (R.query(*args, torch.float64, thresh=R.THRESH, decode_hw=decode_hw, out_hw=out_hw),
            R.query(*args, torch.float32, thresh=R.THRESH, decode_hw=decode_hw, out_hw=out_hw))


def _check_discrete(label, what, differs, deciding, tol, n_map):
    """differs: bool map hip != truth; deciding: the truth's distance from the decision."""
    near = deciding.abs() <= tol
    bad, excluded = int((differs & ~near).sum()), int(near.sum())
    print(f"{label} {what}: {int(differs.sum())} pixels differ from the truth's, {bad} of them outside the tolerance {tol:.3e}; "
          f"{excluded} of {n_map} pixels ({excluded / n_map:.5f}) lie within it")
    assert bad == 0, (label, what, bad)
    assert excluded <= R.EXCLUDED_CAP * n_map, (label, what, excluded, n_map)


def _check(label, case, decode_hw=None, out_hw=None, truth=None):
    """Every output of one query against the reference's statements.  truth: (t64, t32) if the caller has them already."""
    t64, t32 = truth if truth is not None else _reference(case, decode_hw, out_hw)
    q = _query(case)
    out = q.relevancy(case["codes"].to(DEV), out_hw=out_hw, decode_hw=decode_hw)
    torch.cuda.synchronize()
    hip = {k: v.cpu().clone() for k, v in out.items()}
    _check_outputs(label, case, hip, t64, t32)
    return q, hip


def _check_outputs(label, case, hip, t64, t32):
    """hip: the outputs of one query (relevancy()'s dict, on the CPU) against the reference's statements."""
    P, H, W = hip["relevancy"].shape
    assert tuple(hip["similarities"].shape) == tuple(t64["sims_dec"].shape)
    _ratio_rule(f"{label} similarities", hip["similarities"], t64["sims_dec"], t32["sims_dec"])
    for name in ("relevancy", "smoothed", "blended"):
        _ratio_rule(f"{label} {name}", hip[name], t64[name], t32[name])
    for p in range(P):
        _scalar_rule(f"{label} score[{p}]", hip["score"][p], t64["score"][p], t32["score"][p])
        _scalar_rule(f"{label} min[{p}]", hip["minmax"][p, 0], t64["minmax"][p, 0], t32["minmax"][p, 0])
        _scalar_rule(f"{label} max[{p}]", hip["minmax"][p, 1], t64["minmax"][p, 1], t32["minmax"][p, 1])
    # the mask: decided by the normalised map against thresh
    assert hip["mask"].dtype == torch.uint8 and int(hip["mask"].max()) <= 1
    tol_n = _tolerance(t64["normed"], t32["normed"])
    tol_s = _tolerance(t64["smoothed"], t32["smoothed"])
    for p in range(P):
        _check_discrete(label, f"mask[{p}]", hip["mask"][p] != t64["mask"][p], t64["normed"][p] - R.THRESH, tol_n, H * W)
        x, y = int(hip["coord"][p, 0]), int(hip["coord"][p, 1])
        assert 0 <= x < W and 0 <= y < H
        gap = float(t64["score"][p] - t64["smoothed"][p, y, x])
        print(f"{label} coord[{p}] = ({x}, {y}); the truth's {t64['coords'][p].tolist()[:3]}; the truth's averaged map there is "
              f"{gap:.3e} below its maximum (tolerance {tol_s:.3e})")
        assert 0.0 <= gap <= tol_s
        # and it is the first pixel in row-major order that holds the device's own maximum
        flat = hip["smoothed"][p].reshape(-1)
        assert float(flat[y * W + x]) == float(hip["score"][p]) == float(flat.max())
        assert int((flat == flat.max()).nonzero()[0]) == y * W + x
    if case["labels"] is not None:
        assert hip["labels"].dtype == torch.int32 and tuple(hip["labels"].shape) == (H, W)
        assert int(hip["labels"].min()) >= -1 and int(hip["labels"].max()) < case["labels"].shape[0]
        _check_discrete(label, "labels", hip["labels"].long() != t64["labels"], t64["label_margin"],
                        _tolerance(t64["sims"], t32["sims"]), H * W)
    else:
        assert "labels" not in hip


def _golden_case(key):
    from test_lang_query_ref_golden import golden_case
    Z = R.golden()
    case, decode_hw, out_hw = golden_case(Z, key)
    t64, t32 = _reference(case, decode_hw, out_hw)
    # the relevancy is the recorded one (the reference's own get_max_across), not the restatement's
    t64["relevancy"], t32["relevancy"] = torch.from_numpy(Z[f"{key}_relevancy_f64"]), torch.from_numpy(Z[f"{key}_relevancy_f32"])
    return case, decode_hw, out_hw, (t64, t32)


@pytest.mark.parametrize("key", list(R.GOLDEN_CASES))
def test_golden(hip, key):
    case, decode_hw, out_hw, truth = _golden_case(key)
    _check(f"golden {key}", case, decode_hw, out_hw, truth)


# h, w, positives, labels: no multiple of any tile, one row, one column, the mapping loop's target size; P = 1 and P = 8
@pytest.mark.parametrize("h,w,n_pos,n_labels", [(101, 157, 3, 0), (1, 300, 2, 3), (300, 1, 2, 0), (192, 192, 1, 5),
                                               (67, 45, 8, 0), (33, 64, 8, 8)])
def test_sizes_and_phrase_counts(hip, h, w, n_pos, n_labels):
    case = R.make_case(h, w, 10 + n_pos, n_pos, n_labels)
    _check(f"{w} x {h}, P = {n_pos}, L = {n_labels}", case)


def test_decode_small_and_upsample_full_size(hip):
    """The reference's evaluation sequence: the codes resized to 640 x 480, decoded there, the result brought back to
    1200 x 680 (here: the similarity planes; the reference: the 768-channel features, which the restatement follows)."""
    case = R.make_case(680, 1200, 4, 3, 0)
    _check("1200 x 680 via 640 x 480", case, decode_hw=(480, 640), out_hw=(680, 1200))


def test_full_size_direct(hip):
    case = R.make_case(680, 1200, 5, 3, 4)
    _check("1200 x 680 direct", case)


def test_resampling_shapes(hip):
    """Down and up by factors that are no integers, and an output size of its own."""
    case = R.make_case(90, 120, 6, 2, 3)
    _check("120 x 90 -> 77 x 50 -> 131 x 95", case, decode_hw=(50, 77), out_hw=(95, 131))


def test_repeat_and_identity_resize_are_bit_identical(hip):
    case = R.make_case(101, 157, 7, 3, 4)
    q = _query(case)
    codes = case["codes"].to(DEV)
    a = {k: v.clone() for k, v in q.relevancy(codes).items()}
    b = {k: v.clone() for k, v in q.relevancy(codes).items()}
    c = {k: v.clone() for k, v in q.relevancy(codes, out_hw=(101, 157), decode_hw=(101, 157)).items()}
    assert set(a) == set(b) == set(c) and "labels" in a
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.equal(a[k], c[k]), k
    s = q.similarities(codes).clone()
    assert torch.equal(s, a["similarities"]) and torch.equal(q.similarities(codes, decode_hw=(101, 157)), s)
    # buffers are reused
    assert q.similarities(codes).data_ptr() == q.similarities(codes).data_ptr()


def test_similarities_are_the_composition_of_the_two_decoders(hip):
    """similarities of a [15,N] view against OnlineLanguageCodec.decode (HIP) -> the general decoder and the products in torch,
    float64 as truth and float32 as ref32."""
    N = 5000
    case = R.make_case(50, 100, 8, 3, 2)
    q = _query(case)
    flat_codes = case["codes"].reshape(15, N).to(DEV)
    sims = q.similarities(flat_codes).cpu()
    assert tuple(sims.shape) == (3 + 2 + 4, 1, N)
    rows32 = q.codec.decode(flat_codes, layout="channels").cpu()
    phrases = torch.cat([case["pos"], case["labels"], case["neg"]])
    with torch.no_grad():
        t = [torch.mm(R.decoder_from(case["dec_state"], dt).decode(rows32.to(dt)), phrases.to(dt).T).T for dt in (torch.float64, torch.float32)]
    _ratio_rule("composition", sims.reshape(-1, N), t[0], t[1])


def test_peak_memory_has_no_feature_image(hip):
    """A 1200 x 680 query allocates its outputs and the scratch the library asks for, nothing else: no 768-wide (or 512-wide)
    image.  The scratch is below 64 N bytes at K = 7."""
    from online_lang_splatting_amd import _abi
    from online_lang_splatting_amd._lib import lib
    H, W = 680, 1200
    N = H * W
    case = R.make_case(40, 48, 0, 3, 0)
    q = _query(case)
    codes = torch.rand(15, H, W, device=DEV) - 0.5
    p = _abi.OlsrLangQueryParams(n_widths=6, K=7, n_pos=3, out_width=W, out_height=H, dec_width=W, dec_height=H, in_width=W, in_height=H)
    scratch = lib().olsr_lang_query_scratch_bytes(C.byref(p))
    assert scratch < 64 * N
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = q.relevancy(codes)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    outputs = sum(v.numel() * v.element_size() for v in out.values())
    # torch's caching allocator hands out a large block whole when splitting it would leave less than 1 MiB, and counts the
    # whole block as allocated: every buffer may weigh up to 1 MiB more than it holds (9 MiB here; a 768-wide image is 2.5 GB)
    slack = (1 << 20) * (len(out) + 1)
    requested = torch.cuda.memory_stats().get("requested_bytes.all.peak")
    print(f"1200 x 680, K = 7: peak grew by {grown} bytes (requested peak, whole process: {requested}); outputs {outputs}, "
          f"scratch {scratch}, allocator slack allowed {slack}; a [N,768] float32 image would be {N * 768 * 4}")
    assert grown <= outputs + scratch + slack
    assert outputs + scratch < 64 * N + 7 * 4 * N + 3 * (3 * 4 + 1) * N


def test_errors_are_raised_not_copied(hip):
    case = R.make_case(40, 48, 0, 3, 0)
    q = _query(case)
    codes = case["codes"].to(DEV)
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        q.relevancy(case["codes"])
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        q.similarities(codes.double())
    with pytest.raises(RuntimeError, match=r"expected \[15,h,w\]"):
        q.relevancy(codes[:14])
    with pytest.raises(RuntimeError, match="float32 tensor on the GPU"):
        q.set_phrases(case["pos"], case["neg"].to(DEV))
    with pytest.raises(RuntimeError, match="at most 64"):
        q.set_labels(torch.zeros(60, 768, device=DEV))
    assert q.counts == (3, 0, 4)
    from online_lang_splatting_amd.lang_query import LanguageQuery
    fresh = LanguageQuery(q.decoder, q.codec)
    with pytest.raises(RuntimeError, match="set_phrases first"):
        fresh.similarities(codes)


def test_query_on_a_rendered_language_map(hip):
    """End to end: render(...)["language"] of a small scene goes into the query as it is ([15,H,W], channel-major, with empty
    pixels whose code is the zero vector) and is held to the reference's statements on the same tensor."""
    import math
    from types import SimpleNamespace

    from online_lang_splatting_amd import render
    from parity_common import make_scene
    from test_gpu_api import _Model, _view
    dev = torch.device(DEV)
    sc = make_scene(3000, 160, 120, 15, seed=5, max_sh_degree=1, sh_degree=1)
    pkg = render(_view(sc, dev), _Model(sc, dev), SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False), sc.bg.to(dev))
    lang = pkg["language"].detach()
    assert tuple(lang.shape) == (15, 120, 160) and lang.is_contiguous() and math.isfinite(float(lang.abs().sum()))
    case = R.make_case(120, 160, 9, 3, 4)
    case["codes"] = lang.cpu().clone()
    q, hip_out = _check("rendered 160 x 120", case)
    again = q.relevancy(lang)
    assert torch.equal(again["relevancy"].cpu(), hip_out["relevancy"])


def test_validator_sentences(hip):
    """The opening checks' sentences, word for word, on the smallest inputs that reach them."""
    from online_lang_splatting_amd.lang_query import LanguageDecoder
    case = R.make_case(40, 48, 0, 3, 0)
    q = _query(case)
    with _raises_exactly("LanguageDecoder: a GPU device is required (there is no torch fallback)"):
        LanguageDecoder("cpu")
    with _raises_exactly("relevancy: codes must be a float32 tensor on the GPU"):
        q.relevancy(case["codes"])
    with _raises_exactly("similarities: codes must be a float32 tensor on the GPU"):
        q.similarities(case["codes"].to(DEV).double())
    with _raises_exactly("set_phrases: pos_embeds must be a float32 tensor on the GPU"):
        q.set_phrases(case["pos"], case["neg"].to(DEV))
    with _raises_exactly("set_phrases: neg_embeds has shape (2, 31), expected [n,768] with n >= 1"):
        q.set_phrases(case["pos"].to(DEV), torch.rand(2, 31, device=DEV))
    with _raises_exactly("set_labels: label_embeds must be a float32 tensor on the GPU"):
        q.set_labels(torch.zeros(2, 768, device=DEV).double())
    assert q.counts == (3, 0, 4)
