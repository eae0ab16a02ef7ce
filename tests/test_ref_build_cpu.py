"""The oracle against the reference's own kernel source.  No GPU needed.

Every parity test of this project compares the HIP kernels with oracle/oracle.cpp, a restatement of the reference
rasteriser written by hand.  Here that restatement is held to the thing it restates: the reference's forward.cu,
backward.cu and rasterizer_impl.cu, compiled unmodified as host C++ over an execution model of our own (oracle/ref_shim/,
oracle/ref_build.py) and driven through the reference's own Rasterizer / LanguageRasterizer entry points
(oracle/oracle_ref.py).  Blocks run in ascending tile order, which is the order the oracle's ordered accumulation
follows, so every comparison below except one is an equality on bits (parity_common.same_bits):

  * reference build vs liboracle.so: num_rendered, radii, n_touched, the per-Gaussian state, keys, point_list, ranges,
    n_contrib, final_T and the opacity image;
  * reference build vs liboracle_plain.so (the oracle with the forward's three accumulations as a multiply and an add,
    which is what a contraction-off build of the reference performs): all of that and the colour, language and depth images;
  * liboracle.so (fmaf accumulations, the project's model of nvcc's contraction) vs the reference build on those three
    images: |delta| <= 2 (n_contrib + 1) 2^-24 max|f| per pixel and channel, max|f| over that channel's features.  Both
    sides add the same terms f alpha T, sum of alpha T <= 1, and differ by one rounding per term;
  * the whole backward on sc.cotangents(seed), the oracle in BWD_REFERENCE mode: the six composite-level tensors and
    every per-Gaussian output;
  * backward_chain of both sides on the same random composite-level gradients: every CHAIN_KEYS tensor.

The scenes and the conditions each must meet (asserted on the oracle's output before anything is compared) are in
tests/ref_scenes.py.  Out of scope: the planted non-finite scenes (the reference converts NaN to int there, which C++
leaves undefined) and the needle scenes.
"""
import pytest
import torch

import ref_scenes as S
from parity_common import COMPOSITE_KEYS, first_difference

from oracle import oracle_ref

pytestmark = pytest.mark.skipif(not oracle_ref.available(),
                                reason="oracle/_ref holds no reference build and the reference tree is absent")

NAMES = tuple(S.SCENES)
PER_GAUSSIAN_KEYS = ("dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations", "dL_dtau")


def _eq(a, b, what):
    assert a.shape == b.shape or a.numel() == b.numel(), f"{what}: shapes {tuple(a.shape)} vs {tuple(b.shape)}"
    if a.dtype in (torch.int64, torch.int32, torch.uint8, torch.bool):
        same = bool((a.reshape(-1).long() == b.reshape(-1).long()).all())
        assert same, f"{what}: {int((a.reshape(-1).long() != b.reshape(-1).long()).sum())} of {a.numel()} integers differ"
        return
    d = first_difference(a, b)
    assert d is None, f"{what}: {d[3]} of {a.numel()} elements differ, first at {d[0]}: {d[1]!r} vs {d[2]!r}"


def _forward_state_equal(fr, fo, where):
    assert fr["R"] == fo["R"], f"{where}: num_rendered {fr['R']} vs {fo['R']}"
    for k in ("radii", "n_touched", "opacity"):
        _eq(fr[k], fo[k], f"{where}: {k}")
    for k in S.STATE_FIELDS:
        _eq(fr["state"][k], fo["state"][k], f"{where}: {k}")


@pytest.fixture(scope="module", params=NAMES)
def scene(request):
    """The scene's name, once its conditions hold on the oracle's own output (the measured values go to -s output)."""
    m = S.conditions(request.param)
    print(f"\n{request.param}: {m}")
    return request.param


def test_forward_state_equals_oracle(scene):
    fr, _ = S.ref_run(scene)
    fo, _ = S.oracle_run(scene)
    _forward_state_equal(fr, fo, f"{scene}: reference build vs oracle")


def test_forward_equals_plain_oracle(scene):
    fr, _ = S.ref_run(scene)
    fp, _ = S.oracle_run(scene, "plain_accum")
    assert S.oracle_module("plain_accum").lib().oracle_variant() == b"plain_accum"
    _forward_state_equal(fr, fp, f"{scene}: reference build vs plain-accumulation oracle")
    for k in ("color", "language", "depth"):
        if fr[k] is not None:
            _eq(fr[k], fp[k], f"{scene}: reference build vs plain-accumulation oracle: {k} image")


def test_forward_images_within_derived_bound(scene):
    fr, _ = S.ref_run(scene)
    fo, _ = S.oracle_run(scene)
    for k in ("color", "language", "depth"):
        if fr[k] is None or fr[k].numel() == 0:
            continue
        bound = S.image_bound(scene, fo, k)
        err = (fo[k].double() - fr[k].double()).abs()
        worst = (err - bound).max().item()
        print(f"{scene}: {k}: max |oracle - reference build| {err.max().item():.3e}, smallest margin to the bound {-worst:.3e}")
        assert bool((err <= bound).all()), (f"{scene}: {k}: {int((err > bound).sum())} values outside "
                                            f"2 (n_contrib + 1) 2^-24 max|f|, worst excess {worst:.3e}")


def test_backward_equals_oracle(scene):
    _, gr = S.ref_run(scene)
    _, go = S.oracle_run(scene)
    for k in COMPOSITE_KEYS + PER_GAUSSIAN_KEYS:
        _eq(gr[k], go[k], f"{scene}: backward: {k}")


def test_backward_chain_equals_oracle(scene):
    """computeCov2DCUDA and the backward preprocessCUDA themselves against the oracle's chain, on gradients neither made."""
    fr, _ = S.ref_run(scene)
    fo, _ = S.oracle_run(scene)
    sp = S.spec(scene)
    P, F = sp.scene.P, max(sp.scene.F, 0)
    g = torch.Generator().manual_seed(4242)
    comp = dict(dL_dmeans2D=torch.randn(P, 3, generator=g) * 1e-3, dL_dconic=torch.randn(P, 2, 2, generator=g) * 1e-2,
                dL_dcolors=torch.randn(P, 3, generator=g) * 1e-3, dL_ddepths=torch.randn(P, 1, generator=g) * 1e-3)
    O = S.oracle_module("default")
    O.TILE = oracle_ref.TILE = sp.tile
    want = O.backward_chain(F, comp, *fo["bwd_args"])
    got = oracle_ref.backward_chain(F, comp, *fr["bwd_args"])
    for k in O.CHAIN_KEYS:
        _eq(got[k], want[k], f"{scene}: chain: {k}")
    if scene != "all_culled":
        assert any(bool((want[k] != 0).any()) for k in O.CHAIN_KEYS), f"{scene}: the chain produced only zeros"


def test_mark_visible_equals_oracle():
    from oracle import oracle_C
    sc = S.spec("ragged").scene
    cam = sc.camera
    a = (sc.means3D, cam.world_view_transform, cam.full_proj_transform)
    assert torch.equal(oracle_ref.mark_visible(*a), oracle_C.mark_visible(*a))
    assert 0 < int(oracle_C.mark_visible(*a).sum()) < sc.P


def test_every_build_was_used():
    """Each of the four builds has run at least one scene above (tile 15 with 15, 3 and 16 channels, tile 16 with 15)."""
    from oracle import ref_build
    used = {(S.spec(n).tile, S.spec(n).scene.F or 15) for n in NAMES}
    assert set(ref_build.BUILDS) <= used, (ref_build.BUILDS, used)
