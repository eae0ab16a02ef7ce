"""The carried depth order's two repair launches (csrc/k_order_carry.hip) held to the host model tests/order_carry_ref.py
with EQUALITIES: the verdict carry_missed() is a pure function of (the array on entry, the frame's keys), so a kernel that
misses where the algorithm hits (a silent loss of the repair) and one that hits where it must miss (wrong lists) both fail.
The keys are driven directly: P Gaussians on the optical axis of the identity pose, so the view depth IS means3D[:, 2] and
every Gaussian emits into the centre of the image — the instance list is the depth order.  tests/order_carry_scenes.py is the
case table (one element moved by about half a window from every kind of rank, block reversals astride window and half-window
edges, blocks of ties), which tests/test_order_carry_ref_cpu.py shows to be two-sided by the model alone.

Per case, frame 0 leaves a known order; frame 1 (the case's permutation of the depths) must give the model's verdict, the plain
workspace's lists, images and gradients bit for bit, and leave THE sort of its keys behind whether it hit or missed; the next
frame on the same depths is a hit.  The all-ones cases plant the depth bit pattern 0xFFFFFFFF — the key of the repair's own
padding — and every frame of them must take the radix passes."""
import numpy as np
import pytest
import torch

import order_carry_ref as M
import order_carry_scenes as S
from online_lang_splatting_amd import _C, _abi
from online_lang_splatting_amd.scene import Scene, default_camera
from test_gpu_order_carry import _assert_identical, _cam, _frame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W_IMG, H_IMG = 64, 48
CAPACITY = 1 << 17   # (at most four instances per Gaussian: 40 000 at P = 10 000)
_WS = {}
_SCENE = {}


def _scene(P, F):
    """everything but the depths: sub-pixel jitter about the optical axis, tiny isotropic Gaussians, low opacity"""
    if (P, F) not in _SCENE:
        g = torch.Generator().manual_seed(77 + P)
        jit = (torch.rand(P, 2, generator=g) - 0.5) * 0.2 / (W_IMG / 2.0)   # +- 0.1 pixel at depth 1
        lang = torch.randn(P, F, generator=g) if F else None
        _SCENE[(P, F)] = Scene(default_camera(W_IMG, H_IMG, 0.0, 0.0), torch.zeros(P, 3), torch.full((P, 1), 0.02),
                               torch.full((P, 3), 1e-3), torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(P, 1).contiguous(),
                               (torch.rand(P, 1, 3, generator=g) * 3.0 - 1.5).contiguous(),
                               (lang / lang.norm(dim=1, keepdim=True)).contiguous() if F else None, 0, torch.zeros(3), F), jit
    return _SCENE[(P, F)]


def _workspaces(P, F, tile, flags, binning=_abi.BINNING_ELLIPSE):
    """one plain and one carrying workspace per launch shape, shared by the cases (what the array holds never matters)"""
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    key = (P, F, tile, flags, binning)
    if key not in _WS:
        kw = dict(tile=tile, flags=flags, binning=binning)
        dev = torch.device(DEV)
        _WS[key] = (RasterWorkspace(P, W_IMG, H_IMG, F, 1, CAPACITY, dev, **kw),
                    RasterWorkspace(P, W_IMG, H_IMG, F, 1, CAPACITY, dev, carry_order=True, **kw))
    return _WS[key]


def _inputs(sc, jit, z, dev):
    """the scene's arrays on the device with depths z (float32 numpy, any bit pattern): x, y = jitter * z, NaN-free"""
    zt = torch.from_numpy(np.ascontiguousarray(z))
    zf = torch.where(zt.isnan(), torch.ones_like(zt), zt)
    means = torch.cat([jit * zf[:, None], zt[:, None]], dim=1).contiguous()
    assert np.array_equal(means[:, 2].numpy().view(np.uint32), z.view(np.uint32))   # (bit patterns survive the copy)
    sc.means3D = means
    return dict(bg=sc.bg.to(dev), means3D=means.to(dev), opacities=sc.opacities.to(dev), scales=sc.scales.to(dev),
                rotations=sc.rotations.to(dev), shs=sc.shs.to(dev), language=sc.language.to(dev) if sc.F else None)


def _geom(ws, name, dtype):
    return _C.state_field("geometry", ws.geom, name, P=ws.P, F=ws.F, dtype=dtype, count=ws.P).cpu().numpy().copy()


def _keys_on_device(ws):
    return _geom(ws, "sort_keys", torch.int32).view(np.uint32)


def _array(ws):
    return ws.depth_order_carry.cpu().numpy().view(np.uint32).copy()


@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_verdict_and_order_equal_the_model(hip, case):
    dev = torch.device(DEV)
    P = case.P
    sc, jit = _scene(P, case.F)
    plain, carry = _workspaces(P, case.F, case.tile, _abi.FLAG_FRAMES_IN_FLIGHT if case.in_flight else 0)
    cam = _cam(sc.camera, dev)
    cot = [t.to(dev) if t is not None else None for t in sc.cotangents(1)]
    z0, z1 = S.depths(case)

    _frame(carry, sc, cam, _inputs(sc, jit, z0, dev), cot)                         # frame 0 (hit or miss: whatever the array held)
    entry = _array(carry)
    assert np.array_equal(entry, M.sorted_order(M.keys_of_depths(z0)))

    g1 = _inputs(sc, jit, z1, dev)
    ref = _frame(plain, sc, cam, g1, cot)
    assert ref[3] >= P                                                              # every Gaussian emits: `depths` is complete
    got = _frame(carry, sc, cam, g1, cot)                                           # frame 1
    depths = _geom(carry, "depths", torch.float32)
    assert np.array_equal(depths.view(np.uint32), z1.view(np.uint32))              # the view depth is means3D[:, 2], bit for bit
    keys = M.keys_of_depths(depths)
    _order, want_miss, _ = M.repair(entry, keys)
    missed = carry.carry_missed()
    print(f"{case.id}: model {'miss' if want_miss else 'hit'}, kernels {'miss' if missed else 'hit'}")
    assert missed == want_miss                                                      # 1
    _assert_identical(got, ref)                                                     # 2
    assert np.array_equal(_array(carry), M.sorted_order(keys))                      # 3 (hit or miss)
    if not missed:
        assert np.array_equal(_keys_on_device(carry), keys)                         # 4
        inst = _geom(carry, "tiles_touched", torch.int32).view(np.uint32)
        totals = _C.state_field("geometry", carry.geom, "carry_totals", P=P, F=carry.F, dtype=torch.int64,
                                count=(P + 1023) // 1024).cpu().numpy().view(np.uint64)
        assert np.array_equal(totals, M.repair(entry, keys, inst)[2])               # (the totals the emission went by)

    again = _frame(carry, sc, cam, g1, cot)                                         # 5
    assert not carry.carry_missed()
    _assert_identical(again, ref)
    assert np.array_equal(_array(carry), M.sorted_order(keys))


# ---------------------------------------------------------------------------------------------------- the all-ones key
@pytest.fixture(scope="module")
def all_ones_key(hip):
    """What the device makes of a view depth with the bit pattern 0xFFFFFFFF: the sort key of such a Gaussian (at P <= 8192 a
    frame that misses leaves the keys in place: the one-launch sort reads them only), and whether it wrote `depths` for it."""
    dev = torch.device(DEV)
    P, g = 3000, 5
    sc, jit = _scene(P, 0)
    _plain, carry = _workspaces(P, 0, 15, 0)
    _frame(carry, sc, _cam(sc.camera, dev), _inputs(sc, jit, S.all_ones_depths(P, (g,)), dev),
           [t.to(dev) if t is not None else None for t in sc.cotangents(1)])
    key = int(_keys_on_device(carry)[g])
    depth_bits = int(_geom(carry, "depths", torch.float32).view(np.uint32)[g])
    radius = int(carry.out["radii"][g])
    print(f"all-ones depth bits: sort key {key:#010x}, depths[g] {depth_bits:#010x}, radius {radius} "
          f"({'payload kept' if key == 0xFFFFFFFF else 'NaN canonicalised'})")
    assert key & 0x7F800000 == 0x7F800000 and key & 0x007FFFFF   # a NaN either way
    return key


def _all_ones_keys(P, gs, z, key):
    keys = M.keys_of_depths(z)
    keys[list(gs)] = key
    return keys


@pytest.mark.parametrize("P,gs", S.ALL_ONES, ids=[f"P{P}-g{'_'.join(map(str, gs))}" for P, gs in S.ALL_ONES])
def test_a_depth_of_all_ones_always_takes_the_radix_passes(hip, all_ones_key, P, gs):
    """Two frames: the first from whatever the array held, the second from the order the first one's sort left — the frame
    on which the unguarded proof accepted an array with one Gaussian twice and another never."""
    dev = torch.device(DEV)
    F = 3 if len(gs) > 1 else 0
    sc, jit = _scene(P, F)
    plain, carry = _workspaces(P, F, 15, 0)
    cam = _cam(sc.camera, dev)
    cot = [t.to(dev) if t is not None else None for t in sc.cotangents(1)]
    z = S.all_ones_depths(P, gs)
    g_in = _inputs(sc, jit, z, dev)
    keys = _all_ones_keys(P, gs, z, all_ones_key)
    ref = _frame(plain, sc, cam, g_in, cot)
    assert ref[3] >= P - len(gs)
    for frame in range(2):
        entry = _array(carry)
        got = _frame(carry, sc, cam, g_in, cot)
        missed = carry.carry_missed()
        if P <= 8192:
            assert np.array_equal(_keys_on_device(carry), keys)
        assert missed == M.repair(entry, keys)[1], frame
        if all_ones_key == 0xFFFFFFFF:
            assert missed, frame
        _assert_identical(got, ref)
        assert np.array_equal(_array(carry), M.sorted_order(keys)), frame


def test_a_depth_of_all_ones_meets_the_oracle(hip, oracle, all_ones_key):
    """The instance list and the images of the second frame (the one that starts from a sorted array) against the oracle, with
    the reference's bounding-square binning."""
    from parity_common import run_forward
    dev = torch.device(DEV)
    P, gs, F = 3000, (5, 1500, 2500), 3
    sc, jit = _scene(P, F)
    _plain, carry = _workspaces(P, F, 15, 0, binning=_abi.BINNING_RECT)
    cam = _cam(sc.camera, dev)
    cot = [t.to(dev) if t is not None else None for t in sc.cotangents(1)]
    g_in = _inputs(sc, jit, S.all_ones_depths(P, gs), dev)
    _frame(carry, sc, cam, g_in, cot)
    out, _grads, pl, R = _frame(carry, sc, cam, g_in, cot)
    assert carry.carry_missed() == (all_ones_key == 0xFFFFFFFF)
    fo, _ = run_forward(oracle, sc, None, 15, 0)
    pl_ref = oracle.get_field(fo["geom"], "point_list")
    oracle.release(fo["geom"])
    assert R == fo["R"] and torch.equal(pl.cpu(), pl_ref)
    assert torch.equal(out["color"].cpu(), fo["color"]) and torch.equal(out["language"].cpu(), fo["language"])
    assert torch.equal(out["radii"].cpu(), fo["radii"]) and torch.equal(out["depth"].cpu(), fo["depth"])
    assert torch.equal(out["n_touched"].cpu(), fo["n_touched"])
