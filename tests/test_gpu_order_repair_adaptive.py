"""The carried-order repair (csrc/k_order_carry.hip) skips the merge levels a window does not need — all of them when the window
already ascends under the new keys, otherwise every level whose sibling runs are already in order.  A skipped level is the
identity, so phase A's windows, phase B's windows, phase B's proof, the totals, the carried array and `miss` must be exactly
what the full merges leave.

The expectation is restated here in torch and never taken from the code under test: stable-sort phase A's aligned 2 048-rank
windows of the carried array under the frame's keys, stable-sort phase B's half-shifted windows of that, apply the proof
(strict ascent inside a window; a window's last pair below the smaller head of the next window's two half-windows in phase
A's output; no index out of range) -> `miss`.  Hit or miss, the array must hold the full (key, index) order afterwards, and
the instance lists, the tile ranges and the forward images must equal those of a workspace that sorts from scratch.

Shapes: the smallest that can go wrong — one Gaussian, a ragged single window, exactly one window, one rank more, ragged
third window, three windows and one rank; 256- and 1 024-thread workgroups (their element-per-thread loops differ)."""
import pytest
import torch

from online_lang_splatting_amd import _C, _abi
from online_lang_splatting_amd.scene import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, H, TILE, F = 64, 48, 15, 3
OC_W = 2048
TILES = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)


def _expected_miss(carry, keys, P):
    """the two phases and the proof on the CPU: (miss, the array phase B leaves — None when an index is out of range)"""
    g = carry.cpu().long() & 0xFFFFFFFF
    if bool((g >= P).any()):
        return True, None                      # (phase A raises miss itself; what it sorts then is nobody's business)
    a = (keys[g] << 32) | g                    # keys < 2^31 (bits of a positive float): fits int64
    for s in range(0, P, OC_W):                # phase A
        a[s:s + OC_W] = a[s:s + OC_W].sort(stable=True).values
    b = a.clone()
    bad = False
    for j in range((P + OC_W // 2 + OC_W - 1) // OC_W):   # phase B
        s, e = max(j * OC_W - OC_W // 2, 0), min(j * OC_W + OC_W // 2, P)
        b[s:e] = a[s:e].sort(stable=True).values
        bad |= not bool((b[s + 1:e] > b[s:e - 1]).all())
        nxt = j * OC_W + OC_W // 2             # first rank of the next window
        if nxt < P:
            nmin = a[nxt] if nxt + OC_W // 2 >= P else torch.minimum(a[nxt], a[nxt + OC_W // 2])
            bad |= not bool(b[nxt - 1] < nmin)
    return bad, b & 0xFFFFFFFF


def _swap(o, i, j):
    o = o.clone()
    o[i], o[j] = o[j].clone(), o[i].clone()
    return o


def _move(o, src, dst):
    """the Gaussian at rank src stands at rank dst instead (the ranks between close up / make room)"""
    l = o.tolist()
    l.insert(dst, l.pop(src))
    return torch.tensor(l, dtype=o.dtype)


def _cases(order, P):
    """(name, carried array, expected miss if it can be said without the model or None)"""
    c = [("exact", order.clone(), False), ("zeros", torch.zeros_like(order), P > 1)]
    for r in (10, 701):                        # even and odd rank: the pair is a sibling pair at level 1 / at level 2
        if r + 1 < P:
            c.append((f"adjacent_swap_{r}", _swap(order, r, r + 1), False))
    for r in (1023, 2047, 4095):               # across phase B's / phase A's window edges
        if r + 1 < P:
            c.append((f"swap_{r}|{r + 1}", _swap(order, r, r + 1), False))
    for d in (1023, 1024, 1025):
        for s in (100, 1500):                  # forwards, inside phase A's window / across its edge
            if s + d < P:
                c.append((f"rank_{s}_carried_at_{s + d}", _move(order, s, s + d), None))
        if 2047 + d < P:                       # backwards, onto the last rank of phase A's first window: phase B's window
            c.append((f"rank_{2047 + d}_carried_at_2047", _move(order, 2047 + d, 2047), d > 1024))   # reaches rank 3071
        if 2048 < P:                           # forwards, onto the first rank of phase A's second window: phase B's window
            c.append((f"rank_{2048 - d}_carried_at_2048", _move(order, 2048 - d, 2048), d > 1024))   # reaches down to rank 1024
        if 1023 + d < P:
            c.append((f"rank_{1023 + d}_carried_at_1023", _move(order, 1023 + d, 1023), None))
    for pos in (1, 1024, 2048):
        if pos < P:
            dup = order.clone()
            dup[pos] = dup[pos - 1]
            c.append((f"duplicate_at_{pos}", dup, True))
    for pos, v in ((0, P), (P - 1, -1), (P // 2, 2**31 - 1)):
        oor = order.clone()
        oor[pos] = v
        c.append((f"out_of_range_{v}_at_{pos}", oor, True))
    return c


def _frame(ws):
    out = {k: v.clone() for k, v in ws.forward().items()}
    R, overflow = ws.rendered()
    assert not overflow
    pl = _C.state_field("binning", ws.binning, "point_list", R=ws.capacity, F=ws.F, dtype=torch.int32, count=R).clone()
    ranges = _C.state_field("image", ws.img, "ranges", W=W, H=H, dtype=torch.int32, count=2 * TILES).clone()
    return out, R, pl, ranges


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("P", [1, 1500, 2048, 2049, 5000, 6145])
def test_adaptive_repair_leaves_what_the_full_merges_leave(hip, P, threads):
    from online_lang_splatting_amd.frame_shard import RasterWorkspace
    dev = torch.device(DEV)
    # (the repair's workgroup shape follows the scene flag: four waves beside other frames in flight, sixteen alone)
    flags = _abi.FLAG_FRAMES_IN_FLIGHT if threads == 256 else 0
    sc = make_scene(P, W, H, F, seed=700 + P % 89)
    if P > 3:
        sc.means3D[::3, 2] = sc.means3D[0, 2]   # equal depths in quantity: ties go by index
    c = sc.camera
    args = dict(bg=sc.bg.to(dev), means3D=sc.means3D.to(dev), opacities=sc.opacities.to(dev), scales=sc.scales.to(dev),
                rotations=sc.rotations.to(dev), shs=sc.shs.to(dev), language=sc.language.to(dev),
                viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev),
                projmatrix_raw=c.projection_matrix.to(dev), campos=c.camera_center.to(dev), tanfovx=c.tanfovx,
                tanfovy=c.tanfovy, sh_degree=sc.sh_degree)
    kw = dict(tile=TILE, flags=flags)
    plain = RasterWorkspace(P, W, H, F, sc.shs.shape[1], 400_000, dev, **kw)
    carry = RasterWorkspace(P, W, H, F, sc.shs.shape[1], 400_000, dev, carry_order=True, **kw)
    plain.set_scene(**args)
    carry.set_scene(**args)
    ref_out, ref_R, ref_pl, ref_ranges = _frame(plain)   # the full radix order's lists: computed once, compared with every case

    # the frame's keys: what the preprocess wrote, readable after a frame whose order came from a repair
    _frame(carry)
    assert carry.carry_missed() == (P > 1)
    _frame(carry)
    assert not carry.carry_missed()
    keys = (_C.state_field("geometry", carry.geom, "sort_keys", P=P, F=F, dtype=torch.int32, count=P).cpu().long()
            & 0xFFFFFFFF)
    assert bool((keys > 0).all()) and bool((keys < 2**31).all())
    order = ((keys << 32) | torch.arange(P)).sort().indices.to(torch.int32)
    assert torch.equal(carry.depth_order_carry.cpu(), order)
    if P > 3:
        assert bool((keys[order.long()][1:] == keys[order.long()][:-1]).any())   # ties are present

    verdicts = {}
    for name, arr, known in _cases(order, P):
        miss, left = _expected_miss(arr, keys, P)
        if known is not None:
            assert miss == known, (name, "the test's own model disagrees with the hand-derived verdict")
        if not miss:
            assert torch.equal(left.to(torch.int32), order), (name, "model: a proven repair is the order")
        carry.depth_order_carry.copy_(arr.to(torch.int32))
        out, R, pl, ranges = _frame(carry)
        assert carry.carry_missed() == miss, (name, P, threads)
        assert torch.equal(carry.depth_order_carry.cpu(), order), (name, "carried array after the frame")
        assert R == ref_R, name
        assert torch.equal(pl, ref_pl), (name, "instance lists")
        assert torch.equal(ranges, ref_ranges), (name, "tile ranges")
        for k in ref_out:
            assert torch.equal(out[k], ref_out[k]), (name, k)
        verdicts[name] = miss
    print(f"P={P} threads={threads}: " + " ".join(f"{n}={'miss' if m else 'hit'}" for n, m in verdicts.items()))
