"""The scenes of tests/fwd_batch_scenes.py really are what tests/test_gpu_fwd_batches.py needs them to be (CPU oracle only).

Every case: the list of tile (0, 0) has the constructed length and order.
stop, edge: a quadrant's stop position is the largest n_contrib over its pixels inside the image - the 0-based list position of
    the wall at which its last pixel terminated (asserted on the oracle's record: that pixel blended the entry before and
    not this one, and walls were left over).  Over the case list these positions cover, for both tile sizes and each of
    the four quadrants (= the forward's four waves), 126, 127, 128 and 129, both parities below 16, both halves of a pair,
    and 254 - 257 for at least one quadrant.  No constant of the issue had to move for that: 48 walls of sigma 12 px give
    s + {4, 9, 9, 10} (15 x 15 tiles) and s + {4, 10, 10, 11} (16 x 16), at every s.
never: every pixel of quadrant 0 stopped at a wall.  The test for "stopped" is n_contrib < s + n_walls: a pixel that had
    consumed all the walls would have n_contrib >= s + n_walls, since every wall reaches every pixel of that quadrant with
    alpha >= 1/255 (asserted on the record).  Its final_T obeys T (1 - alpha) < 1e-4 for the terminating wall's alpha: below
    1e-4 / 0.25 where alpha <= 0.75, and below 1e-4 / (1 - 0.99) at the pixels near the walls' centre where alpha sits at the
    0.99 cap (the corner pixel ends at T = 0.01: one wall blended, the second terminates it).  Both are asserted, the first on
    the quadrant's far corner.  The far corner of quadrant 3 blends the last entry of the list.
after: quadrant 0's last pixels, (7, 7) among them, terminate at the last wall, list position s + 4; the entries behind it are
    blended by no pixel of quadrant 0, and the other quadrants hold pixels that five walls do not stop; with one wall less pixel (7, 7) blends every one of
    them.  Both halves of a pair and both sides of the first batch boundary occur as the stop entry.
skips: the entries of opacity 0.003 are in the list and no pixel blends them; every other entry is blended by some pixel.
"""
import pytest
import torch

import bwd_batch_scenes as bs
import fwd_batch_scenes as fs
from parity_common import fwd_args


def _record(oracle, case, tile, F=3):
    sc, kind = fs.make(case, tile, F)
    oracle.TILE = tile
    oracle.lib().oracle_set_record(1)
    try:
        r = oracle.rasterize_language_gaussians(*fwd_args(sc))
    finally:
        oracle.lib().oracle_set_record(0)
    geom = r[4]
    W, H = sc.camera.width, sc.camera.height
    out = dict(sc=sc, kind=kind, W=W, H=H, nc=oracle.get_field(geom, "n_contrib").view(H, W),
               fT=oracle.get_field(geom, "final_T").view(H, W), ranges=oracle.get_field(geom, "ranges").view(-1, 2),
               pl=oracle.get_field(geom, "point_list"), cm=oracle.get_field(geom, "contrib_mask").view(-1, 8))
    oracle.release(geom)
    return out


@pytest.fixture(scope="module")
def records(oracle):
    return {tile: [(c, _record(oracle, c, tile)) for c in fs.cases(tile)] for tile in fs.TILES}


def _bit(cm, pos, rank):
    return (int(cm[pos, rank >> 5]) >> (rank & 31)) & 1


def _quadrant_pixels(q, tile, W, H):
    ys = range(8, min(tile, H)) if q >> 1 else range(0, min(8, H))
    xs = range(8, min(tile, W)) if q & 1 else range(0, min(8, W))
    return [(y, x) for y in ys for x in xs]


def _stops(case, rec, tile):
    """per quadrant: the stop position, or None for a quadrant without a pixel inside the image"""
    r0 = int(rec["ranges"][0, 0])
    first_wall, end_walls = case.s, case.s + case.n_walls
    out = []
    for q in range(4):
        pix = _quadrant_pixels(q, tile, rec["W"], rec["H"])
        if not pix:
            out.append(None)
            continue
        assert all(fs.quadrant_of_rank(y * tile + x, tile) == q for y, x in pix)
        ncs = [int(rec["nc"][y, x]) for y, x in pix]
        # every pixel terminated at a wall, with walls to spare
        assert all(first_wall <= n < end_walls for n in ncs), (case.name, q, min(ncs), max(ncs))
        stop = max(ncs)
        y, x = pix[ncs.index(stop)]
        rank = y * tile + x
        assert rec["kind"][stop] == fs.WALL
        assert _bit(rec["cm"], r0 + stop - 1, rank) == 1 and _bit(rec["cm"], r0 + stop, rank) == 0, (case.name, q, stop)
        out.append(stop)
    return out


@pytest.mark.parametrize("tile", fs.TILES)
def test_lists_have_the_constructed_length_and_order(records, tile):
    for case, rec in records[tile]:
        if case.family == "plain":
            N, lower, _ = case.plain
            L = len(bs.layout(N, lower))
        else:
            L = len(rec["kind"])
            assert L == (case.N if case.family == "skips" else case.s + case.n_walls + case.tail)
        assert rec["sc"].P == L
        r0, r1 = int(rec["ranges"][0, 0]), int(rec["ranges"][0, 1])
        assert r1 - r0 == L, case.name
        assert rec["pl"][r0:r1].tolist() == list(range(L)), case.name   # Gaussian i is list position i


def test_stop_positions_cover_the_batch_and_pair_boundaries(records):
    table = {}
    for tile in fs.TILES:
        seen = [set() for _ in range(4)]
        for case, rec in records[tile]:
            if case.family not in ("stop", "edge"):
                continue
            stops = _stops(case, rec, tile)
            if case.family == "edge":
                w, h = case.wh
                assert [s is None for s in stops] == [False, w <= 8, h <= 8, w <= 8 or h <= 8], (case.name, stops)
            for q, s in enumerate(stops):
                if s is not None:
                    seen[q].add(s)
        table[tile] = seen
        for q in range(4):
            assert {126, 127, 128, 129} <= seen[q], (tile, q, sorted(seen[q]))
            low = {s for s in seen[q] if s < 16}
            assert {s & 1 for s in low} == {0, 1}, (tile, q, sorted(low))
            # a wave's stop entry is the first half of a pair (even position: batches start at even positions) and the second
            assert {s & 1 for s in seen[q] if s >= 16} == {0, 1}
        assert any({254, 255, 256, 257} <= seen[q] for q in range(4)), (tile, [sorted(s) for s in seen])
    print({t: [sorted(s) for s in v] for t, v in table.items()})


@pytest.mark.parametrize("tile", fs.TILES)
def test_stop_offsets_do_not_depend_on_the_entries_in_front(records, tile):
    """faint entries in front of the walls move every quadrant's stop by their number and nothing else"""
    offs = {tuple(s - case.s for s in _stops(case, rec, tile)) for case, rec in records[tile] if case.family == "stop"}
    assert len(offs) == 1, offs
    off = offs.pop()
    assert off[0] < off[1] and off[0] < off[2] and off[1] < off[3] and off[2] < off[3], off   # the waves leave at different walls


@pytest.mark.parametrize("tile", fs.TILES)
def test_never_family(records, tile):
    (case, rec), = [(c, r) for c, r in records[tile] if c.family == "never"]
    r0 = int(rec["ranges"][0, 0])
    L = len(rec["kind"])
    assert L >= 2 * 128 + 1          # at least three batches
    end_walls = case.s + case.n_walls
    cap = 1.0 - float(torch.tensor(0.99, dtype=torch.float32))
    for y, x in _quadrant_pixels(0, tile, rec["W"], rec["H"]):
        rank = y * tile + x
        assert all(_bit(rec["cm"], r0 + p, rank) for p in range(case.s, int(rec["nc"][y, x])))   # every wall in front blended
        assert case.s < int(rec["nc"][y, x]) < end_walls, (y, x)                                  # it stopped at a wall
        assert float(rec["fT"][y, x]) < 1e-4 / cap * (1 + 1e-6)
    assert float(rec["fT"][7, 7]) < 1e-4 / 0.25
    assert int(rec["nc"][:8, :8].max()) < 128                                                     # inside the first batch
    # the last entry of the list that any pixel blends is blended by a pixel of quadrant 3, which therefore walked to it
    blending = [p for p in range(L) if int((rec["cm"][r0 + p] != 0).sum())]
    last = blending[-1]
    assert last == L - 1
    q3 = [int(rec["nc"][y, x]) for y, x in _quadrant_pixels(3, tile, rec["W"], rec["H"])]
    assert max(q3) == last + 1
    # ... while the other waves have left: quadrants 0 - 2 blend nothing behind the walls
    for q in range(3):
        assert max(int(rec["nc"][y, x]) for y, x in _quadrant_pixels(q, tile, rec["W"], rec["H"])) <= end_walls


@pytest.mark.parametrize("tile", fs.TILES)
def test_after_family(oracle, records, tile):
    stops = set()
    px, py = fs.AFTER_PIXEL
    rank = py * tile + px
    assert fs.quadrant_of_rank(rank, tile) == 0
    for case, rec in records[tile]:
        if case.family != "after":
            continue
        r0 = int(rec["ranges"][0, 0])
        last_wall = case.s + case.n_walls - 1
        q0 = rec["nc"][:8, :8]
        assert int(q0.max()) == last_wall == int(rec["nc"][py, px])            # the wave's stop entry is the last wall
        assert int(q0.min()) >= case.s
        assert int(rec["nc"][:tile, :tile].max()) == case.s + case.n_walls             # the other waves never stop
        assert _bit(rec["cm"], r0 + last_wall - 1, rank) == 1 and _bit(rec["cm"], r0 + last_wall, rank) == 0
        for p in range(last_wall + 1, len(rec["kind"])):
            ranks = [r for r in range(tile * tile) if _bit(rec["cm"], r0 + p, r)]
            assert all(fs.quadrant_of_rank(r, tile) != 0 for r in ranks), (case.name, p)
        # one wall less: the pixel is still live behind the walls and blends every entry of the tail
        fewer = _record(oracle, case._replace(n_walls=case.n_walls - 1), tile)
        f0 = int(fewer["ranges"][0, 0])
        assert all(_bit(fewer["cm"], f0 + p, rank) for p in range(last_wall, len(fewer["kind"])))
        stops.add(last_wall)
    assert {s & 1 for s in stops} == {0, 1} and {126, 127, 128} <= stops, stops


@pytest.mark.parametrize("tile", fs.TILES)
def test_skipped_entries_blend_nowhere_and_their_neighbours_do(records, tile):
    parities, seen127, seen128, odd_last, longest_run = set(), False, False, False, 0
    for case, rec in records[tile]:
        if case.family != "skips":
            continue
        r0 = int(rec["ranges"][0, 0])
        nonzero = (rec["cm"][r0:r0 + case.N] != 0).any(dim=1)
        for p, k in enumerate(rec["kind"]):
            assert bool(nonzero[p]) == (k == fs.FAINT), (case.name, p)
        for p in case.skips:
            partner = p ^ 1
            if partner < case.N and rec["kind"][partner] == fs.FAINT:
                parities.add(p & 1)
        seen127 |= 127 in case.skips
        seen128 |= 128 in case.skips
        odd_last |= case.N % 2 == 1 and (case.N - 1) in case.skips
        run = best = 0
        for k in rec["kind"]:
            run = run + 1 if k == fs.SKIP else 0
            best = max(best, run)
        longest_run = max(longest_run, best)
    assert parities == {0, 1} and seen127 and seen128 and odd_last and longest_run > 128


def test_expected_flags_on_a_hand_made_record():
    """expected_flags / expected_tile_work / expected_blended on masks set by hand"""
    def mask(ranks):
        m = torch.zeros(8, dtype=torch.int64)
        for r in ranks:
            m[r >> 5] |= 1 << (r & 31)
        return torch.where(m >= 2 ** 31, m - 2 ** 32, m).to(torch.int32)

    # rank = row * tile + column.  15: rank 0 -> quadrant 0, survivor of packed wave 0; rank 8 -> quadrant 1, 8 % 7 == 1: survivor;
    # rank 2 -> quadrant 0, 2 % 7 == 2: no survivor; rank 8 * 15 = 120 -> quadrant 2, 120 % 7 == 1, >= 112: packed wave 1;
    # rank 224 -> row 14, column 14: quadrant 3, not below 224: no survivor
    cm = torch.stack([mask([]), mask([0]), mask([8]), mask([2]), mask([120]), mask([224]), mask([0, 8, 120, 224])])
    assert fs.expected_flags(cm, 15).tolist() == [0, 1 | 16, 2 | 16, 1, 4 | 32, 8, 15 | 48]
    # 16: rank 8 -> quadrant 1; rank 128 -> row 8: quadrant 2; rank 255 -> quadrant 3; no packed waves
    cm16 = torch.stack([mask([0]), mask([8]), mask([128]), mask([255]), mask([7, 136])])
    assert fs.expected_flags(cm16, 16).tolist() == [1, 2, 4, 8, 1 | 8]
    fl = fs.expected_flags(cm, 15)
    tw = fs.expected_tile_work(fl, torch.tensor([[0, 3], [3, 3], [3, 7]]))
    assert tw.tolist() == [[2, 0, 7], [2, 0, 3]]
    assert fs.expected_blended(fl, torch.tensor([0, 1, 2, 2, 3, 4, 1]), 6).tolist() == [0, 1, 1, 1, 1, 0]
