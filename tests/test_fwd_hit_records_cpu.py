"""The scenes of tests/fwd_hit_scenes.py really produce the conditions tests/test_gpu_fwd_hit_records.py needs (CPU oracle
only, on the oracle's record of which pixel blended which list entry).

Every case: the list of tile (0, 0) has the constructed length (at most 300) and order, the image is 2 x 2 tiles.
plan cases: a ONE w entry is blended by pixels of quadrant w only (and by one at least), an ALL entry by a pixel of every
    quadrant, a NONE entry by no pixel - while it IS in the list.  Over the cases every position of POSITIONS is blended by
    every wave alone, by all four and by none; in the stale cases what wave w blends at position p of batch 0 it does not blend
    at position p of batch 1 (and the reverse).
stop cases: the named quadrant's last pixel terminates at the named position (the largest n_contrib over its pixels; that
    pixel blended the entry before it and not this one).  Every position of POSITIONS occurs for quadrants 0 and 3.
Odd tails: every list has an odd length, so its last pair has the sentinel for a partner.
"""
import pytest

import fwd_batch_scenes as fs
import fwd_hit_scenes as hs
from parity_common import run_forward


def _record(oracle, case, tile, F):
    sc = hs.make(case, tile, F)
    oracle.lib().oracle_set_record(1)
    try:
        fo, _ = run_forward(oracle, sc, None, tile)
    finally:
        oracle.lib().oracle_set_record(0)
    geom = fo["geom"]
    W, H = sc.camera.width, sc.camera.height
    out = dict(sc=sc, W=W, H=H, nc=oracle.get_field(geom, "n_contrib").view(H, W),
               ranges=oracle.get_field(geom, "ranges").view(-1, 2), pl=oracle.get_field(geom, "point_list"),
               cm=oracle.get_field(geom, "contrib_mask").view(-1, 8))
    oracle.release(geom)
    return out


@pytest.fixture(scope="module")
def records(oracle):
    return {(tile, F): [(c, _record(oracle, c, tile, F)) for c in hs.cases(tile)] for tile in hs.TILES for F in (0, 15)}


def _waves(rec, tile, pos):
    """the set of quadrants (forward waves) with a pixel that blended list position `pos` of tile (0, 0)"""
    r0 = int(rec["ranges"][0, 0])
    out = set()
    for rank in range(tile * tile):
        if (int(rec["cm"][r0 + pos, rank >> 5]) >> (rank & 31)) & 1:
            out.add(fs.quadrant_of_rank(rank, tile))
    return out


def test_sizes_and_lists(records):
    for (tile, F), recs in records.items():
        for case, rec in recs:
            L = hs.list_length(case)
            assert L <= 300 and L % 2 == 1, case.name                       # odd batch tails
            assert (rec["W"], rec["H"]) == (2 * tile, 2 * tile) and rec["ranges"].shape[0] <= 6
            assert 30 <= rec["W"] <= 45 and rec["H"] <= 32
            r0, r1 = int(rec["ranges"][0, 0]), int(rec["ranges"][0, 1])
            assert r1 - r0 == L == rec["sc"].P, case.name
            assert rec["pl"][r0:r1].tolist() == list(range(L)), case.name   # Gaussian i is list position i (NONE entries too)


def test_planned_entries_are_blended_by_the_planned_waves(records):
    for (tile, F), recs in records.items():
        alone = {p: set() for p in hs.POSITIONS}
        by_all, by_none = set(), set()
        for case, rec in recs:
            for p, what in case.plan.items():
                got = _waves(rec, tile, p)
                want = {what[1]} if what[0] == "one" else ({0, 1, 2, 3} if what[0] == "all" else set())
                assert got == want, (tile, F, case.name, p, what, got)
                if p < hs.BATCH:
                    if what[0] == "one":
                        alone[p].add(what[1])
                    (by_all if what[0] == "all" else by_none if what[0] == "none" else set()).add(p)
        assert all(alone[p] == {0, 1, 2, 3} for p in hs.POSITIONS), alone
        assert by_all >= set(hs.POSITIONS) and by_none >= set(hs.POSITIONS)


def test_stale_cases_differ_between_the_batches(records):
    for (tile, F), recs in records.items():
        seen = set()
        for case, rec in recs:
            if not case.name.startswith("stale_"):
                continue
            for p in hs.POSITIONS:
                a, b = _waves(rec, tile, p), _waves(rec, tile, hs.BATCH + p)
                assert a != b, (case.name, p)
                seen.add((bool(a - b), bool(b - a)))     # a wave of batch 0 absent in batch 1 / the reverse
        assert seen >= {(True, False), (False, True), (True, True)}, seen


def test_stop_cases_saturate_the_named_wave_at_the_named_position(records):
    for (tile, F), recs in records.items():
        covered = {q: set() for q in hs.STOP_QUADRANTS}
        for case, rec in recs:
            if case.stop is None:
                continue
            q, p = case.stop
            r0 = int(rec["ranges"][0, 0])
            pix = [(y, x) for y in (range(8, tile) if q >> 1 else range(8)) for x in (range(8, tile) if q & 1 else range(8))]
            ncs = [int(rec["nc"][y, x]) for y, x in pix]
            first_wall, end_walls = case.base.s, case.base.s + case.base.n_walls
            assert all(first_wall <= n < end_walls for n in ncs), (case.name, min(ncs), max(ncs))   # every pixel stopped at a wall
            stop = max(ncs)
            assert stop == p, (tile, F, case.name, stop)
            y, x = pix[ncs.index(stop)]
            rank = y * tile + x
            bit = lambda pos: (int(rec["cm"][r0 + pos, rank >> 5]) >> (rank & 31)) & 1   # noqa: E731
            assert bit(stop - 1) == 1 and bit(stop) == 0, case.name
            assert q not in _waves(rec, tile, stop + 1)     # the wave blends nothing behind its stop entry
            covered[q].add(p)
        assert all(covered[q] == set(hs.POSITIONS) for q in hs.STOP_QUADRANTS), covered
