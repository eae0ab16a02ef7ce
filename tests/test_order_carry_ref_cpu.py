"""The host model of the carried depth order's repair (tests/order_carry_ref.py) on its own, without a GPU:
  soundness     miss == False implies that the array left behind is THE sort, whatever the array and the keys were — the
                all-ones key (the repair's high padding) included, which is what the model's guard is for;
  completeness  an array in which nothing stands more than half a window (1024 ranks) from its place is a hit;
  the table     tests/order_carry_scenes.py, which the GPU test holds the kernels to, has hits AND misses in quantity by the
                model alone, and the model gives the verdicts at the window edges that the algorithm implies."""
import numpy as np
import pytest

import order_carry_ref as M
import order_carry_scenes as S

SIZES = (1, 63, 2047, 2048, 2049, 3000, 4096, 5000, 10000)
SPECIAL = (1, 0x7F800000, 0x7FC00000, 0xFFC00000, 0xFFFFFFFE, 0xFFFFFFFF)


def _keys(rng, P, kind):
    """depth-like keys (distinct in the main, some ties), with the special values planted"""
    keys = rng.integers(0x3E000000, 0x41000000, P, dtype=np.int64).astype(np.uint32)
    if P > 3:
        keys[::3] = keys[0]
    where = dict(none=(), low=(lambda g: g < 1024), mid=(lambda g: (g >= 1024) & (g < 2048)), high=(lambda g: g >= 2048))
    g = np.arange(P)
    if kind == "specials":
        for i, v in enumerate(SPECIAL):
            keys[rng.integers(0, P, 1 + i % 2)] = v
    elif kind.startswith("ones_"):
        _, band, count = kind.split("_")
        cand = g[where[band](g)]
        if cand.size:
            keys[rng.choice(cand, min(cand.size, 1 if count == "one" else 3), replace=False)] = 0xFFFFFFFF
    return keys


KEY_KINDS = ("plain", "specials") + tuple(f"ones_{b}_{c}" for b in ("low", "mid", "high") for c in ("one", "several"))


def _arrays(rng, P, keys):
    """arrays on entry: the order itself, nearly the order, random permutations, duplicates, out of range, reversed"""
    order = M.sorted_order(keys)
    yield "sorted", order
    yield "reversed", order[::-1].copy()
    yield "random", rng.permutation(P).astype(np.uint32)
    yield "duplicates", rng.integers(0, max(P // 2, 1), P).astype(np.uint32)
    yield "out_of_range", rng.integers(0, 2 ** 32, P, dtype=np.int64).astype(np.uint32)
    near = order.copy()
    for _ in range(4):   # a few short moves: what a hit looks like
        i = int(rng.integers(0, P))
        j = min(P, i + int(rng.integers(1, 700)))
        near[i:j] = np.roll(near[i:j], 1)
    yield "near", near
    dup = order.copy()
    if P > 1:
        dup[P // 2] = dup[P // 2 - 1]   # in order, but one index twice and one never
    yield "one_duplicate", dup
    zeros = np.zeros(P, dtype=np.uint32)
    yield "zeros", zeros


@pytest.mark.parametrize("P", SIZES)
def test_a_hit_is_always_the_sort(P):
    rng = np.random.default_rng(P)
    hits = 0
    for kind in KEY_KINDS:
        keys = _keys(rng, P, kind)
        want = M.sorted_order(keys)
        for name, carry in _arrays(rng, P, keys):
            order, miss, _ = M.repair(carry, keys)
            if not miss:
                hits += 1
                assert np.array_equal(order, want), (P, kind, name)
            if (keys == 0xFFFFFFFF).any():
                assert miss, (P, kind, name)   # (the guard: such a frame always takes the radix passes)
    assert hits >= 2   # (the test is not vacuous: the order itself and its neighbour are hits on ordinary keys)


def test_the_all_ones_key_behind_the_pads():
    """The inputs on which the proof WITHOUT the guard accepts an array that is no permutation (P = 3000, 4096, 5000, the order
    itself on entry, key 0xFFFFFFFF on Gaussian 2500 — a real pair that sorts behind the pads of its window): a miss.  The
    same Gaussian with the NaN key 0xFFC00000 is an ordinary hit."""
    for P in (3000, 4096, 5000):
        keys = (0x3F800000 + np.random.default_rng(7).permutation(P)).astype(np.uint32)
        keys[2500] = 0xFFFFFFFF
        assert M.repair(M.sorted_order(keys), keys)[1] is True
        keys[2500] = 0xFFC00000
        order, miss, _ = M.repair(M.sorted_order(keys), keys)
        assert miss is False and np.array_equal(order, M.sorted_order(keys))


def _single_move(P, s, d, forward):
    """an order (identity keys) in which one element stands d ranks from its place"""
    c = S.Case("move_fwd" if forward else "move_bwd", P, s, d)
    keys = S.new_rank(c).astype(np.uint32) + 1   # element r (= index r, at rank r on entry) belongs at new_rank[r]
    return np.arange(P, dtype=np.uint32), keys


@pytest.mark.parametrize("P", S.SIZES)
def test_within_half_a_window_is_a_hit(P):
    rng = np.random.default_rng(P)

    def hit(carry, keys, what):
        order, miss, _ = M.repair(carry, keys)
        assert not miss, what
        assert np.array_equal(order, M.sorted_order(keys)), what
    for d in (1, 2, 511, 1023, 1024):
        for s in S.starts(P, d):
            for fwd in (True, False):
                hit(*_single_move(P, s, d, fwd), (s, d, fwd))
    ident = np.arange(P, dtype=np.uint32)
    for L in (2, 1024, 1025):
        for s in (0, 1, 1023, 1024, 1536, 2047, 2048, 3000, P - L):
            keys = ident + 1
            keys[s:s + L] = keys[s:s + L][::-1].copy()
            hit(ident, keys, ("reversal", s, L))
    for bound in (1, 100, 1024):   # random permutations with bounded displacement: shuffle inside disjoint blocks of <= bound + 1
        for _ in range(3):
            keys, i = ident + 1, int(rng.integers(0, bound + 1))
            while i < P:
                n = min(int(rng.integers(1, bound + 2)), P - i)
                keys[i:i + n] = rng.permutation(keys[i:i + n])
                i += n
            hit(ident, keys, ("bounded", bound))


def test_the_verdict_at_the_window_edges():
    """Where a move of MORE than half a window starts decides the verdict: the element is carried by phase A to the end (the
    start) of its aligned window and by phase B at most half a window further."""
    P = 7000
    miss = lambda s, d, fwd: M.repair(*_single_move(P, s, d, fwd))[1]  # noqa: E731
    assert miss(2047, 1025, True) and not miss(2048, 1025, True)
    assert miss(1023, 1025, False)                      # backward onto rank 1023
    assert miss(1025, 2047, True) and miss(2047, 2047, True)
    assert not miss(1024, 2047, True) and not miss(2048, 2047, True)


def test_totals_are_the_instance_counts_of_each_emission_block():
    P = 5000
    rng = np.random.default_rng(3)
    keys = (0x3F800000 + rng.permutation(P)).astype(np.uint32)
    inst = rng.integers(0, 4, P).astype(np.uint32)
    order, miss, totals = M.repair(M.sorted_order(keys), keys, inst)
    assert not miss and totals.size == 5
    for k in range(5):
        blk = inst[order[k * 1024:(k + 1) * 1024]].astype(np.uint64)
        assert int(totals[k]) == int(blk.sum()) + (int((blk != 0).sum()) << 40)


def test_keys_of_depths():
    z = np.array([1.0, 0.2, 0.20000002, 0.0, -1.0, -np.inf, np.inf, 3.5], dtype=np.float32)
    k = M.keys_of_depths(z)
    assert k[0] == 0x3F800000 and k[6] == 0x7F800000 and k[7] == 0x40600000
    assert k[1] == 0x3E4CCCCC and k[2] == 0x3E4CCCCE and k[5] == 1   # the near plane itself; just in front; as far behind as it gets
    assert k[5] < k[4] < k[3] < k[1] < k[2] < k[0]                   # monotone across the near plane, never 0
    nan = np.array([0x7FC00000, 0xFFC00000, 0xFFFFFFFF, 0x7F800001], dtype=np.uint32)
    assert np.array_equal(M.keys_of_depths(nan.view(np.float32)), nan)  # NaN depths keep their bits, sign and payload


def test_the_case_table_has_hits_and_misses():
    verdicts = {c.id: S.model(c)[2][1] for c in S.CASES}
    assert len(verdicts) == len(S.CASES)   # (ids are unique)
    misses = sum(verdicts.values())
    assert misses >= 8 and len(verdicts) - misses >= 8, (misses, len(verdicts))
    for tile, in_flight in ((16, False), (15, True)):   # ... and so has each variant of the launch
        v = [verdicts[c.id] for c in S.CASES if c.tile == tile and c.in_flight == in_flight]
        assert sum(v) >= 4 and len(v) - sum(v) >= 4, (tile, in_flight, v)
    for c in S.CASES:   # on every hit the model's array is the sort of frame 1's keys
        carry, k1, (order, miss, _) = S.model(c)
        if not miss:
            assert np.array_equal(order, M.sorted_order(k1)), c.id
    for P, gs in S.ALL_ONES:
        keys = M.keys_of_depths(S.all_ones_depths(P, gs))
        assert (keys[list(gs)] == 0xFFFFFFFF).all()
        assert M.repair(M.sorted_order(keys), keys)[1] is True
