"""The case table that tests/test_order_carry_ref_cpu.py (the host model alone) and tests/test_gpu_order_carry_model.py (the
kernels against the model) share: two frames of P Gaussians on the optical axis whose depth is their rank — frame 0
z = 1 + rank * 2**-12 (exact in fp32), frame 1 a permutation of those depths — so that the carried array frame 0 leaves is known
and frame 1 moves chosen elements by chosen numbers of ranks across chosen window edges.  numpy only.

A case says where every element of frame 0's order belongs in frame 1:
  move_fwd (s, d)   the element at rank s belongs at rank s + d (those between move down by one)
  move_bwd (s, d)   the element at rank s + d belongs at rank s (those between move up by one)
  reverse  (s, L)   ranks [s, s + L) in reverse
  ties     (s, L)   ranks [s, s + L) take ONE depth; their order in the array is the reverse of the index order ties go by
"""
from dataclasses import dataclass

import numpy as np

import order_carry_ref as M

STEP = 2.0 ** -12
SIZES = (7000, 10000)     # a carried order's fallback: the one-launch sort (<= 8192) / the radix passes
MOVES = (1023, 1024, 1025, 2047, 2048)


@dataclass(frozen=True)
class Case:
    kind: str
    P: int
    a: int               # s
    b: int               # d or L
    F: int = 0
    tile: int = 15
    in_flight: bool = False   # _abi.FLAG_FRAMES_IN_FLIGHT: the 256-thread instantiation

    @property
    def id(self):
        return (f"{self.kind}-P{self.P}-{self.a}-{self.b}-F{self.F}" + ("-t16" if self.tile == 16 else "")
                + ("-inflight" if self.in_flight else ""))


def starts(P, d):
    return (0, 1, 1023, 1024, 1025, 2047, 2048, 3000, P - 1 - d)


def _table():
    cases, n = [], 0

    def add(kind, P, a, b, **kw):
        nonlocal n
        cases.append(Case(kind, P, a, b, F=(0, 3)[n % 2], **kw))
        n += 1
    for P in SIZES:
        for d in MOVES:
            for s in starts(P, d):
                add("move_fwd", P, s, d)
                add("move_bwd", P, s, d)
        for L in (1024, 1025, 2049):
            add("reverse", P, 2 * M.W - L // 2, L)            # astride a window edge (rank 4096)
            add("reverse", P, M.W + M.HALF - L // 2, L)       # astride a half-window edge (rank 3072)
        add("ties", P, 2500, 3000)
        add("ties", P, 2500, 1025)
    # each family once more (a hit and a miss of each) in the 256-thread instantiation and with tile 16
    for kw in (dict(in_flight=True), dict(tile=16)):
        for P in SIZES:
            add("move_fwd", P, 1023, 1024, **kw)
            add("move_fwd", P, 2047, 1025, **kw)
            add("move_bwd", P, 1024, 1024, **kw)
            add("move_bwd", P, 1023, 1025, **kw)
            add("reverse", P, 2 * M.W - 512, 1025, **kw)
            add("reverse", P, M.W + M.HALF - 1024, 2049, **kw)
            add("ties", P, 2500, 1025, **kw)
            add("ties", P, 2500, 3000, **kw)
    return cases


CASES = _table()

# (P, the Gaussians whose depth has the bit pattern 0xFFFFFFFF): below 1024, between 1024 and 2048, above; one and several
ALL_ONES = [(P, gs) for P in (3000, 4096, 10000) for gs in ((5,), (1500,), (2500,), (5, 1500, 2500))]


def rank0_of(kind, P):
    """Gaussian index -> its rank in frame 0.  A fixed shuffle (an index is not its rank anywhere in these tests), except for
    the tie cases, where descending index = ascending rank makes the array the reverse of the order equal keys take."""
    if kind == "ties":
        return np.arange(P - 1, -1, -1, dtype=np.int64)
    return np.random.default_rng(1000 + P).permutation(P).astype(np.int64)


def new_rank(case):
    """rank in frame 0 -> the depth slot (rank, up to ties) in frame 1"""
    r = np.arange(case.P, dtype=np.int64)
    s, n = case.a, case.b
    if case.kind == "move_fwd":
        assert 0 <= s and s + n < case.P
        r[s], r[s + 1:s + n + 1] = s + n, np.arange(s, s + n)
    elif case.kind == "move_bwd":
        assert 0 <= s and s + n < case.P
        r[s + n], r[s:s + n] = s, np.arange(s + 1, s + n + 1)
    elif case.kind == "reverse":
        assert 0 <= s and s + n <= case.P
        r[s:s + n] = r[s:s + n][::-1].copy()
    elif case.kind == "ties":
        assert 0 <= s and s + n <= case.P
        r[s:s + n] = s
    else:
        raise KeyError(case.kind)
    return r


def depths(case):
    """(frame 0's depths, frame 1's) per Gaussian, float32"""
    r0 = rank0_of(case.kind, case.P)
    z = lambda r: (1.0 + r.astype(np.float64) * STEP).astype(np.float32)  # noqa: E731  (exact: 13 + 12 bits at most)
    return z(r0), z(new_rank(case)[r0])


def model(case):
    """(the array frame 0 leaves, frame 1's keys, the model's (order, miss, totals) on them)"""
    z0, z1 = depths(case)
    carry = M.sorted_order(M.keys_of_depths(z0))
    k1 = M.keys_of_depths(z1)
    return carry, k1, M.repair(carry, k1)


def all_ones_depths(P, gs):
    """the depths of an all-ones case: frame 0's of the shuffle, with the bit pattern 0xFFFFFFFF on the Gaussians gs"""
    z = (1.0 + rank0_of("all_ones", P).astype(np.float64) * STEP).astype(np.float32)
    z.view(np.uint32)[list(gs)] = 0xFFFFFFFF
    return z
