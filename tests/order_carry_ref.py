"""Host model of the carried depth order's repair (online_lang_splatting_amd/csrc/k_order_carry.hip) in numpy: the ALGORITHM —
which ranks a window holds, what stands in for ranks outside [0, P), what is compared with what — not the implementation (no
merge levels, no galloping searches, no level skipping: a window sort is np.sort on the 64-bit pairs, which is what a stable
merge sort of them leaves).  The verdict `miss` and the array left behind are pure functions of (array on entry, keys), so the
kernels can be held to this model with equalities (tests/test_gpu_order_carry_model.py); that the model itself is sound — a
hit is always the sort — and complete up to half a window is tests/test_order_carry_ref_cpu.py.

    phase A   window b holds ranks [b W, (b + 1) W) of the array on entry, each as the pair (keys[g] << 32 | g); a rank
              >= P is the high pad (0xFFFFFFFF << 32 | l), l its place in the window; an entry g >= P takes the key
              0xFFFFFFFF and raises miss; THE GUARD: so does an entry g < P whose key is 0xFFFFFFFF, because the pads do not
              lie above such a pair.  The sorted window's first ranks below P are phase A's output.
    phase B   window j holds ranks [j W - W / 2, j W + W / 2) of phase A's output; ranks < 0 are low pads (0 << 32 | l),
              ranks >= P high pads.  Sorted; its places that are ranks in [0, P) are the result.  miss unless: inside the
              window every written rank's pair is strictly above its predecessor's (place 0 and rank 0 have none), every
              written index is < P, and the window's LAST pair — pad or not — is strictly below the smaller of the two pairs of
              phase A's output at the next window's first rank and half a window further (those that are < P).
    totals    per EMIT_CHUNK ranks of the result, the instance counts of its Gaussians packed as emit_total_pack does.
"""
import numpy as np

W = 2048            # OC_W
HALF = W // 2
EMIT_CHUNK = 1024
EMIT_TOTAL_SHIFT = 40
KEY_PAD = 0xFFFFFFFF
U64 = np.uint64


def sorted_order(keys_u32):
    """The reference's order: ascending (key, index) — what the radix passes leave."""
    keys = np.asarray(keys_u32, dtype=np.uint32)
    return np.lexsort((np.arange(keys.size), keys)).astype(np.uint32)


def keys_of_depths(depths_f32):
    """The sort key of k_preprocess.hip (preprocess_one) on bit patterns: the depth's bits where NOT (z <= 0.2f) — a NaN of
    either sign included —, and behind the near plane 0x3E4CCCCC - min(bits(0.2f - z) >> 1, 0x3E4CCCCB), at least 1."""
    z = np.ascontiguousarray(depths_f32, dtype=np.float32)
    bits = z.view(np.uint32)
    behind = z <= np.float32(0.2)          # (False for NaN)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.float32(0.2) - np.where(behind, z, np.float32(0.0))).astype(np.float32)
    tb = np.minimum(t.view(np.uint32) >> np.uint32(1), np.uint32(0x3E4CCCCB))
    return np.where(behind, np.uint32(0x3E4CCCCC) - tb, bits).astype(np.uint32)


def _pairs(key, gid):
    return (key.astype(U64) << U64(32)) | gid.astype(U64)


def emit_total_pack(inst):
    inst = np.asarray(inst).astype(U64)
    return inst | ((inst != 0).astype(U64) << U64(EMIT_TOTAL_SHIFT))


def repair(carry_u32, keys_u32, inst_count=None):
    """(order uint32[P], miss, totals uint64[ceil(P / EMIT_CHUNK)] or None) — what the two launches leave in the array, their
    verdict, and (given inst_count uint32[P]) the totals phase B leaves for the emission.  On a miss `order` is NOT the frame's
    order (the radix passes overwrite it); it is returned as the kernels would have written it."""
    carry = np.asarray(carry_u32).astype(np.uint32)
    keys = np.asarray(keys_u32).astype(np.uint32)
    P = carry.size
    assert keys.size == P and P > 0
    lanes = np.arange(W, dtype=U64)
    pad_low, pad_high = lanes, (U64(KEY_PAD) << U64(32)) | lanes
    miss = False

    # phase A
    in_range = carry < P
    key = np.where(in_range, keys[np.where(in_range, carry, 0)], np.uint32(KEY_PAD))
    miss |= bool((key == KEY_PAD).any())   # an index out of range, or (the guard) a real key the pads do not lie above
    real = _pairs(key, carry)
    a_out = np.empty(P, dtype=U64)
    for base in range(0, P, W):
        n = min(W, P - base)
        win = pad_high.copy()
        win[:n] = real[base:base + n]
        a_out[base:base + n] = np.sort(win, kind="stable")[:n]

    # phase B
    out = np.empty(P, dtype=U64)
    nb = (P + HALF + W - 1) // W
    for j in range(nb):
        start = j * W - HALF
        lo, hi = max(start, 0), min(start + W, P)          # the ranks of this window that exist
        win = np.where(start + lanes.astype(np.int64) < 0, pad_low, pad_high)
        win[lo - start:hi - start] = a_out[lo:hi]
        r = np.sort(win, kind="stable")
        out[lo:hi] = r[lo - start:hi - start]
        first = max(lo - start, 1) if lo > 0 else lo - start + 1   # places l > 0 whose rank i > 0
        miss |= bool((r[first:hi - start] <= r[first - 1:hi - start - 1]).any())
        nxt = start + W
        if nxt < P:
            nmin = a_out[nxt]
            if nxt + HALF < P:
                nmin = min(nmin, a_out[nxt + HALF])
            miss |= not (r[W - 1] < nmin)
    order = (out & U64(0xFFFFFFFF)).astype(np.uint32)
    miss |= bool((order >= P).any())

    totals = None
    if inst_count is not None:
        inst = np.asarray(inst_count).astype(np.uint32)
        packed = np.where(order < P, emit_total_pack(inst[np.where(order < P, order, 0)]), U64(0))
        nt = (P + EMIT_CHUNK - 1) // EMIT_CHUNK
        totals = np.array([packed[k * EMIT_CHUNK:(k + 1) * EMIT_CHUNK].sum(dtype=U64) for k in range(nt)], dtype=U64)
    return order, bool(miss), totals
