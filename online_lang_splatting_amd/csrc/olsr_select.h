// olsr_select.h — the steps of the radix select on 32-bit keys that k_frontend.hip and k_keyframe_seed.hip share
// ("The radix select: one copy").
//
// Include after olsr_device.h (u32 comes from there).
//
// The select finds the key of a given rank among the keys that take part, most significant digit first: SELECT_PASSES
// passes of 8 bits.  A pass counts, per workgroup, the keys that share the digits found so far into h[256] by their next
// digit (select_count), adds h to the pass's global histogram (select_flush), and one workgroup of 256 threads — thread t
// holds bucket t's count — scans the counts with block_excl_scan and narrows to the bucket that holds the rank
// (select_narrow).  The histograms are integer atomics: the order of the additions is free, the result is not.
//
// Whether an element takes part is the caller's argument and never a reserved key: every 32-bit word can be a key.  (The
// front end stores 0xFFFFFFFF for an element that takes no part and passes `key != FE_NO_KEY`; the seeding's sampling key
// is a bijection of the pixel index, so 0xFFFFFFFF is the key of one pixel per seed and has to be counted.)
//
// Barriers: none in here.  The one barrier of a scan-and-narrow is block_excl_scan's, called at the site because pass 0
// takes a rank from the scan's total (the lower median of n keys, the n_keep-th smallest key of n_valid); the barriers
// around h, s_w, *s_prefix and *s_rank stand at the call sites as olsr_collectives.h asks.
#pragma once

namespace olsr {

constexpr int SELECT_PASSES = 4;   // 8-bit digits, most significant first
__host__ __device__ constexpr int select_shift(int pass) { return 24 - 8 * pass; }

// one key into the workgroup's histogram h[256] of `pass`, when it takes part and shares the prefix of the passes before
// (pass 0 has no prefix: every key that takes part is counted)
__device__ __forceinline__ void select_count(u32* h, bool takes_part, u32 key, int pass, u32 prefix) {
  if (!takes_part) return;
  const int shift = select_shift(pass);
  if (pass > 0 && (key >> (shift + 8)) != prefix) return;
  atomicAdd(&h[(key >> shift) & 255u], 1u);
}

// the workgroup's histogram into the pass's global one g[256] (between two barriers of the caller)
__device__ __forceinline__ void select_flush(const u32* h, u32* g) {
  const u32 c = h[threadIdx.x];
  if (c) atomicAdd(&g[threadIdx.x], c);
}

// Thread t holds bucket t's count `cnt` and its exclusive prefix `excl` over the buckets.  The one thread whose bucket holds
// the rank (excl <= rank < excl + cnt; none when rank >= the total) leaves the prefix with its digit appended and the rank
// inside the bucket in *s_prefix and *s_rank (LDS), which the caller reads behind a barrier of its own.
__device__ __forceinline__ void select_narrow(u32 cnt, u32 excl, u32 prefix, u32 rank, u32* s_prefix, u32* s_rank) {
  if (cnt && excl <= rank && rank < excl + cnt) {
    *s_prefix = (prefix << 8) | threadIdx.x;
    *s_rank = rank - excl;
  }
}

}  // namespace olsr
