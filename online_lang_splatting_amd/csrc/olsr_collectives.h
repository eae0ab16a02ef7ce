// olsr_collectives.h — the wave64 and workgroup scans, sums and ranks every kernel file shares
// ("Wave and workgroup scans, sums and ranks: one copy").
//
// Included at the end of olsr_device.h (lane_id(), ballot(), u32 and u64 come from there).
//
// Barrier contract of the workgroup forms (block_excl_scan, block_rank, single_block_sum): every thread of the workgroup
// calls them; each holds EXACTLY ONE __syncthreads(), between writing the per-wave words s_w[NW] (LDS, supplied by the
// caller) and reading them.  A caller that uses s_w again — a second call, or other data in the same words — writes its
// own __syncthreads() in between, so that the reuse shows at the site.  (block_list_base and single_block_excl_scan
// end with that barrier themselves: they may be called again at once.)
//
// Only integers are combined ACROSS waves here: their sums are exact, so the order is free.  Floating-point values share
// wave_sum alone (one fixed order); how the waves' sums are combined is part of each result's bits and stays at its site.
#pragma once

namespace olsr {

// inclusive prefix over the lanes of a wave
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// sum over the lanes of a wave, in every lane: xor butterfly, steps 32, 16, 8, 4, 2, 1 (integer and floating types)
// (the argument by reference: an element of a local array handed over by value is inlined differently by the clang of
//  ROCm 7.2 (AMD clang 22.0.0git) — mapping_loss_kernel and pb_chain_kernel then need up to 29 more VGPRs and lose a wave
//  of occupancy; profiles/collectives_isa.json holds the figures to compare a later toolchain against)
template <class T>
__device__ __forceinline__ T wave_sum(const T& x) {
  T v = x;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// exclusive prefix of v over the 64 * NW threads of the workgroup, in thread order; *total (unless null) = the sum
template <int NW, class T>
__device__ __forceinline__ T block_excl_scan(T v, T* s_w /* [NW] */, T* total = nullptr) {
  const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
  const T incl = wave_incl_scan(v);
  if (lane == 63) s_w[w] = incl;
  __syncthreads();
  T before = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const T c = s_w[i];
    before += (i < w) ? c : (T)0;
    tot += c;
  }
  if (total) *total = tot;
  return before + incl - v;
}

// block_excl_scan of a 0 / 1 value: one ballot instead of six shuffles
template <int NW>
__device__ __forceinline__ u32 block_rank(bool flag, u32* s_w /* [NW] */, u32* total = nullptr) {
  const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
  const u64 m = ballot(flag);
  if (lane == 0) s_w[w] = (u32)__popcll(m);
  __syncthreads();
  u32 before = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const u32 c = s_w[i];
    before += (i < w) ? c : 0u;
    tot += c;
  }
  if (total) *total = tot;
  return before + (u32)__popcll(m & ((1ull << lane) - 1ull));
}

// Base slot of this thread's `cnt` entries of a list that workgroups append to: ONE global atomic per workgroup.
// Same-address atomics serialise at the memory side (~5 ns each on MI355X: one per wave of a P = 500 k launch is ~40 us);
// the counts are combined in LDS first.  (The list order influences no result.)
template <int NW>
__device__ __forceinline__ u32 block_list_base(u32 cnt, int32_t* counter, u32* s_w /* [NW] */, u32* s_base) {
  u32 tot;
  const u32 excl = block_excl_scan<NW>(cnt, s_w, &tot);
  if (threadIdx.x == 0) *s_base = tot ? (u32)atomicAdd(counter, (int)tot) : 0u;
  __syncthreads();
  const u32 slot = *s_base + excl;
  __syncthreads();  // (s_w / s_base may be reused by a second call)
  return slot;
}

// One workgroup of 64 * NW threads: the sum of in[0 .. n), in every thread.
template <int NW, class T>
__device__ __forceinline__ T single_block_sum(int n, const T* __restrict__ in, T* s_w /* [NW] */) {
  T s = 0;
  for (int i = (int)threadIdx.x; i < n; i += 64 * NW) s += in[i];
  s = wave_sum(s);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = s;
  __syncthreads();
  T tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) tot += s_w[i];
  return tot;
}

// One workgroup of 64 * NW threads: out[i] = in[0] + ... + in[i - 1] for i < n (any n: rounds of 64 * NW values, the
// running total carried from round to round); returns the total in every thread.  `out` may be `in`.
template <int NW, class T>
__device__ __forceinline__ T single_block_excl_scan(int n, const T* in, T* out, T* s_w /* [NW] */) {
  T carry = 0;
  for (int base = 0; base < n; base += 64 * NW) {
    const int i = base + (int)threadIdx.x;
    T round;
    const T excl = block_excl_scan<NW>(i < n ? in[i] : (T)0, s_w, &round);
    if (i < n) out[i] = carry + excl;
    carry += round;
    __syncthreads();  // (s_w is rewritten by the next round, or by the caller's next scan)
  }
  return carry;
}

// the smaller of a host-side count and, when there is one, the device-side count of the same thing
__device__ __forceinline__ int64_t bounded_n(int64_t n_host, const int32_t* n_dev) {
  if (n_dev) {
    const int64_t nd = (int64_t)(*n_dev);
    return nd < n_host ? nd : n_host;
  }
  return n_host;
}

}  // namespace olsr
