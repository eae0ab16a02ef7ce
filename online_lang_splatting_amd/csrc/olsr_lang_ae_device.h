// olsr_lang_ae_device.h — the online language autoencoder 32 -> 24 -> 15 -> 24 -> 32 of one row, in one lane's registers:
// the flat parameter layout of olsr_lang_ae_* and the forward halves, on olsr_dense.h's per-lane layers.  k_lang_ae.hip trains, encodes and decodes with them,
// k_lang_encoder.hip encodes its unit rows, k_lang_query.hip decodes its codes: one sequence of operations, so the three
// agree bit for bit.  Device only; -ffp-contract=off holds, every fma is written out.
#pragma once
#include "../../include/olsr.h"
#include "olsr_dense.h"  // lane_linear, lane_norm

namespace olsr {

constexpr int AE_IN = OLSR_LANG_AE_IN, AE_H = OLSR_LANG_AE_HIDDEN, AE_C = OLSR_LANG_AE_CODE;
constexpr int AE_NP = OLSR_LANG_AE_PARAMS;
// offsets into the flat parameter array (state_dict order)
constexpr int AE_W1 = 0, AE_B1 = AE_W1 + AE_H * AE_IN, AE_W2 = AE_B1 + AE_H, AE_B2 = AE_W2 + AE_C * AE_H;
constexpr int AE_W3 = AE_B2 + AE_C, AE_B3 = AE_W3 + AE_H * AE_C, AE_W4 = AE_B3 + AE_H, AE_B4 = AE_W4 + AE_IN * AE_H;
static_assert(AE_B4 + AE_IN == AE_NP, "flat parameter layout");

// encode: h1 = relu(W1 x + b1), c = z / |z| with z = W2 h1 + b2; returns |z|
__device__ __forceinline__ float ae_encode(const float* __restrict__ P, const float (&x)[AE_IN], float (&h1)[AE_H],
                                           float (&c)[AE_C]) {
  lane_linear<AE_H, AE_IN>(P + AE_W1, P + AE_B1, x, h1);
#pragma unroll
  for (int k = 0; k < AE_H; ++k) h1[k] = fmaxf(h1[k], 0.f);
  lane_linear<AE_C, AE_H>(P + AE_W2, P + AE_B2, h1, c);
  const float n = lane_norm<AE_C>(c);
#pragma unroll
  for (int k = 0; k < AE_C; ++k) c[k] = c[k] / n;
  return n;
}

// decode: h2 = relu(W3 c + b3), r = y / |y| with y = W4 h2 + b4; returns |y|
__device__ __forceinline__ float ae_decode(const float* __restrict__ P, const float (&c)[AE_C], float (&h2)[AE_H],
                                           float (&r)[AE_IN]) {
  lane_linear<AE_H, AE_C>(P + AE_W3, P + AE_B3, c, h2);
#pragma unroll
  for (int k = 0; k < AE_H; ++k) h2[k] = fmaxf(h2[k], 0.f);
  lane_linear<AE_IN, AE_H>(P + AE_W4, P + AE_B4, h2, r);
  const float n = lane_norm<AE_IN>(r);
#pragma unroll
  for (int k = 0; k < AE_IN; ++k) r[k] = r[k] / n;
  return n;
}

// codes of one row: [N,15] rows (layout 0) or [15,N] channel-major (layout 1)
__device__ __forceinline__ void ae_store_codes(float* __restrict__ codes, int layout, int N, int row, const float (&c)[AE_C]) {
#pragma unroll
  for (int k = 0; k < AE_C; ++k) {
    if (layout == OLSR_LANG_AE_CODES_CHANNELS) codes[(size_t)k * N + row] = c[k];
    else codes[(size_t)row * AE_C + k] = c[k];
  }
}

}  // namespace olsr
