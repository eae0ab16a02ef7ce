// olsr_dense.h — the dense layer Y^T = W X^T on v_mfma_f32_16x16x4_f32 that the language nets share (k_lang_query.hip,
// k_lang_encoder.hip, k_lang_single_stage.hip, k_hr_net.hip), and the 4-float vector every MFMA user names (k_render_fwd.hip, k_render_bwd.hip).
//
// Device only; included after olsr_device.h by the units that use it.
//
// Operand layout, once for every caller.  The weights are the A operand, the activations of 64 pixels the B operand.  Lane
// (li = lane & 15, q = lane >> 4) supplies, for the MFMA of element j of a 16-deep k block at k0,
//     A[i = li][k = q] = W[n + li][k0 + 4 q + j]        B[k = q][col = li] = X[pixel 16 pt + li][k0 + 4 q + j]:
// the k order inside a block is permuted the same way on both sides, and each side is one 16-byte load.  In the D layout lane
// (li, q) holds neurons n0 + 16 t + 4 q + {0..3} of pixel 16 pt + li in acc[t][pt].  An MFMA is a k-ordered fmaf chain, so
// the order j, t, pt below and the order of the blocks are part of every result's bits.
#pragma once

namespace olsr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// one 16-deep k block of acc[NT x 16 neurons][64 pixels] += W X^T, given its operands
template <int NT>
__device__ __forceinline__ void dense_mfma_block(const f32x4 (&a)[NT], const f32x4 (&b)[4], f32x4 (&acc)[NT][4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[t][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], b[pt][j], acc[t][pt], 0, 0, 0);
}

// the same with B out of a pixel-major LDS image of S floats per pixel; xk: the lane's pixel li at k0 + 4 q
template <int NT, int S>
__device__ __forceinline__ void dense_block(const f32x4 (&a)[NT], const float* __restrict__ xk, f32x4 (&acc)[NT][4]) {
  f32x4 b[4];
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) b[pt] = *reinterpret_cast<const f32x4*>(xk + pt * 16 * S);
  dense_mfma_block<NT>(a, b, acc);
}

template <int NT>
__device__ __forceinline__ void dense_bias(const float* __restrict__ bias, int n0, int q, f32x4 (&acc)[NT][4]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + n0 + 16 * t + 4 * q);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[t][pt] = bv;
  }
}

// acc[t][pt] = the tile (neurons n0 + 16 t .. + 15) x (pixels 16 pt .. + 15) of W X^T + b over the whole KIN.  The next
// block's weights are loaded before this block's MFMAs are issued.
template <int KIN, int NT, int S>
__device__ __forceinline__ void dense_gemm(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                           int n0, int li, int q, f32x4 (&acc)[NT][4]) {
  static_assert(KIN % 16 == 0 && KIN <= S, "k blocks of 16 out of the image");
  dense_bias<NT>(bias, n0, q, acc);
  const float* wp = W + (size_t)(n0 + li) * KIN + 4 * q;
  const float* xp = X + li * S + 4 * q;
  f32x4 a[NT], an[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * 16 * KIN);
#pragma unroll 2
  for (int k0 = 0; k0 < KIN; k0 += 16) {
    const int kn = k0 + 16 < KIN ? k0 + 16 : k0;
#pragma unroll
    for (int t = 0; t < NT; ++t) an[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * 16 * KIN + kn);
    dense_block<NT, S>(a, xp + k0, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) a[t] = an[t];
  }
}

// ReLU as torch has it: fmaxf(v, 0), except that a NaN stays a NaN (fmaxf alone returns the other operand, and a NaN input row
// would come out as finite numbers)
__device__ __forceinline__ float relu_keep_nan(float v) { return v != v ? v : fmaxf(v, 0.f); }

// BatchNorm in eval(): alpha = weight / sqrt(running_var + eps), beta = bias - running_mean alpha of channel c of
// bn = [weight | bias | mean | var][C], in double, rounded once
__device__ __forceinline__ void bn_fold(const float* __restrict__ bn, int C, int c, double eps, float& alpha, float& beta) {
  const double a = (double)bn[c] / sqrt((double)bn[3 * C + c] + eps);
  alpha = (float)a;
  beta = (float)((double)bn[C + c] - (double)bn[2 * C + c] * a);
}

// What a layer does to its accumulators on their way into the image.  The two ReLUs differ: DENSE_EPI_RELU is the text
// query's plain fmaxf, which turns a NaN activation into 0; DENSE_EPI_BN_RELU keeps it, as torch does.  Each is what its net
// computed before the layers were shared, and which of the two the query should have is a question of behaviour, not of
// sharing: neither was touched.  DENSE_EPI_RELU_NAN is the ReLU alone with the NaN kept: the single-stage query's
// (k_lang_single_stage.hip), where a NaN code pixel has to come out as NaN similarities.
enum { DENSE_EPI_NONE = 0, DENSE_EPI_RELU = 1, DENSE_EPI_BN_RELU = 2, DENSE_EPI_RELU_NAN = 3 };

// the accumulators into the image X[64][S]; alpha, beta: the layer's folded BatchNorm per neuron (DENSE_EPI_BN_RELU)
template <int NT, int S, int EPI>
__device__ __forceinline__ void dense_store(float* __restrict__ X, const float* __restrict__ alpha, const float* __restrict__ beta,
                                            int n0, int li, int q, const f32x4 (&acc)[NT][4]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + 4 * q;
    f32x4 al = f32x4{1.f, 1.f, 1.f, 1.f}, be = f32x4{0.f, 0.f, 0.f, 0.f};
    if (EPI == DENSE_EPI_BN_RELU) {
      al = *reinterpret_cast<const f32x4*>(alpha + n);
      be = *reinterpret_cast<const f32x4*>(beta + n);
    }
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      f32x4 v = acc[t][pt];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (EPI == DENSE_EPI_RELU) v[r] = fmaxf(v[r], 0.f);
        if (EPI == DENSE_EPI_BN_RELU) v[r] = relu_keep_nan(fmaf(al[r], v[r], be[r]));
        if (EPI == DENSE_EPI_RELU_NAN) v[r] = relu_keep_nan(v[r]);
      }
      *reinterpret_cast<f32x4*>(X + (pt * 16 + li) * S + n) = v;
    }
  }
}

// One layer out of the image, in place: X[64][KIN] -> X[64][NOUT].  The first WUSED of the workgroup's WAVES waves share the
// neurons and keep them in accumulators until every wave has read the layer's input.  Every thread calls it: two barriers.
template <int KIN, int NOUT, int WAVES, int WUSED, int S, int EPI>
__device__ __forceinline__ void dense_layer(float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                            const float* __restrict__ alpha, const float* __restrict__ beta, int wave, int li,
                                            int q) {
  constexpr int NT = NOUT / (16 * WUSED);
  static_assert(NT * 16 * WUSED == NOUT && WUSED <= WAVES && NOUT <= S, "an equal share per wave");
  const int n0 = wave * NT * 16;
  const bool mine = WUSED == WAVES || wave < WUSED;  // (no test at all when every wave takes part)
  f32x4 acc[NT][4];
  if (mine) dense_gemm<KIN, NT, S>(X, W, bias, n0, li, q, acc);
  __syncthreads();  // every wave has read the layer's input
  if (mine) dense_store<NT, S, EPI>(X, alpha, beta, n0, li, q, acc);
  __syncthreads();
}

}  // namespace olsr
