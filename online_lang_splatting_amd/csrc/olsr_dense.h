// olsr_dense.h — the dense layer Y^T = W X^T on v_mfma_f32_16x16x4_f32 that the language nets share (k_lang_query.hip,
// k_lang_encoder.hip, k_hr_net.hip), and the 4-float vector every MFMA user names (k_render_fwd.hip, k_render_bwd.hip).  Around
// the product, what the two encoders and the two stage-A kernels of the text query have in common: the flat parameter layout,
// the BatchNorm table, the streamed first layer, the phrase tail, the per-lane layers of the vector unit, and the launch.
//
// Device code but for dense_launch; included after olsr_device.h by the units that use it.
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

// The tile of the language nets' kernels: 64 pixels (four 16-pixel MFMA column tiles) per workgroup of four waves.
constexpr int LANG_M = 64;               // pixels per workgroup
constexpr int LANG_WAVES = 4;            // 256 threads
constexpr int LANG_S = 516;              // LDS floats per pixel of the activation image: 512 + 4 (16 pixels' float4 reads of one
                                         // k column hit 64 different banks)
constexpr int LANG_KC = 64;              // input channels per chunk of a streamed first layer
constexpr int LANG_CS = LANG_KC + 4;     // LDS floats per pixel of a chunk (68 = 4 mod 64, as LANG_S)
constexpr size_t LANG_ACT_BYTES = (size_t)LANG_M * LANG_S * sizeof(float);  // the activation image
static_assert(LANG_ACT_BYTES <= 160 * 1024, "one LDS image per workgroup");

// The flat parameter array of an MLP of L Linear layers in state_dict order: per layer weight [d[i + 1], d[i]] at w[i] and
// bias at b[i]; with bn, behind every layer but the last a BatchNorm1d's weight | bias | running_mean | running_var at n[i],
// and a[i], where the layer's channels start in the folded table alpha[bn_channels] | beta[bn_channels] (bn_fold_table).
template <int L>
struct FlatMlp {
  int d[L + 1], w[L], b[L], n[L], a[L];
  int bn_channels, total;
};
template <int NW>
constexpr FlatMlp<NW - 1> flat_mlp(const int (&widths)[NW], bool bn) {
  FlatMlp<NW - 1> f{};
  f.d[0] = widths[0];
  int at = 0, ch = 0;
  for (int i = 0; i < NW - 1; ++i) {
    f.d[i + 1] = widths[i + 1];
    f.w[i] = at, at += widths[i + 1] * widths[i];
    f.b[i] = at, at += widths[i + 1];
    f.n[i] = at, f.a[i] = ch;
    if (bn && i + 1 < NW - 1) at += 4 * widths[i + 1], ch += widths[i + 1];
  }
  f.bn_channels = ch, f.total = at;
  return f;
}
// 16-byte loads of every weight and bias from layer `first` on (the matrix layers; an array that is itself 16-byte aligned)
template <int L>
constexpr bool flat_mlp_aligned(const FlatMlp<L>& f, int first = 0) {
  for (int i = first; i < L; ++i)
    if (f.w[i] % 4 != 0 || f.b[i] % 4 != 0) return false;
  return true;
}

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
// every BatchNorm channel of the net f in P into alpha[f.bn_channels] | beta[f.bn_channels], by the workgroup's `threads`
// threads (a channel's value is the same whoever computes it); the caller's next barrier publishes the table
template <int L>
__device__ __forceinline__ void bn_fold_table(const float* __restrict__ P, const FlatMlp<L>& f, double eps,
                                              float* __restrict__ alpha, float* __restrict__ beta, int tid, int threads) {
#pragma unroll
  for (int i = 0; i + 1 < L; ++i)
    for (int c = tid; c < f.d[i + 1]; c += threads) bn_fold(P + f.n[i], f.d[i + 1], c, eps, alpha[f.a[i] + c], beta[f.a[i] + c]);
}

// The vector unit's counterpart of dense_layer, for widths that are no multiples of the 16-wide matrix tile: y = W x + b of
// one row in one lane's registers, W [OUT, IN] row-major, every neuron an fmaf chain that starts from the bias and takes k in
// ascending order; uniform addresses (every lane reads the same parameter).  -ffp-contract=off holds, every fma is written out.
template <int OUT, int IN>
__device__ __forceinline__ void lane_linear(const float* __restrict__ W, const float* __restrict__ b, const float (&x)[IN],
                                            float (&y)[OUT]) {
#pragma unroll
  for (int o = 0; o < OUT; ++o) {
    float a = b[o];
#pragma unroll
    for (int i = 0; i < IN; ++i) a = fmaf(W[o * IN + i], x[i], a);
    y[o] = a;
  }
}

// |v| rounded once: the squares are exact in double, so v / |v| has unit norm to ~1 ulp (a float32 sum of 32 squares alone is
// off by up to a few ulp, which the rows of decode() would inherit; 111 double fmas per row beside ~9 400 float32 ones)
template <int K>
__device__ __forceinline__ float lane_norm(const float (&v)[K]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) s = fma((double)v[k], (double)v[k], s);
  return (float)sqrt(s);
}

// What a layer does to its accumulators on their way into the image.  The two ReLUs differ: DENSE_EPI_RELU is the text
// query's plain fmaxf, which turns a NaN activation into 0; DENSE_EPI_BN_RELU keeps it, as torch does.  Each is what its net
// computed before the layers were shared, and which of the two the query should have is a question of behaviour, not of
// sharing: neither was touched.  DENSE_EPI_RELU_NAN is the ReLU alone with the NaN kept: the single-stage query's
// (ss_query_sims_kernel, k_lang_query.hip), where a NaN code pixel has to come out as NaN similarities.
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

// A thread's 16 elements of the chunk of channels k0 .. k0 + 63 of an input of D0 channels: element i is (pixel, channel) =
// (tid & 63, (tid >> 6) + 4 i) of the channel-major map (CHANNELS), (channel, pixel) the other way round of rows; either way a
// wave's load is 64 consecutive floats.  No alignment is assumed, the pixel tail is guarded, nothing is read past the end.
template <bool CHANNELS, int D0>
__device__ __forceinline__ void dense_chunk_fetch(const float* __restrict__ f, int N, long long plane_stride, int row0, int k0,
                                                  int tid, float (&pre)[16]) {
  const int lo = tid & 63, hi = tid >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = CHANNELS ? lo : hi + 4 * i, c = CHANNELS ? hi + 4 * i : lo;
    const int row = row0 + p;
    float v = 0.f;
    if (row < N) v = CHANNELS ? f[(size_t)(k0 + c) * (size_t)plane_stride + row] : f[(size_t)row * D0 + k0 + c];
    pre[i] = v;
  }
}
// ... parked in the chunk buffer [64 pixels][CS]; both layouts fill the same LDS image, so both give the same bits
template <bool CHANNELS, int CS>
__device__ __forceinline__ void dense_chunk_park(float* __restrict__ buf, int tid, const float (&pre)[16]) {
  const int lo = tid & 63, hi = tid >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = CHANNELS ? lo : hi + 4 * i, c = CHANNELS ? hi + 4 * i : lo;
    buf[p * CS + c] = pre[i];
  }
}

// A first layer whose input does not fit the image: X[64][D1] = EPI(W f^T + b)^T for the 64 pixels from row0 of the D0-channel
// input f.  A wave owns D1 / WAVES neurons for all 64 pixels and keeps them in accumulators while the input passes through
// LDS in chunks of KC channels, [64 pixels][KC + 4] each, double-buffered: the next chunk's global loads are issued before the
// current chunk's MFMAs and stored behind them, the next k block's weights are loaded before this block's MFMAs.  The two
// chunk buffers lie inside the activation image, which is not in use before the layer has finished.  pre: chunk 0 as
// dense_chunk_fetch left it (the caller issues those loads ahead of whatever else it does first, the BatchNorm table for one,
// which the first barrier here publishes too).  Every thread of the WAVES waves calls it; it ends with its store and a barrier.
template <bool CHANNELS, int D0, int D1, int WAVES, int KC, int S, int EPI>
__device__ __forceinline__ void dense_streamed_layer(float* __restrict__ X, const float* __restrict__ f, int N,
                                                     long long plane_stride, int row0, const float* __restrict__ W,
                                                     const float* __restrict__ bias, const float* __restrict__ alpha,
                                                     const float* __restrict__ beta, int wave, int li, int q, int tid,
                                                     float (&pre)[16]) {
  constexpr int M = 64, CS = KC + 4, CHUNKS = D0 / KC, NT = D1 / (16 * WAVES);
  static_assert(NT * 16 * WAVES == D1 && D1 <= S, "an equal share per wave");
  static_assert(CHUNKS * KC == D0 && KC % 16 == 0 && 16 * 64 * WAVES == M * KC, "whole chunks, sixteen elements a thread");
  static_assert(2 * M * CS <= M * S, "both chunk buffers inside the activation image");
  dense_chunk_park<CHANNELS, CS>(X, tid, pre);
  __syncthreads();
  const int n0 = wave * NT * 16;
  f32x4 acc[NT][4];
  dense_bias<NT>(bias, n0, q, acc);
  const float* wp = W + (size_t)(n0 + li) * D0 + 4 * q;
  f32x4 a[NT], an[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * 16 * D0);
#pragma unroll 1
  for (int ch = 0; ch < CHUNKS; ++ch) {
    const bool more = ch + 1 < CHUNKS;
    if (more) dense_chunk_fetch<CHANNELS, D0>(f, N, plane_stride, row0, (ch + 1) * KC, tid, pre);
    const float* xp = X + (ch & 1) * M * CS + li * CS + 4 * q;
#pragma unroll
    for (int kb = 0; kb < KC; kb += 16) {
      const int k0 = ch * KC + kb;
      const int kn = k0 + 16 < D0 ? k0 + 16 : k0;
#pragma unroll
      for (int t = 0; t < NT; ++t) an[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * 16 * D0 + kn);
      dense_block<NT, CS>(a, xp + kb, acc);
#pragma unroll
      for (int t = 0; t < NT; ++t) a[t] = an[t];
    }
    if (more) dense_chunk_park<CHANNELS, CS>(X + ((ch + 1) & 1) * M * CS, tid, pre);  // last read before the previous barrier
    __syncthreads();
  }
  // (every wave is past its last chunk read)
  dense_store<NT, S, EPI>(X, alpha, beta, n0, li, q, acc);
  __syncthreads();
}

// The tail of a text query's stage A: the last layer X[64][KIN] -> FEAT neurons in blocks of 4 x 16 neurons per wave, consumed
// as they arrive.  A block's accumulators are in the B-operand layout of the next product already (neuron on the register,
// pixel on the lane), so the K dot products with the phrase rows [K][FEAT] are four more MFMAs per 16 x 16 tile and |y|^2 is a
// per-lane sum in double: the FEAT-wide row is never stored.  Then the waves' partial dots and norms go through the image,
// which is dead by then, and sims[ph][row0 + px] = (y . phrase) / |y| for the pixels below N.  KT: 16-row tiles of phrases
// (K <= 16 KT).  Every thread of the WAVES waves calls it.
template <int KIN, int FEAT, int KT, int WAVES, int S>
__device__ __forceinline__ void dense_phrase_sims(float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                                  const float* __restrict__ phrases, int K, int N, int row0,
                                                  float* __restrict__ sims, int wave, int li, int q, int tid) {
  constexpr int M = 64, NT = 4, CHUNKS = FEAT / (16 * NT * WAVES);
  static_assert(CHUNKS * 16 * NT * WAVES == FEAT, "blocks of 64 neurons per wave");
  static_assert(WAVES == 4, "the sum of the waves' partial dots is written out for four");
  static_assert((size_t)WAVES * 16 * KT * M * sizeof(float) + (size_t)WAVES * 4 * M * sizeof(double) <= (size_t)M * S * sizeof(float),
                "the partial dots and norms inside the activation image");
  f32x4 sacc[KT][4];  // tile (phrases 16 kt ..) x (pixels 16 pt ..): lane (li, q) holds phrases 16 kt + 4 q + {0..3} of pixel 16 pt + li
  double nrm[4];      // this lane's part of |y|^2 of pixel 16 pt + li
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    nrm[pt] = 0.0;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) sacc[kt][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int ch = 0; ch < CHUNKS; ++ch) {
    const int n0 = (wave * CHUNKS + ch) * NT * 16;
    f32x4 acc[NT][4];
    dense_gemm<KIN, NT, S>(X, W, bias, n0, li, q, acc);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
#pragma unroll
        for (int r = 0; r < 4; ++r) nrm[pt] = fma((double)acc[t][pt][r], (double)acc[t][pt][r], nrm[pt]);
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) {
        // A[i = li][k = q] = phrase 16 kt + li at neuron n0 + 16 t + 4 q + r; B[k = q][col = li] = acc[t][pt][r] as it lies
        const int ph = kt * 16 + li;
        f32x4 pf = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ph < K) pf = *reinterpret_cast<const f32x4*>(phrases + (size_t)ph * FEAT + n0 + 16 * t + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
            sacc[kt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf[r], acc[t][pt][r], sacc[kt][pt], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the activations are no longer read
  float* dots = X;                                                  // [wave][16 KT phrases][64 pixels]
  double* norms = reinterpret_cast<double*>(X + WAVES * 16 * KT * M);  // [wave][q][64 pixels]
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    norms[(wave * 4 + q) * M + pt * 16 + li] = nrm[pt];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) dots[(wave * 16 * KT + kt * 16 + 4 * q + r) * M + pt * 16 + li] = sacc[kt][pt][r];
  }
  __syncthreads();
  for (int e = tid; e < K * M; e += M * WAVES) {
    const int ph = e / M, px = e - ph * M;
    if (row0 + px >= N) continue;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < WAVES * 4; ++k) s += norms[k * M + px];
    const float d = (dots[(0 * 16 * KT + ph) * M + px] + dots[(1 * 16 * KT + ph) * M + px]) +
                    (dots[(2 * 16 * KT + ph) * M + px] + dots[(3 * 16 * KT + ph) * M + px]);
    sims[(size_t)ph * N + row0 + px] = d / (float)sqrt(s);
  }
}

// Host: one workgroup of LANG_WAVES waves per LANG_M of N pixels with `lds` bytes of dynamic LDS.  More than 64 KiB has to be
// asked for first (a host-side attribute of the current device's function: no launch); that call's error is returned.
template <typename... P, typename... A>
static hipError_t dense_launch(void (*kernel)(P...), int N, size_t lds, hipStream_t st, A... args) {
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  kernel<<<(N + LANG_M - 1) / LANG_M, LANG_M * LANG_WAVES, lds, st>>>(args...);
  return hipSuccess;
}

}  // namespace olsr
