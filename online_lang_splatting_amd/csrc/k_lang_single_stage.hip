// k_lang_single_stage.hip — the single-stage language chain (language.single_stage_ae: True): one general autoencoder goes
// straight to the 15-channel code and back, there is no online autoencoder (include/olsr_single_stage.h).
//
//   ss_encoder_kernel     AutoencoderMLP.encode in eval() for 768 -> 384 -> 192 -> 96 -> 48 -> 24 -> 15, x / |x|
//                         (language/autoencoder/model.py:15-56, utils/slam_backend.py:556-576), shaped like k_lang_encoder.hip's
//                         lang_encoder_kernel: 64 pixels per workgroup of four waves, every product Y^T = W X^T of olsr_dense.h.
//     layer 1 (768 -> 384)  a wave owns 96 neurons for all 64 pixels: 24 accumulator tiles that stay in registers while the
//                         input passes through LDS in twelve chunks of 64 channels, [64 pixels][68] each, double-buffered.  The
//                         chunk is read from the channel-major map as it lies (no alignment assumed, the pixel tail guarded,
//                         nothing read past the end) or from rows; both fill the same LDS image, so both give the same bits.
//     layers 2 - 4        384 -> 192 -> 96 -> 48 out of one LDS image [64][516], in place (dense_layer).
//     the tail            48 -> 24 -> 15: the widths are no multiples of the 16-wide matrix tile, so these two layers run per
//                         pixel on the vector unit as fmaf chains that start from the bias and take k in ascending order (the
//                         way olsr_lang_ae_device.h does 32 -> 24 -> 15).  48 -> 24 is spread over the four waves, six neurons
//                         each for all 64 pixels (a neuron's chain is the same whoever computes it); 24 -> 15 and the norm are
//                         one lane per pixel.
//     BatchNorm + ReLU    five BatchNorm1d (384, 192, 96, 48, 24 channels) in the producing layer's epilogue:
//                         relu(fmaf(alpha, h, beta)), alpha and beta from bn_fold in double once per workgroup, kept in LDS;
//                         relu keeps a NaN, as torch's: a NaN input row is a NaN code row.
//     the norm            |h6|^2 in double in channel order, h6 / (float)sqrt, no epsilon (a zero row is NaN, as in the reference).
//   ss_query_sims_kernel  stage A of the text query for the decoder 15 -> 24 -> 48 -> 96 -> 192 -> 384 -> 384 -> 768
//                         (eval/evaluate_langslam.py:266-273, model.py:58-62), shaped like k_lang_query.hip's
//                         lang_query_sims_kernel: the codes (resampled to the decode size if asked) go through 15 -> 24 -> 48
//                         per pixel on the vector unit (decoder.0.weight [24,15] has no 16-byte aligned rows: scalar loads,
//                         bias-first k-ascending fmaf chains, twelve of the 48 neurons per wave), then 48 -> 96 -> 192 -> 384 ->
//                         384 out of the LDS image [64][516] with dense_layer, and the last layer in blocks of 64 neurons per
//                         wave that the K phrase products and the double norm consume as they arrive: the 768-wide row is never
//                         stored.  ReLU keeps a NaN (DENSE_EPI_RELU_NAN), as torch's does: a NaN code pixel gives NaN
//                         similarities for that pixel only (a pixel is a column of every product).  The two-stage stage A's
//                         fmaxf differs there and stays as it is.
// No atomics; a pixel's result depends on its own column of every product only, whatever else is in its tile.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_dense.h"

namespace olsr {

constexpr int SS_M = 64;       // pixels per workgroup
constexpr int SS_WAVES = 4;    // 256 threads
constexpr int SS_S = 516;      // LDS floats per pixel of the activation image (4 mod 64, as LE_S and LQ_S)
constexpr int SS_KC = 64;      // input channels per chunk of the encoder's layer 1
constexpr int SS_CS = SS_KC + 4;
constexpr int SS_FEAT = OLSR_LANG_QUERY_FEATURE_DIM, SS_C = OLSR_LANG_AE_CODE;

// ---- the encoder ----------------------------------------------------------------------------------------------------------

constexpr int SE_D0 = SS_FEAT, SE_D1 = 384, SE_D2 = 192, SE_D3 = 96, SE_D4 = 48, SE_D5 = 24, SE_D6 = SS_C;
constexpr int SE_CHUNKS = SE_D0 / SS_KC;
constexpr int SE_BN = SE_D1 + SE_D2 + SE_D3 + SE_D4 + SE_D5;  // BatchNorm channels: alpha[744] | beta[744] behind the image
// the flat array (state_dict order): Linear weight [out,in], bias [out]; BatchNorm weight, bias, running_mean, running_var
constexpr int SE_W1 = 0, SE_B1 = SE_W1 + SE_D1 * SE_D0, SE_N1 = SE_B1 + SE_D1;
constexpr int SE_W2 = SE_N1 + 4 * SE_D1, SE_B2 = SE_W2 + SE_D2 * SE_D1, SE_N2 = SE_B2 + SE_D2;
constexpr int SE_W3 = SE_N2 + 4 * SE_D2, SE_B3 = SE_W3 + SE_D3 * SE_D2, SE_N3 = SE_B3 + SE_D3;
constexpr int SE_W4 = SE_N3 + 4 * SE_D3, SE_B4 = SE_W4 + SE_D4 * SE_D3, SE_N4 = SE_B4 + SE_D4;
constexpr int SE_W5 = SE_N4 + 4 * SE_D4, SE_B5 = SE_W5 + SE_D5 * SE_D4, SE_N5 = SE_B5 + SE_D5;
constexpr int SE_W6 = SE_N5 + 4 * SE_D5, SE_B6 = SE_W6 + SE_D6 * SE_D5;
static_assert(SE_B6 + SE_D6 == OLSR_SS_ENCODER_PARAMS, "flat encoder layout");
static_assert(SE_B1 % 4 == 0 && SE_W2 % 4 == 0 && SE_B2 % 4 == 0 && SE_W3 % 4 == 0 && SE_B3 % 4 == 0 && SE_W4 % 4 == 0 &&
                  SE_B4 % 4 == 0 && SE_W5 % 4 == 0 && SE_B5 % 4 == 0 && SE_W6 % 4 == 0 && SE_B6 % 4 == 0,
              "every weight matrix and bias starts on a 16-byte boundary");
static_assert(2 * SS_M * SS_CS <= SS_M * SS_S, "both chunk buffers inside the activation image");
constexpr int SE_H5 = 64;  // where a pixel's 24 outputs of 48 -> 24 lie in its row of the image, clear of the 48 inputs
static_assert(SE_D4 <= SE_H5 && SE_H5 + SE_D5 <= SS_S && SE_D4 % SS_WAVES == 0 && SE_D5 % SS_WAVES == 0, "the tail's rows");
constexpr size_t SE_LDS_BYTES = ((size_t)SS_M * SS_S + 2 * SE_BN) * sizeof(float);
static_assert(SE_LDS_BYTES <= 160 * 1024, "one LDS image per workgroup");

// A thread's 16 elements of the chunk of channels k0 .. k0 + 63: element i is (pixel, channel) = (tid & 63, (tid >> 6) + 4 i)
// of the channel-major map, (channel, pixel) the other way round of rows; either way a wave's load is 64 consecutive floats.
template <bool CHANNELS>
__device__ __forceinline__ void se_fetch(const float* __restrict__ f, int N, long long plane_stride, int row0, int k0, int tid,
                                         float (&pre)[16]) {
  const int lo = tid & 63, hi = tid >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = CHANNELS ? lo : hi + 4 * i, c = CHANNELS ? hi + 4 * i : lo;
    const int row = row0 + p;
    float v = 0.f;
    if (row < N) v = CHANNELS ? f[(size_t)(k0 + c) * (size_t)plane_stride + row] : f[(size_t)row * SE_D0 + k0 + c];
    pre[i] = v;
  }
}
template <bool CHANNELS>
__device__ __forceinline__ void se_park(float* __restrict__ buf, int tid, const float (&pre)[16]) {
  const int lo = tid & 63, hi = tid >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = CHANNELS ? lo : hi + 4 * i, c = CHANNELS ? hi + 4 * i : lo;
    buf[p * SS_CS + c] = pre[i];
  }
}

// y[o] = b[o] + sum_k W[o][k] x[k] for OUT consecutive neurons, k ascending; uniform addresses (every lane reads the same
// parameter)
template <int OUT, int IN>
__device__ __forceinline__ void ss_linear(const float* __restrict__ W, const float* __restrict__ b, const float (&x)[IN],
                                          float (&y)[OUT]) {
#pragma unroll
  for (int o = 0; o < OUT; ++o) {
    float a = b[o];
#pragma unroll
    for (int i = 0; i < IN; ++i) a = fmaf(W[o * IN + i], x[i], a);
    y[o] = a;
  }
}

template <bool CHANNELS>
__global__ __launch_bounds__(SS_M * SS_WAVES) void ss_encoder_kernel(int N, long long plane_stride, double bn_eps,
                                                                      const float* __restrict__ features,
                                                                      const float* __restrict__ P, float* __restrict__ codes,
                                                                      int code_layout) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [64][SS_S] | alpha[744] | beta[744]
  float* alpha = X + SS_M * SS_S;
  float* beta = alpha + SE_BN;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * SS_M;
  constexpr int A1 = 0, A2 = SE_D1, A3 = A2 + SE_D2, A4 = A3 + SE_D3, A5 = A4 + SE_D4;  // a layer's channels inside alpha / beta

  float pre[16];
  se_fetch<CHANNELS>(features, N, plane_stride, row0, 0, tid, pre);
  for (int c = tid; c < SE_BN; c += SS_M * SS_WAVES) {
    if (c < A2) bn_fold(P + SE_N1, SE_D1, c - A1, bn_eps, alpha[c], beta[c]);
    else if (c < A3) bn_fold(P + SE_N2, SE_D2, c - A2, bn_eps, alpha[c], beta[c]);
    else if (c < A4) bn_fold(P + SE_N3, SE_D3, c - A3, bn_eps, alpha[c], beta[c]);
    else if (c < A5) bn_fold(P + SE_N4, SE_D4, c - A4, bn_eps, alpha[c], beta[c]);
    else bn_fold(P + SE_N5, SE_D5, c - A5, bn_eps, alpha[c], beta[c]);
  }
  se_park<CHANNELS>(X, tid, pre);
  __syncthreads();

  // layer 1: the 384 outputs stay in accumulators while the input's chunks pass through the two buffers
  {
    constexpr int NT = SE_D1 / (16 * SS_WAVES);
    static_assert(NT * 16 * SS_WAVES == SE_D1, "an equal share per wave");
    const int n0 = wave * NT * 16;
    f32x4 acc[NT][4];
    dense_bias<NT>(P + SE_B1, n0, q, acc);
    const float* wp = P + SE_W1 + (size_t)(n0 + li) * SE_D0 + 4 * q;
    f32x4 a[NT], an[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * 16 * SE_D0);
#pragma unroll 1
    for (int ch = 0; ch < SE_CHUNKS; ++ch) {
      const bool more = ch + 1 < SE_CHUNKS;
      if (more) se_fetch<CHANNELS>(features, N, plane_stride, row0, (ch + 1) * SS_KC, tid, pre);
      const float* xp = X + (ch & 1) * SS_M * SS_CS + li * SS_CS + 4 * q;
#pragma unroll
      for (int kb = 0; kb < SS_KC; kb += 16) {
        const int k0 = ch * SS_KC + kb;
        const int kn = k0 + 16 < SE_D0 ? k0 + 16 : k0;
#pragma unroll
        for (int t = 0; t < NT; ++t) an[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * 16 * SE_D0 + kn);
        dense_block<NT, SS_CS>(a, xp + kb, acc);
#pragma unroll
        for (int t = 0; t < NT; ++t) a[t] = an[t];
      }
      if (more) se_park<CHANNELS>(X + ((ch + 1) & 1) * SS_M * SS_CS, tid, pre);  // last read before the previous barrier
      __syncthreads();
    }
    // (every wave is past its last chunk read)
    dense_store<NT, SS_S, DENSE_EPI_BN_RELU>(X, alpha + A1, beta + A1, n0, li, q, acc);
    __syncthreads();
  }
  dense_layer<SE_D1, SE_D2, SS_WAVES, 4, SS_S, DENSE_EPI_BN_RELU>(X, P + SE_W2, P + SE_B2, alpha + A2, beta + A2, wave, li, q);
  dense_layer<SE_D2, SE_D3, SS_WAVES, 3, SS_S, DENSE_EPI_BN_RELU>(X, P + SE_W3, P + SE_B3, alpha + A3, beta + A3, wave, li, q);
  dense_layer<SE_D3, SE_D4, SS_WAVES, 3, SS_S, DENSE_EPI_BN_RELU>(X, P + SE_W4, P + SE_B4, alpha + A4, beta + A4, wave, li, q);

  // 48 -> 24: wave w computes neurons 6 w .. 6 w + 5 of pixel `lane`, each a bias-first k-ascending chain
  {
    constexpr int PER = SE_D5 / SS_WAVES;
    const int nb = __builtin_amdgcn_readfirstlane(wave) * PER;
    float* mine = X + lane * SS_S;
    float x[SE_D4], y[PER];
#pragma unroll
    for (int k4 = 0; k4 < SE_D4 / 4; ++k4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(mine + 4 * k4);
#pragma unroll
      for (int r = 0; r < 4; ++r) x[4 * k4 + r] = v[r];
    }
    ss_linear<PER, SE_D4>(P + SE_W5 + nb * SE_D4, P + SE_B5 + nb, x, y);
#pragma unroll
    for (int o = 0; o < PER; ++o) mine[SE_H5 + nb + o] = relu_keep_nan(fmaf(alpha[A5 + nb + o], y[o], beta[A5 + nb + o]));
  }
  __syncthreads();

  // one lane per pixel: 24 -> 15 and x / |x|
  const int row = row0 + tid;
  if (tid < SS_M && row < N) {
    const float* mine = X + tid * SS_S + SE_H5;
    float x[SE_D5], c[SE_D6];
#pragma unroll
    for (int k4 = 0; k4 < SE_D5 / 4; ++k4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(mine + 4 * k4);
#pragma unroll
      for (int r = 0; r < 4; ++r) x[4 * k4 + r] = v[r];
    }
    ss_linear<SE_D6, SE_D5>(P + SE_W6, P + SE_B6, x, c);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SE_D6; ++k) s = fma((double)c[k], (double)c[k], s);
    const float n = (float)sqrt(s);
#pragma unroll
    for (int k = 0; k < SE_D6; ++k) {
      const float u = c[k] / n;
      if (code_layout == OLSR_LANG_AE_CODES_CHANNELS) codes[(size_t)k * N + row] = u;
      else codes[(size_t)row * SE_D6 + k] = u;
    }
  }
}

// ---- stage A of the text query --------------------------------------------------------------------------------------------

constexpr int SQ_D0 = SS_C, SQ_D1 = 24, SQ_D2 = 48, SQ_D3 = 96, SQ_D4 = 192, SQ_D5 = 384, SQ_D6 = 384, SQ_D7 = SS_FEAT;
// the decoder's layers in the flat array (state_dict order: weight [out,in], bias [out] per layer)
constexpr int SQ_W1 = 0, SQ_B1 = SQ_W1 + SQ_D1 * SQ_D0, SQ_W2 = SQ_B1 + SQ_D1, SQ_B2 = SQ_W2 + SQ_D2 * SQ_D1,
              SQ_W3 = SQ_B2 + SQ_D2, SQ_B3 = SQ_W3 + SQ_D3 * SQ_D2, SQ_W4 = SQ_B3 + SQ_D3, SQ_B4 = SQ_W4 + SQ_D4 * SQ_D3,
              SQ_W5 = SQ_B4 + SQ_D4, SQ_B5 = SQ_W5 + SQ_D5 * SQ_D4, SQ_W6 = SQ_B5 + SQ_D5, SQ_B6 = SQ_W6 + SQ_D6 * SQ_D5,
              SQ_W7 = SQ_B6 + SQ_D6, SQ_B7 = SQ_W7 + SQ_D7 * SQ_D6;
static_assert(SQ_B7 + SQ_D7 == OLSR_SS_DECODER_PARAMS, "flat decoder layout");
static_assert(SQ_W3 % 4 == 0 && SQ_B3 % 4 == 0 && SQ_W4 % 4 == 0 && SQ_B4 % 4 == 0 && SQ_W5 % 4 == 0 && SQ_B5 % 4 == 0 &&
                  SQ_W6 % 4 == 0 && SQ_B6 % 4 == 0 && SQ_W7 % 4 == 0 && SQ_B7 % 4 == 0,
              "16-byte loads of every weight and bias of the matrix layers");

// F.interpolate(mode="bilinear", align_corners=False) along one axis: the two taps and their weights (ATen UpSample.h:
// area_pixel_compute_source_index and guard_index_and_lambda, in float as for a float32 tensor); k_lang_query.hip's lq_taps
struct SsTaps {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ SsTaps ss_taps(int dst, int in_size, float scale) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  SsTaps t;
  t.i0 = min((int)src, in_size - 1);
  t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
  t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
  t.l0 = 1.f - t.l1;
  return t;
}
__device__ __forceinline__ float ss_sample(const float* __restrict__ plane, int w, const SsTaps& ty, const SsTaps& tx) {
  const float* r0 = plane + (size_t)ty.i0 * w;
  const float* r1 = plane + (size_t)ty.i1 * w;
  return ty.l0 * (tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1]) + ty.l1 * (tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1]);
}

struct SsGeom {
  int in_w, in_h, dec_w, dec_h;
  int resample_codes;
  float code_sx, code_sy;
};

// one hidden layer in place: X[64][KIN] -> relu(W X^T + b)^T = X[64][NOUT], the first WUSED waves share the neurons
template <int KIN, int NOUT, int WUSED>
__device__ __forceinline__ void sq_hidden(float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                          int wave, int li, int q) {
  dense_layer<KIN, NOUT, SS_WAVES, WUSED, SS_S, DENSE_EPI_RELU_NAN>(X, W, bias, nullptr, nullptr, wave, li, q);
}

// KT: 16-row tiles of phrases (K <= 16 KT)
template <int KT>
__global__ __launch_bounds__(SS_M * SS_WAVES) void ss_query_sims_kernel(int N, SsGeom g, int K, const float* __restrict__ codes,
                                                                         const float* __restrict__ dec,
                                                                         const float* __restrict__ phrases,
                                                                         float* __restrict__ sims) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [64][SS_S]; afterwards the waves' partial dots and norms
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * SS_M;
  // the pixel's codes (resampled to the decode size if asked) -> 15 -> 24 -> 48; wave w keeps neurons 12 w .. 12 w + 11 of the
  // 48 (the 24 are computed by each of the four: a neuron's chain is the same whoever computes it) -> X[pixel][0..47]
  {
    constexpr int PER = SQ_D2 / SS_WAVES;
    const int nb = __builtin_amdgcn_readfirstlane(wave) * PER;
    const int row = row0 + lane;
    float h2[PER];
    if (row < N) {
      float c[SQ_D0], h1[SQ_D1];
      if (g.resample_codes) {
        const int oy = row / g.dec_w, ox = row - oy * g.dec_w;
        const SsTaps ty = ss_taps(oy, g.in_h, g.code_sy), tx = ss_taps(ox, g.in_w, g.code_sx);
#pragma unroll
        for (int k = 0; k < SQ_D0; ++k) c[k] = ss_sample(codes + (size_t)k * g.in_w * g.in_h, g.in_w, ty, tx);
      } else {
#pragma unroll
        for (int k = 0; k < SQ_D0; ++k) c[k] = codes[(size_t)k * N + row];
      }
      ss_linear<SQ_D1, SQ_D0>(dec + SQ_W1, dec + SQ_B1, c, h1);
#pragma unroll
      for (int k = 0; k < SQ_D1; ++k) h1[k] = relu_keep_nan(h1[k]);
      ss_linear<PER, SQ_D1>(dec + SQ_W2 + nb * SQ_D1, dec + SQ_B2 + nb, h1, h2);
#pragma unroll
      for (int k = 0; k < PER; ++k) h2[k] = relu_keep_nan(h2[k]);
    } else {
#pragma unroll
      for (int k = 0; k < PER; ++k) h2[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) X[lane * SS_S + nb + k] = h2[k];
  }
  __syncthreads();
  sq_hidden<SQ_D2, SQ_D3, 3>(X, dec + SQ_W3, dec + SQ_B3, wave, li, q);
  sq_hidden<SQ_D3, SQ_D4, 4>(X, dec + SQ_W4, dec + SQ_B4, wave, li, q);
  sq_hidden<SQ_D4, SQ_D5, 4>(X, dec + SQ_W5, dec + SQ_B5, wave, li, q);
  sq_hidden<SQ_D5, SQ_D6, 4>(X, dec + SQ_W6, dec + SQ_B6, wave, li, q);
  // the last layer in blocks of 4 x 16 neurons per wave, consumed as they arrive (lang_query_sims_kernel's tail)
  constexpr int NT = 4, CHUNKS = SQ_D7 / (16 * NT * SS_WAVES);
  static_assert(CHUNKS * 16 * NT * SS_WAVES == SQ_D7, "blocks of 64 neurons per wave");
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
    dense_gemm<SQ_D6, NT, SS_S>(X, dec + SQ_W7, dec + SQ_B7, n0, li, q, acc);
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
        if (ph < K) pf = *reinterpret_cast<const f32x4*>(phrases + (size_t)ph * SS_FEAT + n0 + 16 * t + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
            sacc[kt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf[r], acc[t][pt][r], sacc[kt][pt], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the activations are no longer read
  float* dots = X;                                                           // [wave][16 KT phrases][64 pixels]
  double* norms = reinterpret_cast<double*>(X + SS_WAVES * 16 * KT * SS_M);  // [wave][q][64 pixels]
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    norms[(wave * 4 + q) * SS_M + pt * 16 + li] = nrm[pt];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) dots[(wave * 16 * KT + kt * 16 + 4 * q + r) * SS_M + pt * 16 + li] = sacc[kt][pt][r];
  }
  __syncthreads();
  for (int e = tid; e < K * SS_M; e += SS_M * SS_WAVES) {
    const int ph = e / SS_M, px = e - ph * SS_M;
    if (row0 + px >= N) continue;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SS_WAVES * 4; ++k) s += norms[k * SS_M + px];
    const float d = (dots[(0 * 16 * KT + ph) * SS_M + px] + dots[(1 * 16 * KT + ph) * SS_M + px]) +
                    (dots[(2 * 16 * KT + ph) * SS_M + px] + dots[(3 * 16 * KT + ph) * SS_M + px]);
    sims[(size_t)ph * N + row0 + px] = d / (float)sqrt(s);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

template <bool CHANNELS>
static hipError_t se_launch(const olsr_ss_encoder_params& p, int N, const float* features, const float* params, float* codes,
                            hipStream_t st) {
  // more than 64 KiB of dynamic LDS has to be asked for (a host-side attribute of the current device's function: no launch)
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ss_encoder_kernel<CHANNELS>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)SE_LDS_BYTES);
  if (e != hipSuccess) return e;
  ss_encoder_kernel<CHANNELS><<<(N + SS_M - 1) / SS_M, SS_M * SS_WAVES, SE_LDS_BYTES, st>>>(
      N, (long long)p.plane_stride, p.bn_eps, features, params, codes, p.code_layout);
  return hipSuccess;
}

hipError_t launch_ss_encoder(const olsr_ss_encoder_params& p, int N, const float* features, const float* params, float* codes,
                             hipStream_t st) {
  if (p.in_layout == OLSR_LANG_ENCODER_IN_CHANNELS) return se_launch<true>(p, N, features, params, codes, st);
  return se_launch<false>(p, N, features, params, codes, st);
}

template <int KT>
static hipError_t sq_launch(int N, const SsGeom& g, int K, const float* codes, const float* dec, const float* phrases,
                            float* sims, hipStream_t st) {
  constexpr size_t act = (size_t)SS_M * SS_S * sizeof(float);
  constexpr size_t red = (size_t)SS_WAVES * 16 * KT * SS_M * sizeof(float) + (size_t)SS_WAVES * 4 * SS_M * sizeof(double);
  static_assert(red <= act && act <= 160 * 1024, "one LDS image per workgroup");
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ss_query_sims_kernel<KT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)act);
  if (e != hipSuccess) return e;
  ss_query_sims_kernel<KT><<<(N + SS_M - 1) / SS_M, SS_M * SS_WAVES, act, st>>>(N, g, K, codes, dec, phrases, sims);
  return hipSuccess;
}

hipError_t launch_ss_query_sims(const olsr_lang_query_params& p, const float* codes, const float* dec, const float* phrases,
                                float* sims, hipStream_t st) {
  SsGeom g{};
  g.in_w = p.in_width, g.in_h = p.in_height, g.dec_w = p.dec_width, g.dec_h = p.dec_height;
  g.resample_codes = (g.in_w != g.dec_w || g.in_h != g.dec_h) ? 1 : 0;
  g.code_sx = (float)g.in_w / (float)g.dec_w, g.code_sy = (float)g.in_h / (float)g.dec_h;
  const int N = p.dec_width * p.dec_height;
  if (p.K <= 16) return sq_launch<1>(N, g, p.K, codes, dec, phrases, sims, st);
  if (p.K <= 32) return sq_launch<2>(N, g, p.K, codes, dec, phrases, sims, st);
  return sq_launch<4>(N, g, p.K, codes, dec, phrases, sims, st);
}

}  // namespace olsr
