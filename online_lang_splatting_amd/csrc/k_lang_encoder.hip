// k_lang_encoder.hip — the general language encoder 768 -> 512 -> 256 -> 128 -> 64 -> 32, x / |x|.
//
// The reference turns a keyframe's high-resolution CLIP map [1,768,h,w] into the 32-wide rows the online autoencoder trains on
// with clip.permute(0,2,3,1).view(-1,768) and AutoencoderMLP.encode (language/autoencoder/model.py:15-56, in eval(), so every
// BatchNorm1d is its running statistics): five GEMMs, four BatchNorm, four ReLU and a norm in torch ops, a permuted copy of the
// input and every intermediate written and read again.  Here one kernel on olsr_dense.h, as k_lang_query.hip's stage A:
//   lang_encoder_kernel   64 pixels per workgroup of four waves, every product Y^T = W X^T on v_mfma_f32_16x16x4_f32 with the
//                         weights straight from global memory / L2 (every weight read by exactly one wave of the workgroup)
//                         and the activations out of LDS.
//     layer 1 (768 -> 512)  a wave owns 128 neurons for all 64 pixels: 32 accumulator tiles that stay in registers while the
//                         input passes through LDS in twelve chunks of 64 channels, [64 pixels][68] each, double-buffered: the
//                         next chunk's global loads are issued before the current chunk's MFMAs and stored behind them.  The
//                         chunk is read from the channel-major map as it lies (64 consecutive pixels of a plane per wave and
//                         load: no alignment is assumed, the pixel tail is guarded, nothing is read past the end) or from rows;
//                         both fill the same LDS image, so both give the same bits.  The two chunk buffers lie inside the
//                         activation image, which is not in use before layer 1 has finished.
//     layers 2 - 5        out of one LDS image [64][516], in place (dense_layer): a wave keeps its share of the layer's neurons
//                         in accumulators until every wave has read the layer's input.
//     BatchNorm + ReLU    in the producing layer's epilogue: relu(fmaf(alpha, h, beta)) with alpha = weight / sqrt(var + eps),
//                         beta = bias - mean alpha per channel, computed in double once per workgroup, rounded once, kept in LDS.
//                         relu is fmaxf(., 0) with a NaN kept, as torch's: a NaN input row is a NaN output row.
//     the norm            one lane per pixel: |h5|^2 in double in channel order, h5 / (float)sqrt, no epsilon (a zero row is NaN,
//                         as in the reference).  The unit rows leave through LDS as one contiguous block.
//     the online encoder  optional, the same lane: ae_encode (olsr_lang_ae_device.h), what lang_ae_encode_kernel calls, on the
//                         unit row, so the codes equal olsr_lang_ae_encode of the stored features bit for bit.
// No atomics; a pixel's result depends on its own column of every product only, whatever else is in its tile.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_dense.h"
#include "olsr_lang_ae_device.h"

namespace olsr {

constexpr int LE_M = 64;      // pixels per workgroup
constexpr int LE_WAVES = 4;   // 256 threads
constexpr int LE_S = 516;     // LDS floats per pixel of the activation image: 512 + 4, as LQ_S
constexpr int LE_KC = 64;     // input channels per layer-1 chunk
constexpr int LE_CS = LE_KC + 4;  // LDS floats per pixel of a chunk (68 = 4 mod 64: the float4 reads of 16 pixels hit 64 banks)
constexpr int LE_D0 = 768, LE_D1 = 512, LE_D2 = 256, LE_D3 = 128, LE_D4 = 64, LE_D5 = OLSR_LANG_AE_IN;
constexpr int LE_CHUNKS = LE_D0 / LE_KC;
constexpr int LE_BN = LE_D1 + LE_D2 + LE_D3 + LE_D4;  // BatchNorm channels: alpha[960] | beta[960] behind the image
// the flat array (state_dict order): Linear weight [out,in], bias [out]; BatchNorm weight, bias, running_mean, running_var
constexpr int LE_W1 = 0, LE_B1 = LE_W1 + LE_D1 * LE_D0, LE_N1 = LE_B1 + LE_D1;
constexpr int LE_W2 = LE_N1 + 4 * LE_D1, LE_B2 = LE_W2 + LE_D2 * LE_D1, LE_N2 = LE_B2 + LE_D2;
constexpr int LE_W3 = LE_N2 + 4 * LE_D2, LE_B3 = LE_W3 + LE_D3 * LE_D2, LE_N3 = LE_B3 + LE_D3;
constexpr int LE_W4 = LE_N3 + 4 * LE_D3, LE_B4 = LE_W4 + LE_D4 * LE_D3, LE_N4 = LE_B4 + LE_D4;
constexpr int LE_W5 = LE_N4 + 4 * LE_D4, LE_B5 = LE_W5 + LE_D5 * LE_D4;
static_assert(LE_B5 + LE_D5 == OLSR_LANG_ENCODER_PARAMS, "flat encoder layout");
static_assert(LE_N1 % 4 == 0 && LE_W2 % 4 == 0 && LE_W3 % 4 == 0 && LE_W4 % 4 == 0 && LE_W5 % 4 == 0 && LE_B5 % 4 == 0,
              "16-byte loads of every weight and bias");
static_assert(2 * LE_M * LE_CS <= LE_M * LE_S, "both chunk buffers inside the activation image");
constexpr size_t LE_LDS_BYTES = ((size_t)LE_M * LE_S + 2 * LE_BN) * sizeof(float);
static_assert(LE_LDS_BYTES <= 160 * 1024, "one LDS image per workgroup");

// one layer out of the activation image, in place; the first WUSED waves share the neurons
template <int KIN, int NOUT, int WUSED, int EPI>
__device__ __forceinline__ void le_layer(float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                         const float* __restrict__ alpha, const float* __restrict__ beta, int wave, int li,
                                         int q) {
  dense_layer<KIN, NOUT, LE_WAVES, WUSED, LE_S, EPI>(X, W, bias, alpha, beta, wave, li, q);
}

// A thread's 16 elements of the chunk of channels k0 .. k0 + 63: element i is (pixel, channel) = (tid & 63, (tid >> 6) + 4 i)
// of the channel-major map, (channel, pixel) the other way round of rows; either way a wave's load is 64 consecutive floats.
template <bool CHANNELS>
__device__ __forceinline__ void le_fetch(const float* __restrict__ f, int N, long long plane_stride, int row0, int k0, int tid,
                                         float (&pre)[16]) {
  const int lo = tid & 63, hi = tid >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = CHANNELS ? lo : hi + 4 * i, c = CHANNELS ? hi + 4 * i : lo;
    const int row = row0 + p;
    float v = 0.f;
    if (row < N) v = CHANNELS ? f[(size_t)(k0 + c) * (size_t)plane_stride + row] : f[(size_t)row * LE_D0 + k0 + c];
    pre[i] = v;
  }
}
template <bool CHANNELS>
__device__ __forceinline__ void le_park(float* __restrict__ buf, int tid, const float (&pre)[16]) {
  const int lo = tid & 63, hi = tid >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = CHANNELS ? lo : hi + 4 * i, c = CHANNELS ? hi + 4 * i : lo;
    buf[p * LE_CS + c] = pre[i];
  }
}

template <bool CHANNELS>
__global__ __launch_bounds__(LE_M * LE_WAVES) void lang_encoder_kernel(int N, long long plane_stride, double bn_eps,
                                                                        const float* __restrict__ features,
                                                                        const float* __restrict__ P,
                                                                        const float* __restrict__ online,
                                                                        float* __restrict__ features32,
                                                                        float* __restrict__ codes, int code_layout) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [64][LE_S] | alpha[960] | beta[960]
  float* alpha = X + LE_M * LE_S;
  float* beta = alpha + LE_BN;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * LE_M;
  constexpr int A1 = 0, A2 = LE_D1, A3 = A2 + LE_D2, A4 = A3 + LE_D3;  // a layer's channels inside alpha / beta

  float pre[16];
  le_fetch<CHANNELS>(features, N, plane_stride, row0, 0, tid, pre);
  for (int c = tid; c < LE_BN; c += LE_M * LE_WAVES) {
    if (c < A2) bn_fold(P + LE_N1, LE_D1, c - A1, bn_eps, alpha[c], beta[c]);
    else if (c < A3) bn_fold(P + LE_N2, LE_D2, c - A2, bn_eps, alpha[c], beta[c]);
    else if (c < A4) bn_fold(P + LE_N3, LE_D3, c - A3, bn_eps, alpha[c], beta[c]);
    else bn_fold(P + LE_N4, LE_D4, c - A4, bn_eps, alpha[c], beta[c]);
  }
  le_park<CHANNELS>(X, tid, pre);
  __syncthreads();

  // layer 1: the 512 outputs stay in accumulators while the input's chunks pass through the two buffers
  {
    constexpr int NT = LE_D1 / (16 * LE_WAVES);
    const int n0 = wave * NT * 16;
    f32x4 acc[NT][4];
    dense_bias<NT>(P + LE_B1, n0, q, acc);
    const float* wp = P + LE_W1 + (size_t)(n0 + li) * LE_D0 + 4 * q;
    f32x4 a[NT], an[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) a[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * 16 * LE_D0);
#pragma unroll 1
    for (int ch = 0; ch < LE_CHUNKS; ++ch) {
      const bool more = ch + 1 < LE_CHUNKS;
      if (more) le_fetch<CHANNELS>(features, N, plane_stride, row0, (ch + 1) * LE_KC, tid, pre);
      const float* xp = X + (ch & 1) * LE_M * LE_CS + li * LE_CS + 4 * q;
#pragma unroll
      for (int kb = 0; kb < LE_KC; kb += 16) {
        const int k0 = ch * LE_KC + kb;
        const int kn = k0 + 16 < LE_D0 ? k0 + 16 : k0;
#pragma unroll
        for (int t = 0; t < NT; ++t) an[t] = *reinterpret_cast<const f32x4*>(wp + (size_t)t * 16 * LE_D0 + kn);
        dense_block<NT, LE_CS>(a, xp + kb, acc);
#pragma unroll
        for (int t = 0; t < NT; ++t) a[t] = an[t];
      }
      if (more) le_park<CHANNELS>(X + ((ch + 1) & 1) * LE_M * LE_CS, tid, pre);  // last read before the previous barrier
      __syncthreads();
    }
    // (every wave is past its last chunk read)
    dense_store<NT, LE_S, DENSE_EPI_BN_RELU>(X, alpha + A1, beta + A1, n0, li, q, acc);
    __syncthreads();
  }
  le_layer<LE_D1, LE_D2, 4, DENSE_EPI_BN_RELU>(X, P + LE_W2, P + LE_B2, alpha + A2, beta + A2, wave, li, q);
  le_layer<LE_D2, LE_D3, 4, DENSE_EPI_BN_RELU>(X, P + LE_W3, P + LE_B3, alpha + A3, beta + A3, wave, li, q);
  le_layer<LE_D3, LE_D4, 4, DENSE_EPI_BN_RELU>(X, P + LE_W4, P + LE_B4, alpha + A4, beta + A4, wave, li, q);
  le_layer<LE_D4, LE_D5, 2, DENSE_EPI_NONE>(X, P + LE_W5, P + LE_B5, nullptr, nullptr, wave, li, q);

  // one lane per pixel: x / |x|, and the online encoder on the unit row
  if (tid < LE_M) {
    float* mine = X + tid * LE_S;
    float u[LE_D5];
    double s = 0.0;
#pragma unroll
    for (int k4 = 0; k4 < LE_D5 / 4; ++k4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(mine + 4 * k4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        u[4 * k4 + r] = v[r];
        s = fma((double)v[r], (double)v[r], s);
      }
    }
    const float n = (float)sqrt(s);
#pragma unroll
    for (int k = 0; k < LE_D5; ++k) u[k] = u[k] / n;
#pragma unroll
    for (int k4 = 0; k4 < LE_D5 / 4; ++k4)
      *reinterpret_cast<f32x4*>(mine + 4 * k4) = f32x4{u[4 * k4], u[4 * k4 + 1], u[4 * k4 + 2], u[4 * k4 + 3]};
    const int row = row0 + tid;
    if (codes != nullptr && row < N) {
      float h1[AE_H], c[AE_C];
      ae_encode(online, u, h1, c);
      ae_store_codes(codes, code_layout, N, row, c);
    }
  }
  if (features32 == nullptr) return;
  __syncthreads();
  // the tile's rows are one contiguous block of the output
  float* dst = features32 + (size_t)row0 * LE_D5;
#pragma unroll
  for (int i = 0; i < LE_M * LE_D5 / (LE_M * LE_WAVES); ++i) {
    const int e = tid + i * LE_M * LE_WAVES, p = e / LE_D5, k = e - p * LE_D5;
    if (row0 + p < N) dst[e] = X[p * LE_S + k];
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

template <bool CHANNELS>
static hipError_t le_launch(const olsr_lang_encoder_params& p, int N, const float* features, const float* params,
                            const float* online, float* features32, float* codes, hipStream_t st) {
  // more than 64 KiB of dynamic LDS has to be asked for (a host-side attribute of the current device's function: no launch)
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lang_encoder_kernel<CHANNELS>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)LE_LDS_BYTES);
  if (e != hipSuccess) return e;
  lang_encoder_kernel<CHANNELS><<<(N + LE_M - 1) / LE_M, LE_M * LE_WAVES, LE_LDS_BYTES, st>>>(
      N, (long long)p.plane_stride, p.bn_eps, features, params, online, features32, codes, p.code_layout);
  return hipSuccess;
}

hipError_t launch_lang_encoder(const olsr_lang_encoder_params& p, int N, const float* features, const float* params,
                               const float* online, float* features32, float* codes, hipStream_t st) {
  if (p.in_layout == OLSR_LANG_ENCODER_IN_CHANNELS) return le_launch<true>(p, N, features, params, online, features32, codes, st);
  return le_launch<false>(p, N, features, params, online, features32, codes, st);
}

}  // namespace olsr
