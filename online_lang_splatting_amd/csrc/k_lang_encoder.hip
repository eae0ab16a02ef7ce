// k_lang_encoder.hip — the language encoders: the general one 768 -> 512 -> 256 -> 128 -> 64 -> 32, x / |x|, and the
// single-stage chain's 768 -> 384 -> 192 -> 96 -> 48 -> 24 -> 15, x / |x| (language.single_stage_ae: True, where one general
// autoencoder goes straight to the 15-channel code and there is no online autoencoder; include/olsr_single_stage.h).
//
// The reference turns a keyframe's high-resolution CLIP map [1,768,h,w] into the rows the next stage works on with
// clip.permute(0,2,3,1).view(-1,768) and AutoencoderMLP.encode (language/autoencoder/model.py:15-56, utils/slam_backend.py:
// 556-576, in eval(), so every BatchNorm1d is its running statistics): the GEMMs, BatchNorms, ReLUs and a norm in torch ops, a
// permuted copy of the input and every intermediate written and read again.  Here one kernel per net on olsr_dense.h, as
// k_lang_query.hip's stage A; the two differ in their width lists and in what follows the matrix layers.
//   both                  64 pixels per workgroup of four waves, every product Y^T = W X^T on v_mfma_f32_16x16x4_f32 with the
//                         weights straight from global memory / L2 (every weight read by exactly one wave of the workgroup)
//                         and the activations out of LDS.
//     layer 1             dense_streamed_layer: a wave owns a quarter of the neurons (128 of 512, 96 of 384) for all 64 pixels
//                         in accumulators while the input passes through LDS in twelve chunks of 64 channels, read from the
//                         channel-major map as it lies or from rows.
//     the matrix layers   out of one LDS image [64][516], in place (dense_layer): a wave keeps its share of the layer's neurons
//                         in accumulators until every wave has read the layer's input.
//     BatchNorm + ReLU    in the producing layer's epilogue: relu(fmaf(alpha, h, beta)) with alpha = weight / sqrt(var + eps),
//                         beta = bias - mean alpha per channel, computed in double once per workgroup, rounded once, kept in LDS
//                         (bn_fold_table).  relu is fmaxf(., 0) with a NaN kept, as torch's: a NaN input row is a NaN output row.
//     the norm            one lane per pixel: |h|^2 in double in channel order, h / (float)sqrt, no epsilon (a zero row is NaN,
//                         as in the reference).
//   lang_encoder_kernel   layers 2 - 5 are matrix layers.  The unit rows leave through LDS as one contiguous block.
//     the online encoder  optional, the norm's lane: ae_encode (olsr_lang_ae_device.h), what lang_ae_encode_kernel calls, on the
//                         unit row, so the codes equal olsr_lang_ae_encode of the stored features bit for bit.
//   ss_encoder_kernel     layers 2 - 4 (down to 48) are matrix layers.
//     the tail            48 -> 24 -> 15: the widths are no multiples of the 16-wide matrix tile, so these two layers run per
//                         pixel on the vector unit as fmaf chains that start from the bias and take k in ascending order
//                         (lane_linear, the way olsr_lang_ae_device.h does 32 -> 24 -> 15).  48 -> 24 is spread over the four
//                         waves, six neurons each for all 64 pixels (a neuron's chain is the same whoever computes it), with the
//                         fifth BatchNorm + ReLU; 24 -> 15 and the norm are one lane per pixel.
// No atomics; a pixel's result depends on its own column of every product only, whatever else is in its tile.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_dense.h"
#include "olsr_lang_ae_device.h"

namespace olsr {

// the flat arrays (state_dict order): Linear weight [out,in], bias [out]; BatchNorm weight, bias, running_mean, running_var
constexpr int LE_D[] = {OLSR_LANG_QUERY_FEATURE_DIM, 512, 256, 128, 64, OLSR_LANG_AE_IN};
constexpr int SE_D[] = {OLSR_LANG_QUERY_FEATURE_DIM, 384, 192, 96, 48, 24, OLSR_LANG_AE_CODE};
constexpr auto LE = flat_mlp(LE_D, true);
constexpr auto SE = flat_mlp(SE_D, true);
static_assert(LE.total == OLSR_LANG_ENCODER_PARAMS, "flat encoder layout");
static_assert(SE.total == OLSR_SS_ENCODER_PARAMS, "flat encoder layout");
static_assert(flat_mlp_aligned(LE) && flat_mlp_aligned(SE), "every weight matrix and bias starts on a 16-byte boundary");
// the image, and alpha | beta of every BatchNorm channel (960, 744) behind it
constexpr size_t LE_LDS_BYTES = LANG_ACT_BYTES + 2 * LE.bn_channels * sizeof(float);
constexpr size_t SE_LDS_BYTES = LANG_ACT_BYTES + 2 * SE.bn_channels * sizeof(float);
static_assert(LE_LDS_BYTES <= 160 * 1024 && SE_LDS_BYTES <= 160 * 1024, "one LDS image per workgroup");
constexpr int SE_H5 = 64;  // where a pixel's 24 outputs of 48 -> 24 lie in its row of the image, clear of the 48 inputs
static_assert(SE.d[4] <= SE_H5 && SE_H5 + SE.d[5] <= LANG_S && SE.d[4] % 4 == 0 && SE.d[5] % LANG_WAVES == 0, "the tail's rows");

// layer I (from 0) of the encoder E out of the activation image, in place; the first WUSED waves share the neurons
template <const auto& E, int I, int WUSED, int EPI = DENSE_EPI_BN_RELU>
__device__ __forceinline__ void enc_layer(float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ alpha,
                                          const float* __restrict__ beta, int wave, int li, int q) {
  dense_layer<E.d[I], E.d[I + 1], LANG_WAVES, WUSED, LANG_S, EPI>(X, P + E.w[I], P + E.b[I], alpha + E.a[I], beta + E.a[I], wave,
                                                                  li, q);
}

template <bool CHANNELS>
__global__ __launch_bounds__(LANG_M * LANG_WAVES) void lang_encoder_kernel(int N, long long plane_stride, double bn_eps,
                                                                            const float* __restrict__ features,
                                                                            const float* __restrict__ P,
                                                                            const float* __restrict__ online,
                                                                            float* __restrict__ features32,
                                                                            float* __restrict__ codes, int code_layout) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [64][LANG_S] | alpha[960] | beta[960]
  float* alpha = X + LANG_M * LANG_S;
  float* beta = alpha + LE.bn_channels;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * LANG_M;
  constexpr int D0 = LE.d[0], D1 = LE.d[1], D5 = LE.d[5];

  float pre[16];
  dense_chunk_fetch<CHANNELS, D0>(features, N, plane_stride, row0, 0, tid, pre);
  bn_fold_table(P, LE, bn_eps, alpha, beta, tid, LANG_M * LANG_WAVES);
  dense_streamed_layer<CHANNELS, D0, D1, LANG_WAVES, LANG_KC, LANG_S, DENSE_EPI_BN_RELU>(
      X, features, N, plane_stride, row0, P + LE.w[0], P + LE.b[0], alpha + LE.a[0], beta + LE.a[0], wave, li, q, tid, pre);
  enc_layer<LE, 1, 4>(X, P, alpha, beta, wave, li, q);
  enc_layer<LE, 2, 4>(X, P, alpha, beta, wave, li, q);
  enc_layer<LE, 3, 4>(X, P, alpha, beta, wave, li, q);
  enc_layer<LE, 4, 2, DENSE_EPI_NONE>(X, P, alpha, beta, wave, li, q);

  // one lane per pixel: x / |x|, and the online encoder on the unit row
  if (tid < LANG_M) {
    float* mine = X + tid * LANG_S;
    float u[D5];
    double s = 0.0;
#pragma unroll
    for (int k4 = 0; k4 < D5 / 4; ++k4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(mine + 4 * k4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        u[4 * k4 + r] = v[r];
        s = fma((double)v[r], (double)v[r], s);
      }
    }
    const float n = (float)sqrt(s);
#pragma unroll
    for (int k = 0; k < D5; ++k) u[k] = u[k] / n;
#pragma unroll
    for (int k4 = 0; k4 < D5 / 4; ++k4)
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
  float* dst = features32 + (size_t)row0 * D5;
#pragma unroll
  for (int i = 0; i < LANG_M * D5 / (LANG_M * LANG_WAVES); ++i) {
    const int e = tid + i * LANG_M * LANG_WAVES, p = e / D5, k = e - p * D5;
    if (row0 + p < N) dst[e] = X[p * LANG_S + k];
  }
}

template <bool CHANNELS>
__global__ __launch_bounds__(LANG_M * LANG_WAVES) void ss_encoder_kernel(int N, long long plane_stride, double bn_eps,
                                                                          const float* __restrict__ features,
                                                                          const float* __restrict__ P, float* __restrict__ codes,
                                                                          int code_layout) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [64][LANG_S] | alpha[744] | beta[744]
  float* alpha = X + LANG_M * LANG_S;
  float* beta = alpha + SE.bn_channels;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * LANG_M;
  constexpr int D0 = SE.d[0], D1 = SE.d[1], D4 = SE.d[4], D5 = SE.d[5], D6 = SE.d[6];

  float pre[16];
  dense_chunk_fetch<CHANNELS, D0>(features, N, plane_stride, row0, 0, tid, pre);
  bn_fold_table(P, SE, bn_eps, alpha, beta, tid, LANG_M * LANG_WAVES);
  dense_streamed_layer<CHANNELS, D0, D1, LANG_WAVES, LANG_KC, LANG_S, DENSE_EPI_BN_RELU>(
      X, features, N, plane_stride, row0, P + SE.w[0], P + SE.b[0], alpha + SE.a[0], beta + SE.a[0], wave, li, q, tid, pre);
  enc_layer<SE, 1, 4>(X, P, alpha, beta, wave, li, q);
  enc_layer<SE, 2, 3>(X, P, alpha, beta, wave, li, q);
  enc_layer<SE, 3, 3>(X, P, alpha, beta, wave, li, q);

  // 48 -> 24: wave w computes neurons 6 w .. 6 w + 5 of pixel `lane`, each a bias-first k-ascending chain
  {
    constexpr int PER = D5 / LANG_WAVES;
    const int nb = __builtin_amdgcn_readfirstlane(wave) * PER;
    float* mine = X + lane * LANG_S;
    float x[D4], y[PER];
#pragma unroll
    for (int k4 = 0; k4 < D4 / 4; ++k4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(mine + 4 * k4);
#pragma unroll
      for (int r = 0; r < 4; ++r) x[4 * k4 + r] = v[r];
    }
    lane_linear<PER, D4>(P + SE.w[4] + nb * D4, P + SE.b[4] + nb, x, y);
#pragma unroll
    for (int o = 0; o < PER; ++o)
      mine[SE_H5 + nb + o] = relu_keep_nan(fmaf(alpha[SE.a[4] + nb + o], y[o], beta[SE.a[4] + nb + o]));
  }
  __syncthreads();

  // one lane per pixel: 24 -> 15 and x / |x|
  const int row = row0 + tid;
  if (tid < LANG_M && row < N) {
    const float* mine = X + tid * LANG_S + SE_H5;
    float x[D5], c[D6];
#pragma unroll
    for (int k4 = 0; k4 < D5 / 4; ++k4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(mine + 4 * k4);
#pragma unroll
      for (int r = 0; r < 4; ++r) x[4 * k4 + r] = v[r];
    }
    lane_linear<D6, D5>(P + SE.w[5], P + SE.b[5], x, c);
    const float n = lane_norm<D6>(c);
#pragma unroll
    for (int k = 0; k < D6; ++k) c[k] = c[k] / n;
    ae_store_codes(codes, code_layout, N, row, c);
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

hipError_t launch_lang_encoder(const olsr_lang_encoder_params& p, int N, const float* features, const float* params,
                               const float* online, float* features32, float* codes, hipStream_t st) {
  const auto kernel = p.in_layout == OLSR_LANG_ENCODER_IN_CHANNELS ? &lang_encoder_kernel<true> : &lang_encoder_kernel<false>;
  return dense_launch(kernel, N, LE_LDS_BYTES, st, N, (long long)p.plane_stride, p.bn_eps, features, params, online, features32,
                      codes, p.code_layout);
}

hipError_t launch_ss_encoder(const olsr_ss_encoder_params& p, int N, const float* features, const float* params, float* codes,
                             hipStream_t st) {
  const auto kernel = p.in_layout == OLSR_LANG_ENCODER_IN_CHANNELS ? &ss_encoder_kernel<true> : &ss_encoder_kernel<false>;
  return dense_launch(kernel, N, SE_LDS_BYTES, st, N, (long long)p.plane_stride, p.bn_eps, features, params, codes, p.code_layout);
}

}  // namespace olsr
