// k_lang_query.hip — open-vocabulary text queries on a rendered language map.
//
// The reference's evaluation (eval/evaluate_onlinelangslam.py:266-287, eval/openclip_encoder.py:44-107) decodes the 15-channel
// code map to 768 CLIP dimensions with two torch modules (EncoderDecoderOnline.decode 15 -> 24 -> 32, AutoencoderMLP.decode
// 32 -> 192 -> 256 -> 384 -> 512 -> 768, ReLU between layers, each followed by x / |x|), multiplies the [N,768] feature image
// with the phrase embeddings, and post-processes the similarities on the host (softmax against the negatives, cv2.filter2D,
// max / min, threshold).  Here:
//   lang_query_sims_kernel       stage A.  64 pixels per workgroup of four waves.  The activations of the 64 pixels live in ONE
//                                LDS image [64][516] (pixel-major); every layer is olsr_dense.h's Y^T = W X^T on
//                                v_mfma_f32_16x16x4_f32 with the weights as the A operand (straight from global memory / L2, every
//                                weight read by exactly one wave of the workgroup, so each is read once per 64 pixels).  A wave
//                                owns a quarter of the layer's output neurons for all 64 pixels and keeps them in accumulators
//                                until every wave has finished reading the layer's input, then overwrites the image in place.
//                                The last layer (512 -> 768) is produced in blocks of 64 neurons per wave; a block's accumulators
//                                are in the B-operand layout of the next product already (neuron on the register, pixel on the
//                                lane), so the K dot products with the phrase rows are four more MFMAs per 16 x 16 tile and the
//                                squared norm is a per-lane sum in double.  The 768-wide row is never stored anywhere.
//   ss_query_sims_kernel         stage A of the single-stage chain (language.single_stage_ae: True, include/
//                                olsr_single_stage.h; eval/evaluate_langslam.py:266-273, model.py:58-62): no online decoder, the
//                                general one is 15 -> 24 -> 48 -> 96 -> 192 -> 384 -> 384 -> 768.  The codes go through 15 -> 24 ->
//                                48 per pixel on the vector unit (decoder.0.weight [24,15] has no 16-byte aligned rows: scalar
//                                loads, bias-first k-ascending fmaf chains, twelve of the 48 neurons per wave), then 48 -> 96 ->
//                                192 -> 384 -> 384 out of the image and the same tail.  Its ReLU keeps a NaN
//                                (DENSE_EPI_RELU_NAN), as torch's does: a NaN code pixel gives NaN similarities for that pixel
//                                only (a pixel is a column of every product).  lang_query_sims_kernel's fmaxf differs there and
//                                stays as it is.
//   lang_query_relevancy_kernel  stage B, per output pixel: bilinear up-sampling of the similarity planes, the pairwise softmax
//                                against the negatives, the label argmax.
//   lang_query_smooth_kernel     the 30 x 30 mean (filter2D defaults: correlation, anchor (15,15), reflect-101) separable out of
//                                LDS with double sums, the blended map, and per 32 x 32 tile the partial max / argmax / min / max.
//   lang_query_reduce_kernel     the partials of a phrase in tile order: score, coordinate, min / max.  No atomics anywhere.
//   lang_query_mask_kernel       the thresholded mask of evaluate_onlinelangslam.py:146-152.
// Arithmetic is float32 throughout (an MFMA is a k-ordered fmaf chain); the norms and the window sums are double.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_dense.h"
#include "olsr_lang_ae_device.h"

#include <type_traits>

namespace olsr {

constexpr int LQ_C = AE_C, LQ_IN = AE_IN;  // the online decoder's ends (olsr_lang_ae_device.h)
constexpr int LQ_FEAT = OLSR_LANG_QUERY_FEATURE_DIM;
// the general decoders' layers in the flat arrays (state_dict order: weight [out,in], bias [out] per layer)
constexpr int LQ_D[] = {LQ_IN, 192, 256, 384, 512, LQ_FEAT};
constexpr int SQ_D[] = {LQ_C, 24, 48, 96, 192, 384, 384, LQ_FEAT};
constexpr auto LQ = flat_mlp(LQ_D, false);
constexpr auto SQ = flat_mlp(SQ_D, false);
static_assert(LQ.total == OLSR_LANG_QUERY_DECODER_PARAMS, "flat decoder layout");
static_assert(SQ.total == OLSR_SS_DECODER_PARAMS, "flat decoder layout");
static_assert(flat_mlp_aligned(LQ) && flat_mlp_aligned(SQ, 2), "16-byte loads of every weight and bias of the matrix layers");

// F.interpolate(mode="bilinear", align_corners=False) along one axis: the two taps and their weights (ATen UpSample.h:
// area_pixel_compute_source_index and guard_index_and_lambda, in float as for a float32 tensor)
struct LqTaps {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ LqTaps lq_taps(int dst, int in_size, float scale) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  LqTaps t;
  t.i0 = min((int)src, in_size - 1);
  t.i1 = t.i0 + (t.i0 < in_size - 1 ? 1 : 0);
  t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
  t.l0 = 1.f - t.l1;
  return t;
}
__device__ __forceinline__ float lq_sample(const float* __restrict__ plane, int w, const LqTaps& ty, const LqTaps& tx) {
  const float* r0 = plane + (size_t)ty.i0 * w;
  const float* r1 = plane + (size_t)ty.i1 * w;
  return ty.l0 * (tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1]) + ty.l1 * (tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1]);
}

struct LqGeom {
  int in_w, in_h, dec_w, dec_h, out_w, out_h;
  int resample_codes, resample_sims;
  float code_sx, code_sy, sim_sx, sim_sy;
};

// ---- stage A --------------------------------------------------------------------------------------------------------------

// a pixel's 15 codes out of the channel-major map, straight or resampled to the decode size
__device__ __forceinline__ void lq_fetch_codes(const float* __restrict__ codes, const LqGeom& g, int N, int row, float (&c)[LQ_C]) {
  if (g.resample_codes) {
    const int oy = row / g.dec_w, ox = row - oy * g.dec_w;
    const LqTaps ty = lq_taps(oy, g.in_h, g.code_sy), tx = lq_taps(ox, g.in_w, g.code_sx);
#pragma unroll
    for (int k = 0; k < LQ_C; ++k) c[k] = lq_sample(codes + (size_t)k * g.in_w * g.in_h, g.in_w, ty, tx);
  } else {
#pragma unroll
    for (int k = 0; k < LQ_C; ++k) c[k] = codes[(size_t)k * N + row];
  }
}

// hidden layer I (from 0) of the decoder D in place: X[64][KIN] -> relu(W X^T + b)^T = X[64][NOUT], the first WUSED waves
// share the neurons
template <const auto& D, int I, int WUSED, int EPI>
__device__ __forceinline__ void lq_hidden(float* __restrict__ X, const float* __restrict__ dec, int wave, int li, int q) {
  dense_layer<D.d[I], D.d[I + 1], LANG_WAVES, WUSED, LANG_S, EPI>(X, dec + D.w[I], dec + D.b[I], nullptr, nullptr, wave, li, q);
}

// KT: 16-row tiles of phrases (K <= 16 KT)
template <int KT>
__global__ __launch_bounds__(LANG_M * LANG_WAVES) void lang_query_sims_kernel(int N, LqGeom g, int K,
                                                                               const float* __restrict__ codes,
                                                                               const float* __restrict__ online,
                                                                               const float* __restrict__ dec,
                                                                               const float* __restrict__ phrases,
                                                                               float* __restrict__ sims) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [64][LANG_S]; afterwards the waves' partial dots and norms
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * LANG_M;
  // the pixel's codes (resampled to the decode size if asked) -> online decoder -> X[pixel][0..31]
  if (tid < LANG_M) {
    const int row = row0 + tid;
    float c[LQ_C];
    if (row < N) {
      lq_fetch_codes(codes, g, N, row, c);
      float h2[AE_H], r[LQ_IN];
      ae_decode(online, c, h2, r);  // r = y / |y|, as olsr_lang_ae_decode has it
#pragma unroll
      for (int k = 0; k < LQ_IN; ++k) X[tid * LANG_S + k] = r[k];
    } else {
#pragma unroll
      for (int k = 0; k < LQ_IN; ++k) X[tid * LANG_S + k] = 0.f;
    }
  }
  __syncthreads();
  lq_hidden<LQ, 0, 4, DENSE_EPI_RELU>(X, dec, wave, li, q);
  lq_hidden<LQ, 1, 4, DENSE_EPI_RELU>(X, dec, wave, li, q);
  lq_hidden<LQ, 2, 4, DENSE_EPI_RELU>(X, dec, wave, li, q);
  lq_hidden<LQ, 3, 4, DENSE_EPI_RELU>(X, dec, wave, li, q);
  dense_phrase_sims<LQ.d[4], LQ_FEAT, KT, LANG_WAVES, LANG_S>(X, dec + LQ.w[4], dec + LQ.b[4], phrases, K, N, row0, sims, wave, li,
                                                              q, tid);
}

template <int KT>
__global__ __launch_bounds__(LANG_M * LANG_WAVES) void ss_query_sims_kernel(int N, LqGeom g, int K, const float* __restrict__ codes,
                                                                             const float* __restrict__ dec,
                                                                             const float* __restrict__ phrases,
                                                                             float* __restrict__ sims) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [64][LANG_S]; afterwards the waves' partial dots and norms
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * LANG_M;
  // the pixel's codes (resampled to the decode size if asked) -> 15 -> 24 -> 48; wave w keeps neurons 12 w .. 12 w + 11 of the
  // 48 (the 24 are computed by each of the four: a neuron's chain is the same whoever computes it) -> X[pixel][0..47]
  {
    constexpr int D1 = SQ.d[1], PER = SQ.d[2] / LANG_WAVES;
    const int nb = __builtin_amdgcn_readfirstlane(wave) * PER;
    const int row = row0 + lane;
    float h2[PER];
    if (row < N) {
      float c[LQ_C], h1[D1];
      lq_fetch_codes(codes, g, N, row, c);
      lane_linear<D1, LQ_C>(dec + SQ.w[0], dec + SQ.b[0], c, h1);
#pragma unroll
      for (int k = 0; k < D1; ++k) h1[k] = relu_keep_nan(h1[k]);
      lane_linear<PER, D1>(dec + SQ.w[1] + nb * D1, dec + SQ.b[1] + nb, h1, h2);
#pragma unroll
      for (int k = 0; k < PER; ++k) h2[k] = relu_keep_nan(h2[k]);
    } else {
#pragma unroll
      for (int k = 0; k < PER; ++k) h2[k] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) X[lane * LANG_S + nb + k] = h2[k];
  }
  __syncthreads();
  lq_hidden<SQ, 2, 3, DENSE_EPI_RELU_NAN>(X, dec, wave, li, q);
  lq_hidden<SQ, 3, 4, DENSE_EPI_RELU_NAN>(X, dec, wave, li, q);
  lq_hidden<SQ, 4, 4, DENSE_EPI_RELU_NAN>(X, dec, wave, li, q);
  lq_hidden<SQ, 5, 4, DENSE_EPI_RELU_NAN>(X, dec, wave, li, q);
  dense_phrase_sims<SQ.d[6], LQ_FEAT, KT, LANG_WAVES, LANG_S>(X, dec + SQ.w[6], dec + SQ.b[6], phrases, K, N, row0, sims, wave, li,
                                                              q, tid);
}

// ---- stage B --------------------------------------------------------------------------------------------------------------

constexpr int LQ_WIN = 30, LQ_ANCHOR = 15;  // filter2D: the window covers -15 .. +14
constexpr int LQ_TILE = 32, LQ_HALO = LQ_TILE + LQ_WIN - 1;

// BORDER_REFLECT_101: gfedcb|abcdefgh|gfedcba
__device__ __forceinline__ int lq_reflect101(int i, int n) {
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  i %= period;
  if (i < 0) i += period;
  return i < n ? i : period - i;
}

__global__ __launch_bounds__(256) void lang_query_relevancy_kernel(LqGeom g, int K, int n_pos, int n_labels,
                                                                   const float* __restrict__ sims, float* __restrict__ rel,
                                                                   int32_t* __restrict__ labels) {
  const int n_out = g.out_w * g.out_h;
  const int px = blockIdx.x * 256 + threadIdx.x;
  if (px >= n_out) return;
  const size_t plane = (size_t)g.dec_w * g.dec_h;
  LqTaps ty{}, tx{};
  if (g.resample_sims) {
    const int oy = px / g.out_w, ox = px - oy * g.out_w;
    ty = lq_taps(oy, g.dec_h, g.sim_sy);
    tx = lq_taps(ox, g.dec_w, g.sim_sx);
  }
  auto sim = [&](int k) { return g.resample_sims ? lq_sample(sims + k * plane, g.dec_w, ty, tx) : sims[k * plane + px]; };
  const int neg0 = n_pos + n_labels;
  float sn = sim(neg0);
  for (int k = neg0 + 1; k < K; ++k) sn = fmaxf(sn, sim(k));
  // softmax(10 [s_p, s_n])[0], smallest over the negatives: the one with the largest s_n (torch.softmax's own steps)
  for (int p = 0; p < n_pos; ++p) {
    const float a = 10.f * sim(p), b = 10.f * sn, m = fmaxf(a, b);
    const float ea = expf(a - m), eb = expf(b - m);
    rel[(size_t)p * n_out + px] = ea / (ea + eb);
  }
  if (labels != nullptr) {
    int best = 0;
    float bv = sim(n_pos);
    for (int k = 1; k < K - n_pos; ++k) {
      const float v = sim(n_pos + k);
      if (v > bv) bv = v, best = k;
    }
    labels[px] = best < n_labels ? best : -1;
  }
}

struct LqPartial {
  float score;  // largest averaged value, and the first pixel (row-major) that has it
  int32_t index;
  float bmin, bmax;  // of the blended map
};
__device__ __forceinline__ void lq_combine(LqPartial& a, const LqPartial& b) {
  if (b.index >= 0 && (a.index < 0 || b.score > a.score || (b.score == a.score && b.index < a.index)))
    a.score = b.score, a.index = b.index;
  a.bmin = fminf(a.bmin, b.bmin);
  a.bmax = fmaxf(a.bmax, b.bmax);
}
// over the 256 threads of a workgroup; the result is in thread 0
__device__ __forceinline__ LqPartial lq_block_reduce(LqPartial v, LqPartial* red) {
#pragma unroll
  for (int mm = 32; mm >= 1; mm >>= 1) {
    LqPartial o;
    o.score = __shfl_xor(v.score, mm), o.index = __shfl_xor(v.index, mm);
    o.bmin = __shfl_xor(v.bmin, mm), o.bmax = __shfl_xor(v.bmax, mm);
    lq_combine(v, o);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; ++w) lq_combine(v, red[w]);
  return v;
}

__global__ __launch_bounds__(256) void lang_query_smooth_kernel(int W, int H, const float* __restrict__ rel,
                                                                float* __restrict__ smoothed, float* __restrict__ blended,
                                                                LqPartial* __restrict__ partials) {
  __shared__ float tile[LQ_HALO][LQ_HALO + 2];
  __shared__ double hsum[LQ_HALO][LQ_TILE];
  __shared__ LqPartial red[4];
  const int t = threadIdx.x, p = blockIdx.z;
  const int x0 = blockIdx.x * LQ_TILE, y0 = blockIdx.y * LQ_TILE;
  const size_t n_out = (size_t)W * H;
  const float* src = rel + p * n_out;
  for (int e = t; e < LQ_HALO * LQ_HALO; e += 256) {
    const int r = e / LQ_HALO, c = e - r * LQ_HALO;
    tile[r][c] = src[(size_t)lq_reflect101(y0 + r - LQ_ANCHOR, H) * W + lq_reflect101(x0 + c - LQ_ANCHOR, W)];
  }
  __syncthreads();
  for (int e = t; e < LQ_HALO * LQ_TILE; e += 256) {
    const int r = e / LQ_TILE, c = e - r * LQ_TILE;
    double s = 0.0;
#pragma unroll 6
    for (int k = 0; k < LQ_WIN; ++k) s += (double)tile[r][c + k];
    hsum[r][c] = s;
  }
  __syncthreads();
  LqPartial mine{0.f, -1, INFINITY, -INFINITY};
  const int c = t & 31, x = x0 + c;
#pragma unroll
  for (int j = 0; j < LQ_TILE / 8; ++j) {
    const int r = (t >> 5) + 8 * j, y = y0 + r;
    if (x >= W || y >= H) continue;
    double s = 0.0;
#pragma unroll 6
    for (int k = 0; k < LQ_WIN; ++k) s += hsum[r + k][c];
    const float avg = (float)(s / (double)(LQ_WIN * LQ_WIN));
    const float b = 0.5f * (avg + tile[r + LQ_ANCHOR][c + LQ_ANCHOR]);
    const size_t o = (size_t)y * W + x;
    smoothed[p * n_out + o] = avg;
    blended[p * n_out + o] = b;
    LqPartial v{avg, (int32_t)o, b, b};
    lq_combine(mine, v);
  }
  const LqPartial total = lq_block_reduce(mine, red);
  if (t == 0) partials[((size_t)p * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void lang_query_reduce_kernel(int W, int tiles, const LqPartial* __restrict__ partials,
                                                                float* __restrict__ score, int32_t* __restrict__ coord,
                                                                float* __restrict__ minmax) {
  __shared__ LqPartial red[4];
  const int p = blockIdx.x;
  LqPartial mine{0.f, -1, INFINITY, -INFINITY};
  for (int e = threadIdx.x; e < tiles; e += 256) lq_combine(mine, partials[(size_t)p * tiles + e]);
  const LqPartial total = lq_block_reduce(mine, red);
  if (threadIdx.x == 0) {
    score[p] = total.score;
    coord[2 * p] = total.index % W;  // (x, y), as the reference's coord[..., ::-1]
    coord[2 * p + 1] = total.index / W;
    minmax[2 * p] = total.bmin;
    minmax[2 * p + 1] = total.bmax;
  }
}

// output - min; / (max + 1e-9); * 2 - 1; clip to [0, 1]; > thresh  (evaluate_onlinelangslam.py:146-152, float32 steps)
__global__ __launch_bounds__(256) void lang_query_mask_kernel(size_t n_out, int n_pos, float thresh,
                                                              const float* __restrict__ blended, const float* __restrict__ minmax,
                                                              uint8_t* __restrict__ mask) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_out * n_pos) return;
  const int p = (int)(e / n_out);
  const float lo = minmax[2 * p], hi = minmax[2 * p + 1];
  float v = blended[e] - lo;
  v = v / ((hi - lo) + 1e-9f);
  v = v * 2.0f + -1.0f;
  v = fminf(fmaxf(v, 0.f), 1.f);
  mask[e] = v > thresh ? 1 : 0;
}

// ---- host -----------------------------------------------------------------------------------------------------------------

static LqGeom lq_geom(const olsr_lang_query_params& p) {
  LqGeom g{};
  g.in_w = p.in_width, g.in_h = p.in_height, g.dec_w = p.dec_width, g.dec_h = p.dec_height;
  g.out_w = p.out_width, g.out_h = p.out_height;
  g.resample_codes = (g.in_w != g.dec_w || g.in_h != g.dec_h) ? 1 : 0;
  g.resample_sims = (g.out_w != g.dec_w || g.out_h != g.dec_h) ? 1 : 0;
  g.code_sx = (float)g.in_w / (float)g.dec_w, g.code_sy = (float)g.in_h / (float)g.dec_h;
  g.sim_sx = (float)g.dec_w / (float)g.out_w, g.sim_sy = (float)g.dec_h / (float)g.out_h;
  return g;
}

static inline size_t lq_tiles(int w, int h) { return (size_t)((w + LQ_TILE - 1) / LQ_TILE) * ((h + LQ_TILE - 1) / LQ_TILE); }

// the scratch: per positive and 32 x 32 tile of the output one LqPartial
static LqPartial* lq_carve(void* buf, const olsr_lang_query_params& p, size_t& bytes) {
  Carver c(buf);
  LqPartial* partials = c.take<LqPartial>((size_t)(p.n_pos > 0 ? p.n_pos : 0) * lq_tiles(p.out_width, p.out_height));
  bytes = c.total();
  return partials;
}

size_t lang_query_scratch_bytes(const olsr_lang_query_params& p) {
  size_t bytes = 0;
  lq_carve(nullptr, p, bytes);
  return bytes;
}

// f(KT) for the number of 16-row phrase tiles that K phrases need
template <typename F>
static hipError_t lq_for_phrase_tiles(int K, F f) {
  if (K <= 16) return f(std::integral_constant<int, 1>());
  if (K <= 32) return f(std::integral_constant<int, 2>());
  return f(std::integral_constant<int, 4>());
}

hipError_t launch_lang_query_sims(const olsr_lang_query_params& p, const float* codes, const float* online, const float* dec,
                                  const float* phrases, float* sims, hipStream_t st) {
  const LqGeom g = lq_geom(p);
  const int N = p.dec_width * p.dec_height;
  return lq_for_phrase_tiles(p.K, [&](auto kt) {
    return dense_launch(&lang_query_sims_kernel<kt()>, N, LANG_ACT_BYTES, st, N, g, p.K, codes, online, dec, phrases, sims);
  });
}

hipError_t launch_ss_query_sims(const olsr_lang_query_params& p, const float* codes, const float* dec, const float* phrases,
                                float* sims, hipStream_t st) {
  const LqGeom g = lq_geom(p);
  const int N = p.dec_width * p.dec_height;
  return lq_for_phrase_tiles(p.K, [&](auto kt) {
    return dense_launch(&ss_query_sims_kernel<kt()>, N, LANG_ACT_BYTES, st, N, g, p.K, codes, dec, phrases, sims);
  });
}

void launch_lang_query_relevancy(const olsr_lang_query_params& p, const float* sims, float* relevancy, float* smoothed,
                                 float* blended, float* score, int32_t* coord, float* minmax, uint8_t* mask, int32_t* labels,
                                 void* scratch, hipStream_t st) {
  const LqGeom g = lq_geom(p);
  const int W = p.out_width, H = p.out_height;
  const size_t n_out = (size_t)W * H;
  lang_query_relevancy_kernel<<<(unsigned)((n_out + 255) / 256), 256, 0, st>>>(g, p.K, p.n_pos, p.n_labels, sims, relevancy,
                                                                              labels);
  if (p.n_pos <= 0) return;
  size_t bytes;
  LqPartial* partials = lq_carve(scratch, p, bytes);
  const dim3 grid((W + LQ_TILE - 1) / LQ_TILE, (H + LQ_TILE - 1) / LQ_TILE, p.n_pos);
  lang_query_smooth_kernel<<<grid, 256, 0, st>>>(W, H, relevancy, smoothed, blended, partials);
  lang_query_reduce_kernel<<<p.n_pos, 256, 0, st>>>(W, (int)lq_tiles(W, H), partials, score, coord, minmax);
  if (mask != nullptr)
    lang_query_mask_kernel<<<(unsigned)((n_out * p.n_pos + 255) / 256), 256, 0, st>>>(n_out, p.n_pos, p.thresh, blended, minmax,
                                                                                     mask);
}

}  // namespace olsr
