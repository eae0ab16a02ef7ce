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

namespace olsr {

constexpr int LQ_C = AE_C, LQ_IN = AE_IN;  // the online decoder's ends (olsr_lang_ae_device.h)

constexpr int LQ_M = 64;        // pixels per workgroup
constexpr int LQ_WAVES = 4;     // 256 threads
constexpr int LQ_S = 516;       // LDS floats per pixel: 512 + 4 (16 pixels' float4 reads of one k column hit 64 different banks)
constexpr int LQ_FEAT = OLSR_LANG_QUERY_FEATURE_DIM;
// the general decoder's layers in the flat array (state_dict order: weight [out,in], bias [out] per layer)
constexpr int LQ_D0 = 32, LQ_D1 = 192, LQ_D2 = 256, LQ_D3 = 384, LQ_D4 = 512, LQ_D5 = LQ_FEAT;
constexpr int LQ_OW1 = 0, LQ_OB1 = LQ_OW1 + LQ_D1 * LQ_D0, LQ_OW2 = LQ_OB1 + LQ_D1, LQ_OB2 = LQ_OW2 + LQ_D2 * LQ_D1,
              LQ_OW3 = LQ_OB2 + LQ_D2, LQ_OB3 = LQ_OW3 + LQ_D3 * LQ_D2, LQ_OW4 = LQ_OB3 + LQ_D3, LQ_OB4 = LQ_OW4 + LQ_D4 * LQ_D3,
              LQ_OW5 = LQ_OB4 + LQ_D4, LQ_OB5 = LQ_OW5 + LQ_D5 * LQ_D4;
static_assert(LQ_OB5 + LQ_D5 == OLSR_LANG_QUERY_DECODER_PARAMS, "flat decoder layout");

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

// one hidden layer in place: X[64][KIN] -> relu(W X^T + b)^T = X[64][NOUT], a quarter of the neurons per wave
template <int KIN, int NOUT>
__device__ __forceinline__ void lq_hidden(float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ bias,
                                          int wave, int li, int q) {
  dense_layer<KIN, NOUT, LQ_WAVES, LQ_WAVES, LQ_S, DENSE_EPI_RELU>(X, W, bias, nullptr, nullptr, wave, li, q);
}

// KT: 16-row tiles of phrases (K <= 16 KT)
template <int KT>
__global__ __launch_bounds__(LQ_M * LQ_WAVES) void lang_query_sims_kernel(int N, LqGeom g, int K,
                                                                                 const float* __restrict__ codes,
                                                                                 const float* __restrict__ online,
                                                                                 const float* __restrict__ dec,
                                                                                 const float* __restrict__ phrases,
                                                                                 float* __restrict__ sims) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [64][LQ_S]; afterwards the waves' partial dots and norms
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * LQ_M;
  // the pixel's codes (resampled to the decode size if asked) -> online decoder -> X[pixel][0..31]
  if (tid < LQ_M) {
    const int row = row0 + tid;
    float c[LQ_C];
    if (row < N) {
      if (g.resample_codes) {
        const int oy = row / g.dec_w, ox = row - oy * g.dec_w;
        const LqTaps ty = lq_taps(oy, g.in_h, g.code_sy), tx = lq_taps(ox, g.in_w, g.code_sx);
#pragma unroll
        for (int k = 0; k < LQ_C; ++k) c[k] = lq_sample(codes + (size_t)k * g.in_w * g.in_h, g.in_w, ty, tx);
      } else {
#pragma unroll
        for (int k = 0; k < LQ_C; ++k) c[k] = codes[(size_t)k * N + row];
      }
      float h2[AE_H], r[LQ_IN];
      ae_decode(online, c, h2, r);  // r = y / |y|, as olsr_lang_ae_decode has it
#pragma unroll
      for (int k = 0; k < LQ_IN; ++k) X[tid * LQ_S + k] = r[k];
    } else {
#pragma unroll
      for (int k = 0; k < LQ_IN; ++k) X[tid * LQ_S + k] = 0.f;
    }
  }
  __syncthreads();
  lq_hidden<LQ_D0, LQ_D1>(X, dec + LQ_OW1, dec + LQ_OB1, wave, li, q);
  lq_hidden<LQ_D1, LQ_D2>(X, dec + LQ_OW2, dec + LQ_OB2, wave, li, q);
  lq_hidden<LQ_D2, LQ_D3>(X, dec + LQ_OW3, dec + LQ_OB3, wave, li, q);
  lq_hidden<LQ_D3, LQ_D4>(X, dec + LQ_OW4, dec + LQ_OB4, wave, li, q);
  // the last layer in blocks of 4 x 16 neurons per wave, consumed as they arrive
  constexpr int NT = 4, CHUNKS = LQ_D5 / (16 * NT * LQ_WAVES);
  static_assert(CHUNKS * 16 * NT * LQ_WAVES == LQ_D5, "blocks of 64 neurons per wave");
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
    dense_gemm<LQ_D4, NT, LQ_S>(X, dec + LQ_OW5, dec + LQ_OB5, n0, li, q, acc);
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
        if (ph < K) pf = *reinterpret_cast<const f32x4*>(phrases + (size_t)ph * LQ_FEAT + n0 + 16 * t + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int pt = 0; pt < 4; ++pt)
            sacc[kt][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pf[r], acc[t][pt][r], sacc[kt][pt], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // the activations are no longer read
  float* dots = X;                                                            // [wave][16 KT phrases][64 pixels]
  double* norms = reinterpret_cast<double*>(X + LQ_WAVES * 16 * KT * LQ_M);  // [wave][q][64 pixels]
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    norms[(wave * 4 + q) * LQ_M + pt * 16 + li] = nrm[pt];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) dots[(wave * 16 * KT + kt * 16 + 4 * q + r) * LQ_M + pt * 16 + li] = sacc[kt][pt][r];
  }
  __syncthreads();
  for (int e = tid; e < K * LQ_M; e += LQ_M * LQ_WAVES) {
    const int ph = e / LQ_M, px = e - ph * LQ_M;
    if (row0 + px >= N) continue;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < LQ_WAVES * 4; ++k) s += norms[k * LQ_M + px];
    const float d = (dots[(0 * 16 * KT + ph) * LQ_M + px] + dots[(1 * 16 * KT + ph) * LQ_M + px]) +
                    (dots[(2 * 16 * KT + ph) * LQ_M + px] + dots[(3 * 16 * KT + ph) * LQ_M + px]);
    sims[(size_t)ph * N + row0 + px] = d / (float)sqrt(s);
  }
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

// [per positive and 32 x 32 tile of the output one LqPartial] behind a 256-byte aligned base
size_t lang_query_scratch_bytes(const olsr_lang_query_params& p) {
  const size_t n_pos = p.n_pos > 0 ? (size_t)p.n_pos : 0;
  return n_pos * lq_tiles(p.out_width, p.out_height) * sizeof(LqPartial) + 256;
}

template <int KT>
static hipError_t lq_launch_sims(int N, const LqGeom& g, int K, const float* codes, const float* online, const float* dec,
                                 const float* phrases, float* sims, hipStream_t st) {
  constexpr size_t act = (size_t)LQ_M * LQ_S * sizeof(float);
  constexpr size_t red = (size_t)LQ_WAVES * 16 * KT * LQ_M * sizeof(float) + (size_t)LQ_WAVES * 4 * LQ_M * sizeof(double);
  static_assert(red <= act && act <= 160 * 1024, "one LDS image per workgroup");
  // more than 64 KiB of dynamic LDS has to be asked for (a host-side attribute of the current device's function: no launch)
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&lang_query_sims_kernel<KT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)act);
  if (e != hipSuccess) return e;
  lang_query_sims_kernel<KT><<<(N + LQ_M - 1) / LQ_M, LQ_M * LQ_WAVES, act, st>>>(N, g, K, codes, online, dec, phrases, sims);
  return hipSuccess;
}

hipError_t launch_lang_query_sims(const olsr_lang_query_params& p, const float* codes, const float* online, const float* dec,
                                  const float* phrases, float* sims, hipStream_t st) {
  const LqGeom g = lq_geom(p);
  const int N = p.dec_width * p.dec_height;
  if (p.K <= 16) return lq_launch_sims<1>(N, g, p.K, codes, online, dec, phrases, sims, st);
  if (p.K <= 32) return lq_launch_sims<2>(N, g, p.K, codes, online, dec, phrases, sims, st);
  return lq_launch_sims<4>(N, g, p.K, codes, online, dec, phrases, sims, st);
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
  LqPartial* partials = (LqPartial*)(((uintptr_t)scratch + 255) / 256 * 256);
  const dim3 grid((W + LQ_TILE - 1) / LQ_TILE, (H + LQ_TILE - 1) / LQ_TILE, p.n_pos);
  lang_query_smooth_kernel<<<grid, 256, 0, st>>>(W, H, relevancy, smoothed, blended, partials);
  lang_query_reduce_kernel<<<p.n_pos, 256, 0, st>>>(W, (int)lq_tiles(W, H), partials, score, coord, minmax);
  if (mask != nullptr)
    lang_query_mask_kernel<<<(unsigned)((n_out * p.n_pos + 255) / 256), 256, 0, st>>>(n_out, p.n_pos, p.thresh, blended, minmax,
                                                                                     mask);
}

}  // namespace olsr
