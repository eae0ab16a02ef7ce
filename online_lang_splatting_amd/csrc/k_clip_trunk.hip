// k_clip_trunk.hip — the CLIP ConvNeXt image tower (include/olsr_clip_trunk.h): a frame in, res2 / res3 / clip_vis_dense out.
//
// Between launches a map is pixel-major ([pixel][channel], NHWC): a pixel's channels are one contiguous row, which is what
// the B operand of the dense layers, the LayerNorms and the depthwise convolution's lanes all want.  The three outputs are
// written channel-major by the epilogue that produces them.  Five kernels:
//   ct_gemm_kernel<SRC, EPI>  Y^T = W X^T on v_mfma_f32_16x16x4_f32, a workgroup of four waves per 64 pixels x 64 neurons (16 per
//                        wave, four accumulator tiles), k_hr_net.hip's loop: the weights are the A operand straight from the
//                        packed array, the next block's load ahead of the current MFMAs; the activations pass through a
//                        double-buffered LDS image [64 pixels][32 + 4].  Tiling over neurons as well as pixels is what keeps
//                        the late stages busy: 36 pixel tiles at stage 2 become 36 x 48 workgroups for fc1.
//     SRC  PLAIN          a pixel-major map (fc1's and fc2's input).
//          LN1, LN4       a pixel-major map normalised while it is staged: the head's LayerNorm, and the downsample's, whose
//                         2x2 stride-2 convolution is a dense layer over k = (2 ky + kx) Cin + c.  The statistics of the tile's
//                         64 (256) input pixels are computed first, a wave per pixel.
//          STEM           the frame itself: normalised and sampled bilinearly at the resized grid's 4x4 patch while it is staged
//                         (k = 16 c + 4 ky + kx).  No resized copy exists.
//     EPI  BIAS, GELU     pixel-major out.   RESID  x + gamma * acc, pixel-major and / or channel-major.   HEAD  channel-major.
//   ct_mlp_fused_kernel<NT>  a block's fc1 -> GELU -> fc2 -> residual for C = 64 NT <= 256 per 64-pixel tile: the normalised input
//                        [64][C + 4] stays in LDS, the hidden row passes through a [64][64 + 4] buffer 64 neurons at a time
//                        (a wave computes 16 of them, then all four waves take the chunk as 64 more k of fc2, C / 4 output
//                        neurons per wave in accumulators).  Stage 0's hidden map (113 MB per block at the real size) is never
//                        stored.  Same k order as the two launches above, so the same bits.
//   ct_dw_ln_kernel      depthwise 7x7 + LayerNorm: a wave owns four adjacent pixels of a row, a lane the channels lane + 64 i;
//                        a row of the window is loaded once for the four outputs.  The raw sums are parked in the output
//                        row, which the same lanes read back for the statistics and the normalisation.
//   ct_ln_rows_kernel    the stem's LayerNorm in place, a wave per pixel.
//   ct_to_nhwc_kernel    olsr_convnext_block's channel-major input into the workspace.
// Arithmetic and k order: include/olsr_clip_trunk.h.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_collectives.h"
#include "olsr_dense.h"

namespace olsr {

constexpr int CT_TP = 64;          // pixels per workgroup
constexpr int CT_TN = 64;          // neurons per workgroup, 16 per wave
constexpr int CT_THREADS = 256;
constexpr int CT_KC = 32;          // k per staged chunk
constexpr int CT_CS = CT_KC + 4;   // LDS floats per pixel of a chunk
constexpr int CT_HS = 64 + 4;      // LDS floats per pixel of the fused kernel's hidden chunk
constexpr int CT_DW_PX = 4;        // adjacent pixels per wave of the depthwise kernel

enum { CT_SRC_PLAIN = 0, CT_SRC_LN1 = 1, CT_SRC_LN4 = 2, CT_SRC_STEM = 3 };
enum { CT_EPI_BIAS = 0, CT_EPI_GELU = 1, CT_EPI_RESID = 2, CT_EPI_HEAD = 3 };

__device__ __forceinline__ float ct_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// mean and 1 / sqrt(var + eps) of a row of C floats, by a whole wave: the same values in every lane
__device__ __forceinline__ void ct_row_stats(const float* row, int C, int lane, double eps, double& mean, double& rstd) {
  double s = 0.0;
  for (int c = lane; c < C; c += 64) s += (double)row[c];
  mean = wave_sum(s) / (double)C;
  double ss = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double d = (double)row[c] - mean;
    ss = fma(d, d, ss);
  }
  rstd = 1.0 / sqrt(wave_sum(ss) / (double)C + eps);
}
__device__ __forceinline__ float ct_ln(float v, double mean, double rstd, float w, float b) {
  return fmaf((float)(((double)v - mean) * rstd), w, b);
}

// ---- depthwise 7x7 + LayerNorm ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT_THREADS) void ct_dw_ln_kernel(const float* __restrict__ X, int h, int w, int C,
                                                              const float* __restrict__ dww, const float* __restrict__ dwb,
                                                              const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                              double eps, float* T) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int groups_x = (w + CT_DW_PX - 1) / CT_DW_PX;
  const long long g = (long long)blockIdx.x * 4 + wave;
  if (g >= (long long)h * groups_x) return;  // (a whole wave; the kernel has no barrier)
  const int y = (int)(g / groups_x), x0 = (int)(g % groups_x) * CT_DW_PX;
  for (int c = lane; c < C; c += 64) {
    float acc[CT_DW_PX];
    const float b = dwb[c];
#pragma unroll
    for (int o = 0; o < CT_DW_PX; ++o) acc[o] = b;
#pragma unroll 1
    for (int ky = 0; ky < 7; ++ky) {
      const int yy = y + ky - 3;
      if (yy < 0 || yy >= h) continue;  // a padded tap adds nothing
      float v[CT_DW_PX + 6];
#pragma unroll
      for (int i = 0; i < CT_DW_PX + 6; ++i) {
        const int xx = x0 - 3 + i;
        v[i] = (xx >= 0 && xx < w) ? X[((size_t)yy * w + xx) * C + c] : 0.f;
      }
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const float wv = dww[(ky * 7 + kx) * C + c];
#pragma unroll
        for (int o = 0; o < CT_DW_PX; ++o) {
          const int xx = x0 + o + kx - 3;
          if (xx >= 0 && xx < w) acc[o] = fmaf(wv, v[o + kx], acc[o]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < CT_DW_PX; ++o)
      if (x0 + o < w) T[((size_t)y * w + x0 + o) * C + c] = acc[o];
  }
  // (each lane reads back what it stored itself)
  for (int o = 0; o < CT_DW_PX; ++o) {
    if (x0 + o >= w) break;
    float* row = T + ((size_t)y * w + x0 + o) * C;
    double mean, rstd;
    ct_row_stats(row, C, lane, eps, mean, rstd);
    for (int c = lane; c < C; c += 64) row[c] = ct_ln(row[c], mean, rstd, lnw[c], lnb[c]);
  }
}

__global__ __launch_bounds__(CT_THREADS) void ct_ln_rows_kernel(float* X, int NP, int C, const float* __restrict__ lnw,
                                                                const float* __restrict__ lnb, double eps) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= NP) return;
  float* row = X + (size_t)p * C;
  double mean, rstd;
  ct_row_stats(row, C, lane, eps, mean, rstd);
  for (int c = lane; c < C; c += 64) row[c] = ct_ln(row[c], mean, rstd, lnw[c], lnb[c]);
}

__global__ __launch_bounds__(CT_THREADS) void ct_to_nhwc_kernel(const float* __restrict__ x, int NP, int C, float* __restrict__ X) {
  const long long e = (long long)blockIdx.x * CT_THREADS + threadIdx.x;
  if (e >= (long long)NP * C) return;
  const int p = (int)(e / C), c = (int)(e - (long long)p * C);
  X[e] = x[(size_t)c * NP + p];
}

// ---- the dense layers -------------------------------------------------------------------------------------------------------------
struct ct_gemm_args {
  const float* src;  // [pixels][Cin] (PLAIN, LN1, LN4) or the frame [3][H W] (STEM)
  int NP;            // output pixels
  int K, Cin;        // k extent (Cin, 4 Cin, or 48) and the source's channels
  int ow;            // the output map's width (LN4, STEM)
  int H, W, R;       // the frame's size and the resized grid's (STEM)
  float mean[3], std[3];
  const float* lnw;  // [Cin] (LN1, LN4)
  const float* lnb;
  double eps;
  const float* wt;    // [OUT][K]
  const float* bias;  // [OUT] (not HEAD)
  int OUT;
  const float* gamma;  // [OUT] (RESID)
  const float* resid;  // [NP][OUT] (RESID); may be out_nhwc
  float* out_nhwc;     // [NP][OUT] or null (RESID)
  float* out_chw;      // [OUT] planes of NP or null (RESID, HEAD)
};

template <int SRC, int EPI>
__global__ __launch_bounds__(CT_THREADS) void ct_gemm_kernel(const ct_gemm_args a) {
  constexpr bool LN = SRC == CT_SRC_LN1 || SRC == CT_SRC_LN4;
  constexpr int TAPS = SRC == CT_SRC_LN4 ? 4 : 1;
  __shared__ __attribute__((aligned(16))) float buf[2][CT_TP * CT_CS];
  __shared__ double stat[LN ? 2 * CT_TP * TAPS : 2];  // [tap][pixel]{mean, rstd}
  __shared__ int in_pix[LN ? CT_TP * TAPS : 1];       // [tap][pixel]: the source pixel

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int P0 = blockIdx.x * CT_TP;
  const int n0 = blockIdx.y * CT_TN + wave * 16;
  const bool mine = n0 < a.OUT;  // (OUT is a multiple of 16; a wave without neurons still stages)

  if (LN) {
    for (int ip = wave; ip < CT_TP * TAPS; ip += 4) {
      const int tap = ip / CT_TP, px = ip - tap * CT_TP, P = P0 + px;
      if (P >= a.NP) continue;  // (staged as zeros, never looked up)
      int src_px = P;
      if (SRC == CT_SRC_LN4) {
        const int oy = P / a.ow, ox = P - oy * a.ow;
        src_px = (2 * oy + (tap >> 1)) * (2 * a.ow) + 2 * ox + (tap & 1);
      }
      double mean, rstd;
      ct_row_stats(a.src + (size_t)src_px * a.Cin, a.Cin, lane, a.eps, mean, rstd);
      if (lane == 0) stat[2 * ip] = mean, stat[2 * ip + 1] = rstd, in_pix[ip] = src_px;
    }
    __syncthreads();
  }

  // ---- what this thread stages per chunk: two float4 of a pixel's row (PLAIN, LN), or eight samples of one pixel (STEM) ---
  float pre[8];
  int oy = 0, ox = 0;
  if (SRC == CT_SRC_STEM) {
    const int P = P0 + (tid & 63);
    oy = P < a.NP ? P / a.ow : 0, ox = P < a.NP ? P - oy * a.ow : 0;
  }
  auto fetch = [&](int k0) {
    if (SRC == CT_SRC_STEM) {
      const bool live = P0 + (tid & 63) < a.NP;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int k = k0 + (tid >> 6) + 4 * i;
        float v = 0.f;
        if (live && k < a.K) {
          const int c = k >> 4, Y = 4 * oy + ((k >> 2) & 3), Xc = 4 * ox + (k & 3);
          // upsample_bilinear2d, align_corners = False (k_hr_net.hip): src = max(scale (dst + 0.5) - 0.5, 0)
          const float sy = fmaxf(((float)a.H / (float)a.R) * ((float)Y + 0.5f) - 0.5f, 0.f);
          const float sx = fmaxf(((float)a.W / (float)a.R) * ((float)Xc + 0.5f) - 0.5f, 0.f);
          const int y0 = min((int)sy, a.H - 1), x0 = min((int)sx, a.W - 1);
          const int y1 = y0 + (a.H != a.R && y0 < a.H - 1 ? 1 : 0), x1 = x0 + (a.W != a.R && x0 < a.W - 1 ? 1 : 0);
          const float ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
          const float* p = a.src + (size_t)c * ((size_t)a.H * a.W);
          const float m = a.mean[c], s = a.std[c];
          const float p00 = (p[(size_t)y0 * a.W + x0] * 255.f - m) / s, p01 = (p[(size_t)y0 * a.W + x1] * 255.f - m) / s;
          const float p10 = (p[(size_t)y1 * a.W + x0] * 255.f - m) / s, p11 = (p[(size_t)y1 * a.W + x1] * 255.f - m) / s;
          v = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11);
        }
        pre[i] = v;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int f = tid + CT_THREADS * i, px = f >> 3, k = k0 + (f & 7) * 4;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (P0 + px < a.NP) {
          if (LN) {
            const int tap = k / a.Cin, ci = k - tap * a.Cin, ip = tap * CT_TP + px;
            v = *reinterpret_cast<const f32x4*>(a.src + (size_t)in_pix[ip] * a.Cin + ci);
            const double mean = stat[2 * ip], rstd = stat[2 * ip + 1];
            const f32x4 lw = *reinterpret_cast<const f32x4*>(a.lnw + ci), lb = *reinterpret_cast<const f32x4*>(a.lnb + ci);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = ct_ln(v[r], mean, rstd, lw[r], lb[r]);
          } else {
            v = *reinterpret_cast<const f32x4*>(a.src + (size_t)(P0 + px) * a.K + k);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) pre[4 * i + r] = v[r];
      }
    }
  };
  auto park = [&](float* b) {
    if (SRC == CT_SRC_STEM) {
#pragma unroll
      for (int i = 0; i < 8; ++i) b[(tid & 63) * CT_CS + (tid >> 6) + 4 * i] = pre[i];
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int f = tid + CT_THREADS * i;
        *reinterpret_cast<f32x4*>(b + (f >> 3) * CT_CS + (f & 7) * 4) = f32x4{pre[4 * i], pre[4 * i + 1], pre[4 * i + 2], pre[4 * i + 3]};
      }
    }
  };

  // ---- K loop: chunks of 32 in order, inside a chunk the 16-deep blocks in order; every 64 k the partial sums, which
  // start from zero, are added to the running sums, which start from the bias (a chain of 6144 single roundings would cost
  // the late stages' fc2 bits that the blocked sum keeps) ---------------------------------------------------------------------
  const float* wp = a.wt + (size_t)(mine ? n0 + li : 0) * (size_t)a.K + 4 * q;
  f32x4 acc[1][4], part[1][4];
  {
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (EPI != CT_EPI_HEAD && mine) bv = *reinterpret_cast<const f32x4*>(a.bias + n0 + 4 * q);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[0][pt] = bv, part[0][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int nchunks = (a.K + CT_KC - 1) / CT_KC;
  f32x4 wa[1] = {*reinterpret_cast<const f32x4*>(wp)};
  fetch(0);
  park(buf[0]);
  __syncthreads();
#pragma unroll 1
  for (int ch = 0; ch < nchunks; ++ch) {
    const bool more = ch + 1 < nchunks;
    if (more) fetch((ch + 1) * CT_KC);
    const float* xb = buf[ch & 1] + li * CT_CS + 4 * q;
#pragma unroll
    for (int kb = 0; kb < CT_KC; kb += 16) {
      const int k = ch * CT_KC + kb;
      if (k < a.K) {  // (the stem's k extent, 48, ends in a half chunk)
        const int kn = k + 16 < a.K ? k + 16 : k;
        const f32x4 wn = *reinterpret_cast<const f32x4*>(wp + kn);
        if (mine) dense_block<1, CT_CS>(wa, xb + kb, part);
        wa[0] = wn;
      }
    }
    if ((ch & 1) || !more) {
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) acc[0][pt] += part[0][pt], part[0][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (more) park(buf[(ch + 1) & 1]);  // last read before the previous barrier
    __syncthreads();
  }
  if (!mine) return;

  // ---- epilogue: lane (li, q) holds neurons n0 + 4 q + {0..3} of pixel 16 pt + li ---------------------------------------------
  const int n = n0 + 4 * q;
  f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
  if (EPI == CT_EPI_RESID) g = *reinterpret_cast<const f32x4*>(a.gamma + n);
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int P = P0 + 16 * pt + li;
    if (P >= a.NP) continue;
    f32x4 v = acc[0][pt];
    if (EPI == CT_EPI_GELU) {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = ct_gelu(v[r]);
    }
    if (EPI == CT_EPI_RESID) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(a.resid + (size_t)P * a.OUT + n);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float br = g[r] * v[r];
        v[r] = x[r] + br;
      }
    }
    if (EPI == CT_EPI_BIAS || EPI == CT_EPI_GELU || (EPI == CT_EPI_RESID && a.out_nhwc))
      *reinterpret_cast<f32x4*>(a.out_nhwc + (size_t)P * a.OUT + n) = v;
    if (EPI == CT_EPI_HEAD || (EPI == CT_EPI_RESID && a.out_chw)) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a.out_chw[(size_t)(n + r) * a.NP + P] = v[r];
    }
  }
}

// acc += the 64 k from wp / xk on, summed from zero (ct_gemm_kernel's rule); wp: the lane's row of tile 0 at its k offset,
// tile t's row `tile_stride` floats on; xk: the lane's pixel li at the same k offset in an image of S floats per pixel
template <int NT, int S>
__device__ __forceinline__ void ct_dense64(const float* __restrict__ wp, size_t tile_stride, const float* __restrict__ xk,
                                           f32x4 (&acc)[NT][4]) {
  f32x4 part[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) part[t][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < 64; kb += 16) {
    f32x4 w[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) w[t] = *reinterpret_cast<const f32x4*>(wp + t * tile_stride + kb);
    dense_block<NT, S>(w, xk + kb, part);
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[t][pt] += part[t][pt];
}

// ---- a narrow block's fc1 -> GELU -> fc2 -> residual ------------------------------------------------------------------------------
struct ct_mlp_args {
  const float* T;      // [NP][C] the normalised depthwise output
  const float* resid;  // [NP][C] the block's input; may be out_nhwc
  int NP;
  const float* w1;  // [4C][C]
  const float* b1;
  const float* w2;  // [C][4C]
  const float* b2;
  const float* gamma;
  float* out_nhwc;  // or null
  float* out_chw;   // or null
};

template <int NT>
__global__ __launch_bounds__(CT_THREADS) void ct_mlp_fused_kernel(const ct_mlp_args a) {
  constexpr int C = 64 * NT, S = C + 4, HID = 4 * C;
  extern __shared__ __attribute__((aligned(16))) float ct_lds[];
  float* A = ct_lds;             // [64][S]
  float* Hc = ct_lds + CT_TP * S;  // [64][CT_HS]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int P0 = blockIdx.x * CT_TP;
#pragma unroll
  for (int i = 0; i < 4 * NT; ++i) {
    const int f = tid + CT_THREADS * i, px = f / (C / 4), c4 = (f - px * (C / 4)) * 4;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (P0 + px < a.NP) v = *reinterpret_cast<const f32x4*>(a.T + (size_t)(P0 + px) * C + c4);
    *reinterpret_cast<f32x4*>(A + px * S + c4) = v;
  }
  __syncthreads();
  const int n0 = wave * 16 * NT;
  f32x4 acc2[NT][4];
  dense_bias<NT>(a.b2, n0, q, acc2);
#pragma unroll 1
  for (int hc = 0; hc < HID / 64; ++hc) {
    const int h0 = hc * 64 + wave * 16;
    f32x4 acc1[1][4];
    dense_bias<1>(a.b1, h0, q, acc1);
#pragma unroll
    for (int k64 = 0; k64 < C; k64 += 64)
      ct_dense64<1, S>(a.w1 + (size_t)(h0 + li) * C + k64 + 4 * q, 0, A + li * S + k64 + 4 * q, acc1);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      f32x4 v = acc1[0][pt];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = ct_gelu(v[r]);
      *reinterpret_cast<f32x4*>(Hc + (16 * pt + li) * CT_HS + wave * 16 + 4 * q) = v;
    }
    __syncthreads();
    ct_dense64<NT, CT_HS>(a.w2 + (size_t)(n0 + li) * HID + hc * 64 + 4 * q, (size_t)16 * HID, Hc + li * CT_HS + 4 * q, acc2);
    __syncthreads();  // the chunk is rewritten next
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + 4 * q;
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.gamma + n);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int P = P0 + 16 * pt + li;
      if (P >= a.NP) continue;
      const f32x4 x = *reinterpret_cast<const f32x4*>(a.resid + (size_t)P * C + n);
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float br = g[r] * acc2[t][pt][r];
        v[r] = x[r] + br;
      }
      if (a.out_nhwc) *reinterpret_cast<f32x4*>(a.out_nhwc + (size_t)P * C + n) = v;
      if (a.out_chw) {
#pragma unroll
        for (int r = 0; r < 4; ++r) a.out_chw[(size_t)(n + r) * a.NP + P] = v[r];
      }
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------

long long ct_block_floats(long long C) { return 8 * C * C + 58 * C; }
static bool ct_fused(int C) { return C <= OLSR_CLIP_TRUNK_FUSED_MAX_C; }
static int ct_block_launches(int C) { return ct_fused(C) ? 2 : 3; }

size_t convnext_block_workspace_bytes(long long C, long long h, long long w) {
  return (size_t)(h * w * C * (ct_fused((int)C) ? 2 : 6)) * sizeof(float);
}

long long clip_trunk_packed_floats(const olsr_clip_trunk_params& p) {
  long long n = (long long)p.dims[0] * 48 + 3LL * p.dims[0];
  for (int i = 0; i < 4; ++i) {
    if (i > 0) n += 2LL * p.dims[i - 1] + 4LL * p.dims[i] * p.dims[i - 1] + p.dims[i];
    n += p.depths[i] * ct_block_floats(p.dims[i]);
  }
  return n + 2LL * p.dims[3] + (long long)p.embed_dim * p.dims[3];
}

long long clip_trunk_launches(const olsr_clip_trunk_params& p) {
  long long n = 2 + 3 + 1;
  for (int i = 0; i < 4; ++i) n += (long long)p.depths[i] * ct_block_launches(p.dims[i]);
  return n;
}

// in floats: the largest stage map, and the largest hidden map of a three-launch stage
static void ct_workspace_parts(const olsr_clip_trunk_params& p, long long& map, long long& hidden) {
  map = hidden = 0;
  for (int i = 0; i < 4; ++i) {
    const long long side = p.R >> (2 + i), m = side * side * p.dims[i];
    map = m > map ? m : map;
    if (!ct_fused(p.dims[i])) hidden = 4 * m > hidden ? 4 * m : hidden;
  }
}
size_t clip_trunk_workspace_bytes(const olsr_clip_trunk_params& p) {
  long long map, hidden;
  ct_workspace_parts(p, map, hidden);
  return (size_t)(2 * map + hidden) * sizeof(float);
}

template <int SRC, int EPI>
static void ct_gemm(const ct_gemm_args& a, hipStream_t st) {
  ct_gemm_kernel<SRC, EPI><<<dim3((a.NP + CT_TP - 1) / CT_TP, (a.OUT + CT_TN - 1) / CT_TN), CT_THREADS, 0, st>>>(a);
}

template <int NT>
static hipError_t ct_mlp_fused(const ct_mlp_args& a, hipStream_t st) {
  return dense_launch(ct_mlp_fused_kernel<NT>, a.NP, (size_t)CT_TP * (64 * NT + 4 + CT_HS) * sizeof(float), st, a);
}

// One block on the pixel-major map X [h w][C]: X -> T (depthwise + LayerNorm) -> out.  Hd: the hidden map of a three-launch
// block.  out_nhwc may be X.  want(): whether the next launch of the call is switched on.
template <class Want>
static hipError_t ct_block(int C, int h, int w, const float* X, float* T, float* Hd, const float* B, double eps, float* out_nhwc,
                           float* out_chw, Want want, hipStream_t st) {
  const int NP = h * w;
  const float* dww = B;
  const float* dwb = dww + 49 * (size_t)C;
  const float* lnw = dwb + C;
  const float* lnb = lnw + C;
  const float* w1 = lnb + C;
  const float* b1 = w1 + 4 * (size_t)C * C;
  const float* w2 = b1 + 4 * C;
  const float* b2 = w2 + 4 * (size_t)C * C;
  const float* gamma = b2 + C;
  if (want()) {
    const long long waves = (long long)h * ((w + CT_DW_PX - 1) / CT_DW_PX);
    ct_dw_ln_kernel<<<(unsigned)((waves + 3) / 4), CT_THREADS, 0, st>>>(X, h, w, C, dww, dwb, lnw, lnb, eps, T);
  }
  if (ct_fused(C)) {
    if (!want()) return hipSuccess;
    const ct_mlp_args m{T, X, NP, w1, b1, w2, b2, gamma, out_nhwc, out_chw};
    switch (C / 64) {
      case 1: return ct_mlp_fused<1>(m, st);
      case 2: return ct_mlp_fused<2>(m, st);
      case 3: return ct_mlp_fused<3>(m, st);
      default: return ct_mlp_fused<4>(m, st);
    }
  }
  ct_gemm_args a{};
  a.src = T, a.NP = NP, a.K = C, a.Cin = C, a.wt = w1, a.bias = b1, a.OUT = 4 * C, a.out_nhwc = Hd;
  if (want()) ct_gemm<CT_SRC_PLAIN, CT_EPI_GELU>(a, st);
  a = ct_gemm_args{};
  a.src = Hd, a.NP = NP, a.K = 4 * C, a.Cin = 4 * C, a.wt = w2, a.bias = b2, a.OUT = C, a.gamma = gamma, a.resid = X;
  a.out_nhwc = out_nhwc, a.out_chw = out_chw;
  if (want()) ct_gemm<CT_SRC_PLAIN, CT_EPI_RESID>(a, st);
  return hipSuccess;
}

hipError_t launch_convnext_block(const olsr_convnext_block_params& p, const float* x, const float* B, float* y, float* ws,
                                 hipStream_t st) {
  const int NP = p.h * p.w;
  float* X = ws;
  float* T = X + (size_t)NP * p.C;
  float* Hd = T + (size_t)NP * p.C;
  const long long n = (long long)NP * p.C;
  ct_to_nhwc_kernel<<<(unsigned)((n + CT_THREADS - 1) / CT_THREADS), CT_THREADS, 0, st>>>(x, NP, p.C, X);
  return ct_block(p.C, p.h, p.w, X, T, Hd, B, p.ln_eps, nullptr, y, [] { return true; }, st);
}

hipError_t launch_clip_trunk(const olsr_clip_trunk_params& p, const float* image, const float* P, float* res2, float* res3,
                             float* vis, float* ws, hipStream_t st) {
  long long map, hidden;
  ct_workspace_parts(p, map, hidden);
  float* X = ws;
  float* T = ws + map;
  float* Hd = ws + 2 * map;
  const bool all = (p.launches[0] | p.launches[1]) == 0;
  int k = 0;
  auto want = [&]() {
    const bool on = all || ((p.launches[k >> 6] >> (k & 63)) & 1u) != 0;
    ++k;
    return on;
  };
  const double eps = p.ln_eps;
  int side = p.R / 4;
  // stem: the frame, normalised and resized while it is staged -> Conv2d(3, d0, 4, 4) -> LayerNorm
  {
    const int d0 = p.dims[0];
    ct_gemm_args a{};
    a.src = image, a.NP = side * side, a.K = 48, a.Cin = 3, a.ow = side, a.H = p.H, a.W = p.W, a.R = p.R;
    for (int c = 0; c < 3; ++c) a.mean[c] = p.mean[c], a.std[c] = p.std[c];
    a.wt = P, a.bias = P + (size_t)d0 * 48, a.OUT = d0, a.out_nhwc = X;
    if (want()) ct_gemm<CT_SRC_STEM, CT_EPI_BIAS>(a, st);
    if (want()) ct_ln_rows_kernel<<<(a.NP + 3) / 4, CT_THREADS, 0, st>>>(X, a.NP, d0, a.bias + d0, a.bias + 2 * d0, eps);
    P = a.bias + 3 * (size_t)d0;
  }
  for (int i = 0; i < 4; ++i) {
    const int C = p.dims[i];
    if (i > 0) {
      // downsample: LayerNorm in the staging of Conv2d(d[i-1], d[i], 2, 2) as a dense layer; X -> T, and the two swap
      const int Cin = p.dims[i - 1];
      side /= 2;
      ct_gemm_args a{};
      a.src = X, a.NP = side * side, a.K = 4 * Cin, a.Cin = Cin, a.ow = side, a.lnw = P, a.lnb = P + Cin, a.eps = eps;
      a.wt = P + 2 * (size_t)Cin, a.bias = a.wt + 4 * (size_t)C * Cin, a.OUT = C, a.out_nhwc = T;
      if (want()) ct_gemm<CT_SRC_LN4, CT_EPI_BIAS>(a, st);
      P = a.bias + C;
      float* t = X;
      X = T, T = t;
    }
    for (int j = 0; j < p.depths[i]; ++j) {
      float* chw = j + 1 == p.depths[i] ? (i == 0 ? res2 : i == 1 ? res3 : nullptr) : nullptr;
      const hipError_t e = ct_block(C, side, side, X, T, Hd, P, eps, X, chw, want, st);
      if (e != hipSuccess) return e;
      P += ct_block_floats(C);
    }
  }
  // head: LayerNorm over d3 in the staging of Linear(d3, E, bias = False), channel-major out
  {
    const int d3 = p.dims[3];
    ct_gemm_args a{};
    a.src = X, a.NP = side * side, a.K = d3, a.Cin = d3, a.lnw = P, a.lnb = P + d3, a.eps = eps;
    a.wt = P + 2 * (size_t)d3, a.OUT = p.embed_dim, a.out_chw = vis;
    if (want()) ct_gemm<CT_SRC_LN1, CT_EPI_HEAD>(a, st);
  }
  return hipSuccess;
}

}  // namespace olsr
