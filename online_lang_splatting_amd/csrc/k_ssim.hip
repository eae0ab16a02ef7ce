// k_ssim.hip — the colour-refinement loss (1 - lambda) L1 + lambda (1 - SSIM) and its gradient w.r.t. the rendered image.
//
// Caller side of the rasterizer path, third loop of the reference's back end (utils/slam_backend.py:769-819).  Replaces
// l1_loss + ssim (gaussian_splatting/utils/loss_utils.py:21-22, 42-101: 11-tap Gaussian window, sigma 1.5, conv2d with zero
// padding 5, per channel, C1 = 0.01^2, C2 = 0.03^2, mean over 3 H W) and the autograd backward of both.
//
// Two launches, one workgroup per 32 x 16 tile of one channel:
//   ssim_stats_kernel  stages the tile of image and target with a 5-pixel halo in LDS (zeros outside the image), blurs
//                      x, y, x^2, y^2, xy horizontally then vertically out of LDS (the window is separable), evaluates the
//                      SSIM map and writes, per pixel, the three derivatives of the map w.r.t. the blurred x, x^2 and xy
//                      into scratch planes; one partial {sum |x - y|, sum ssim} per workgroup.
//   ssim_grad_kernel   blurs the three planes once more (the window is symmetric: the adjoint of the zero-padded convolution
//                      is the same convolution) and combines dL/dx = k_ssim (blur(Dmu) + 2 x blur(Ds1) + y blur(Ds12)) +
//                      k_l1 sgn(x - y); its first workgroup also adds the partials in double -> loss[4].
// Without a gradient output the first kernel writes no planes and a one-block kernel does the final adds.
// Sums are deterministic: fixed-order wave / block trees, then one block adds the partials (as k_loss.hip).
//
// Precision.  Inputs, the SSIM map's arithmetic and every output are float32, but the window sums are ACCUMULATED IN DOUBLE
// (products of two float32 are exact there): sigma^2 = E[x^2] - mu^2 cancels almost completely on flat image regions, where
// neighbouring pixels round alike and a float32 accumulation leaves an error of one sign over the whole region - measured on
// a constant region with 0.2 % noise (tests/golden/ssim.npz, case 2) an all-float32 evaluation of this kernel's expression
// misses the SSIM value by 1.5e-5, fifteen times the reference's own float32 error there, and with double sums by 7e-9.
// -ffp-contract=off holds for this unit like the others; the window sums say fma() themselves.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_loss_device.h"

namespace olsr {

constexpr int SSIM_THREADS = 256;
constexpr int SSIM_R = 5;                      // window radius
constexpr int SSIM_TW = 32, SSIM_TH = 16;      // output tile
constexpr int SSIM_LH = SSIM_TH + 2 * SSIM_R;  // staged rows: y0 - 5 .. y0 + 20
constexpr int SSIM_LW = 48;                    // staged columns: x0 - 8 .. x0 + 39 (whole 16-byte groups; 42 are used)
constexpr int SSIM_X0 = 8 - SSIM_R;            // staged column of the first tap of output column 0
constexpr int SSIM_HN = SSIM_LH * SSIM_TW;     // horizontally blurred values per map

// gaussian(11, 1.5) of the reference: exp(-(i - 5)^2 / 4.5) stored and normalised in float32 (loss_utils.py:42-49).
// tests/test_ssim_ref_golden.py reads these eleven literals and compares them with that formula.
__device__ __forceinline__ float ssim_weight(int k) {
  constexpr float SSIM_WINDOW[11] = {1.0283801e-03f, 7.598758e-03f, 3.6000773e-02f, 1.0936069e-01f, 2.1300553e-01f, 2.6601171e-01f,
                                     2.1300553e-01f, 1.0936069e-01f, 3.6000773e-02f, 7.598758e-03f, 1.0283801e-03f};
  return SSIM_WINDOW[k];
}

// rows y0 - 5 .. y0 + 20, columns x0 - 8 .. x0 + 39 of one plane -> tile[SSIM_LH][SSIM_LW], zeros outside the image.
// VEC4 (W % 4 == 0 and a 16-byte aligned plane; x0 is a multiple of 32): a group of four columns lies inside or outside as one.
template <bool VEC4>
__device__ __forceinline__ void ssim_stage(const float* __restrict__ plane, int W, int H, int x0, int y0,
                                           float* __restrict__ tile) {
  if constexpr (VEC4) {
    for (int i = threadIdx.x; i < SSIM_LH * (SSIM_LW / 4); i += SSIM_THREADS) {
      const int r = i / (SSIM_LW / 4), q = i % (SSIM_LW / 4);
      const int y = y0 - SSIM_R + r, x = x0 - 8 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y >= 0 && y < H && x >= 0 && x < W) v = *reinterpret_cast<const float4*>(plane + (size_t)y * W + x);
      *reinterpret_cast<float4*>(tile + r * SSIM_LW + 4 * q) = v;
    }
  } else {
    for (int i = threadIdx.x; i < SSIM_LH * SSIM_LW; i += SSIM_THREADS) {
      const int r = i / SSIM_LW, c = i % SSIM_LW;
      const int y = y0 - SSIM_R + r, x = x0 - 8 + c;
      tile[i] = (y >= 0 && y < H && x >= 0 && x < W) ? plane[(size_t)y * W + x] : 0.f;
    }
  }
}

// The reference's 2-D window is the float32-ROUNDED outer product fl(w_i w_j) (loss_utils.py:52-54), which is not separable:
// its 121 weights sum to 1 - 6.94e-8, the exact products w_i w_j to 1 - 6.24e-8.  The difference is a gain of the whole window,
// and a gain does not cancel in SSIM: on a flat region sigma^2 = E[x^2] - mu^2 = c^2 (S - S^2) for a window of sum S, small
// against nothing but C2.  Measured at 1200 x 680 on a smooth image with 2 % noise, in float64: the exact products miss the
// reference's SSIM by 7.9e-7, the exact products times this gain by 1e-10 (what is left is the zero-mean part of the rounding,
// which only sees the image's high frequencies).  SSIM_GAIN = sum_ij fl(w_i w_j) / (sum_i w_i)^2, checked by
// tests/test_ssim_ref_golden.py from the formula.
constexpr double SSIM_GAIN = 0.9999999929559621;

// the vertical pass of one output pixel out of a horizontally blurred map [SSIM_LH][SSIM_TW]
__device__ __forceinline__ double ssim_vblur(const double* __restrict__ hb, int row, int col) {
  double a = 0.0;
#pragma unroll
  for (int k = 0; k < 2 * SSIM_R + 1; ++k) a = fma((double)ssim_weight(k), hb[(row + k) * SSIM_TW + col], a);
  return a * SSIM_GAIN;
}

template <bool VEC4, bool GRAD>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_stats_kernel(int W, int H, const float* __restrict__ image,
                                                                  const float* __restrict__ gt,
                                                                  float* __restrict__ planes,
                                                                  double* __restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sx[SSIM_LH * SSIM_LW];
  __shared__ __attribute__((aligned(16))) float sy[SSIM_LH * SSIM_LW];
  __shared__ double hb[5][SSIM_HN];
  __shared__ double red[SSIM_THREADS / 64][2];
  const int x0 = blockIdx.x * SSIM_TW, y0 = blockIdx.y * SSIM_TH, c = blockIdx.z;
  const size_t HW = (size_t)H * W;
  ssim_stage<VEC4>(image + c * HW, W, H, x0, y0, sx);
  ssim_stage<VEC4>(gt + c * HW, W, H, x0, y0, sy);
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_HN; i += SSIM_THREADS) {
    const int r = i / SSIM_TW, col = i % SSIM_TW;
    const float* px = sx + r * SSIM_LW + col + SSIM_X0;
    const float* py = sy + r * SSIM_LW + col + SSIM_X0;
    double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
    for (int k = 0; k < 2 * SSIM_R + 1; ++k) {
      const double w = (double)ssim_weight(k), xv = (double)px[k], yv = (double)py[k];
      a = fma(w, xv, a);
      b = fma(w, yv, b);
      aa = fma(w, xv * xv, aa);
      bb = fma(w, yv * yv, bb);
      ab = fma(w, xv * yv, ab);
    }
    hb[0][i] = a;
    hb[1][i] = b;
    hb[2][i] = aa;
    hb[3][i] = bb;
    hb[4][i] = ab;
  }
  __syncthreads();
  double s_l1 = 0.0, s_ssim = 0.0;
#pragma unroll
  for (int j = 0; j < SSIM_TW * SSIM_TH / SSIM_THREADS; ++j) {
    const int col = threadIdx.x % SSIM_TW, row = threadIdx.x / SSIM_TW + j * (SSIM_THREADS / SSIM_TW);
    const int x = x0 + col, y = y0 + row;
    if (x < W && y < H) {
      const double mu1d = ssim_vblur(hb[0], row, col), mu2d = ssim_vblur(hb[1], row, col);
      const double e11 = ssim_vblur(hb[2], row, col), e22 = ssim_vblur(hb[3], row, col), e12 = ssim_vblur(hb[4], row, col);
      const float C1 = 1e-4f, C2 = 9e-4f;
      const float mu1 = (float)mu1d, mu2 = (float)mu2d;
      const float mu1_sq = (float)(mu1d * mu1d), mu2_sq = (float)(mu2d * mu2d), mu12 = (float)(mu1d * mu2d);
      const float s1 = (float)(e11 - mu1d * mu1d), s2 = (float)(e22 - mu2d * mu2d), s12 = (float)(e12 - mu1d * mu2d);
      const float A1 = 2.f * mu12 + C1, A2 = 2.f * s12 + C2;
      const float B1 = (mu1_sq + mu2_sq) + C1, B2 = (s1 + s2) + C2;
      const float num = A1 * A2, den = B1 * B2;
      const float m = num / den;
      s_ssim += (double)m;
      s_l1 += (double)fabsf(sx[(row + SSIM_R) * SSIM_LW + col + 8] - sy[(row + SSIM_R) * SSIM_LW + col + 8]);
      if constexpr (GRAD) {
        // the chain rule in the grouping autograd takes through the reference's expression: with identical images the
        // large terms of d m / d mu1 cancel the same way, and 2 x Ds1 + y Ds12 cancels exactly
        const float g_num = 1.f / den, g_den = -(m / den);
        const float gA1 = g_num * A2, gA2 = g_num * A1, gB1 = g_den * B2, gB2 = g_den * B1;
        const float d_s12 = 2.f * gA2;  // d m / d sigma12
        const float d_s1 = gB2;         // d m / d sigma1^2
        // d m / d mu1 with blur(x^2), blur(xy) held fixed: through mu1 mu2 (A1 and sigma12) and mu1^2 (B1 and sigma1^2)
        const float d_mu = (2.f * gA1 - d_s12) * mu2 + (gB1 - d_s1) * (2.f * mu1);
        const size_t p = c * HW + (size_t)y * W + x;
        planes[p] = d_mu;
        planes[3 * HW + p] = d_s1;
        planes[6 * HW + p] = d_s12;
      }
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  s_l1 = wave_sum(s_l1);
  s_ssim = wave_sum(s_ssim);
  if (lane == 0) {
    red[w][0] = s_l1;
    red[w][1] = s_ssim;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int k = threadIdx.x;
    const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[2 * b + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  }
}

struct SsimFinalArgs {
  const double* partials;  // [nb][2]
  int nb, W, H;
  float lambda;
  float* loss;  // {total, (1 - lambda) L1, lambda (1 - SSIM), SSIM}
};

// one 256-thread block: the partials in double, fixed order
__device__ __forceinline__ void ssim_final_block(const SsimFinalArgs& a, double (*red)[2]) {
  double acc[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < a.nb; b += SSIM_THREADS) {
    acc[0] += a.partials[2 * (size_t)b];
    acc[1] += a.partials[2 * (size_t)b + 1];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[w][k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n = 3.0 * (double)a.H * (double)a.W;
    const double l1 = ((red[0][0] + red[1][0]) + (red[2][0] + red[3][0])) / n;
    const double ssim = ((red[0][1] + red[1][1]) + (red[2][1] + red[3][1])) / n;
    const double t_l1 = (1.0 - (double)a.lambda) * l1, t_ssim = (double)a.lambda * (1.0 - ssim);
    a.loss[0] = (float)(t_l1 + t_ssim);
    a.loss[1] = (float)t_l1;
    a.loss[2] = (float)t_ssim;
    a.loss[3] = (float)ssim;
  }
}

__global__ __launch_bounds__(SSIM_THREADS) void ssim_final_kernel(const SsimFinalArgs a) {
  __shared__ double red[SSIM_THREADS / 64][2];
  ssim_final_block(a, red);
}

template <bool VEC4>
__global__ __launch_bounds__(SSIM_THREADS) void ssim_grad_kernel(int W, int H, float k_ssim, float k_l1,
                                                                 const float* __restrict__ image,
                                                                 const float* __restrict__ gt,
                                                                 const float* __restrict__ planes,
                                                                 float* __restrict__ d_image, const SsimFinalArgs fin) {
  __shared__ __attribute__((aligned(16))) float sp[3][SSIM_LH * SSIM_LW];
  __shared__ double hb[3][SSIM_HN];
  __shared__ double red[SSIM_THREADS / 64][2];
  const int x0 = blockIdx.x * SSIM_TW, y0 = blockIdx.y * SSIM_TH, c = blockIdx.z;
  const size_t HW = (size_t)H * W;
#pragma unroll
  for (int q = 0; q < 3; ++q) ssim_stage<VEC4>(planes + (3 * q + c) * HW, W, H, x0, y0, sp[q]);
  __syncthreads();
  for (int i = threadIdx.x; i < SSIM_HN; i += SSIM_THREADS) {
    const int r = i / SSIM_TW, col = i % SSIM_TW;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float* p = sp[q] + r * SSIM_LW + col + SSIM_X0;
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < 2 * SSIM_R + 1; ++k) a = fma((double)ssim_weight(k), (double)p[k], a);
      hb[q][i] = a;
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SSIM_TW * SSIM_TH / SSIM_THREADS; ++j) {
    const int col = threadIdx.x % SSIM_TW, row = threadIdx.x / SSIM_TW + j * (SSIM_THREADS / SSIM_TW);
    const int x = x0 + col, y = y0 + row;
    if (x < W && y < H) {
      const float g_mu = (float)ssim_vblur(hb[0], row, col), g_s1 = (float)ssim_vblur(hb[1], row, col),
                  g_s12 = (float)ssim_vblur(hb[2], row, col);
      const size_t p = c * HW + (size_t)y * W + x;
      const float xv = image[p], yv = gt[p];
      const float d_ssim = (g_mu + (2.f * xv) * g_s1) + yv * g_s12;  // d (sum of the SSIM map) / d x
      d_image[p] = k_ssim * d_ssim + k_l1 * loss_sgn(xv - yv);
    }
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) ssim_final_block(fin, red);
}

static inline dim3 ssim_grid(int W, int H) { return dim3((W + SSIM_TW - 1) / SSIM_TW, (H + SSIM_TH - 1) / SSIM_TH, 3); }

struct SsimScratch {
  double* partials;  // [2 per block]
  float* planes;     // Dmu[3,H,W] | Ds1[3,H,W] | Ds12[3,H,W]: the kernels index all three from this one pointer
  static SsimScratch carve(void* buf, int W, int H, size_t& bytes) {
    Carver c(buf);
    const dim3 g = ssim_grid(W, H);
    SsimScratch s;
    s.partials = c.take<double>((size_t)g.x * g.y * g.z * 2);
    s.planes = c.take<float>((size_t)9 * H * W);
    bytes = c.total();
    return s;
  }
};

size_t refinement_loss_scratch_bytes(int W, int H) {
  size_t bytes = 0;
  SsimScratch::carve(nullptr, W > 0 ? W : 0, H > 0 ? H : 0, bytes);
  return bytes;
}

void launch_refinement_loss(int W, int H, float lambda, const float* image, const float* gt_image, float* dL_dimage,
                            float* loss, void* scratch, hipStream_t st) {
  size_t bytes;
  const SsimScratch sc = SsimScratch::carve(scratch, W, H, bytes);
  double* partials = sc.partials;
  float* planes = sc.planes;
  const dim3 grid = ssim_grid(W, H);
  auto al16 = [](const void* q) { return ((uintptr_t)q & 15u) == 0; };
  const bool vec4 = (W % 4) == 0 && al16(image) && al16(gt_image);  // (the planes are 256-byte aligned)
  SsimFinalArgs fin{partials, (int)(grid.x * grid.y * grid.z), W, H, lambda, loss};
  if (dL_dimage == nullptr) {
    if (vec4)
      ssim_stats_kernel<true, false><<<grid, SSIM_THREADS, 0, st>>>(W, H, image, gt_image, planes, partials);
    else
      ssim_stats_kernel<false, false><<<grid, SSIM_THREADS, 0, st>>>(W, H, image, gt_image, planes, partials);
    ssim_final_kernel<<<1, SSIM_THREADS, 0, st>>>(fin);
    return;
  }
  const double n = 3.0 * (double)H * (double)W;
  const float k_ssim = (float)(-(double)lambda / n), k_l1 = (float)((1.0 - (double)lambda) / n);
  if (vec4) {
    ssim_stats_kernel<true, true><<<grid, SSIM_THREADS, 0, st>>>(W, H, image, gt_image, planes, partials);
    ssim_grad_kernel<true><<<grid, SSIM_THREADS, 0, st>>>(W, H, k_ssim, k_l1, image, gt_image, planes, dL_dimage, fin);
  } else {
    ssim_stats_kernel<false, true><<<grid, SSIM_THREADS, 0, st>>>(W, H, image, gt_image, planes, partials);
    ssim_grad_kernel<false><<<grid, SSIM_THREADS, 0, st>>>(W, H, k_ssim, k_l1, image, gt_image, planes, dL_dimage, fin);
  }
}

}  // namespace olsr
