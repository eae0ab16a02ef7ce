// k_lang_ae.hip — the online language autoencoder: one training step, encode and decode.
//
// Caller side of the mapping loop.  BackEnd.train_online_autoencoder (utils/slam_backend.py:266-323) trains
// EncoderDecoderOnline (language/autoencoder/model.py:314-354; Linear 32->24, ReLU, Linear 24->15 | Linear 15->24, ReLU,
// Linear 24->32, each half followed by x / x.norm(dim=-1), no epsilon) on a keyframe's N x 32 feature rows with
//     loss = mean_{N 32}|r - x| + 0.6 (1 - mean_N cos(r, x)),  r = decode(encode(x)),  cos = F.cosine_similarity(dim=1, eps=1e-8)
// as zero_grad / forward / autograd backward / torch.optim.Adam.step: several dozen launches and a host read.  Here:
//   lang_ae_grad_kernel   one row per lane, 256 rows per workgroup.  Forward, loss and the backward to every layer's
//                         pre-activation in registers (every loop is unrolled; the 2 351 parameters are read through uniform
//                         addresses).  Layer by layer, last first, the lanes put {cotangent, layer input, 1} of their rows into
//                         LDS and every thread walks the 256 rows for its own (at most four) elements of that layer's weight and
//                         bias gradient: float32 sums over the workgroup's rows in a fixed order, written as this workgroup's partial.
//   lang_ae_adam_kernel   one thread per parameter: the partials are added across workgroups in DOUBLE in workgroup order, rounded
//                         once to float32 (the gradient autograd would hand to Adam), and the parameter takes torch's single-tensor
//                         Adam step, operation for operation as k_adam.hip: the unfused float32 sequence, bit for bit its
//                         restatement tests/adam_ref.py on the recorded gradient (torch's CPU build fuses some of the
//                         multiply-adds and agrees to rounding only).  Its first workgroup also adds the loss partials.
// No atomics: every sum has a fixed order, so a step is bit-reproducible.  The step count lives on the device (as in k_pose.hip).
//
// Decisions autograd makes and this kernel repeats: relu'(0) = 0 (a unit whose pre-activation is <= 0 passes nothing),
// sgn(0) = 0 for a residual r - x that is exactly zero.  cosine_similarity clamps each norm at eps and divides the rows before
// their product is summed; its gradient is taken through the unclamped norm, as autograd does for a norm above eps.
// -ffp-contract=off holds for this unit like the others; every fma is written out.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_lang_ae_device.h"  // the parameter layout AE_W1 .. AE_B4, ae_encode, ae_decode, ae_store_codes

namespace olsr {

constexpr int AE_ROWS = 256;     // rows per workgroup = threads per workgroup
constexpr int AE_STRIDE = 57;    // LDS floats per row: odd (lane-strided writes hit 64 different banks), >= OUT + IN + 1
constexpr int AE_PSTRIDE = 2352; // floats per workgroup partial

// dx = W^T dy
template <int OUT, int IN>
__device__ __forceinline__ void ae_linear_t(const float* __restrict__ W, const float (&dy)[OUT], float (&dx)[IN]) {
#pragma unroll
  for (int i = 0; i < IN; ++i) dx[i] = 0.f;
#pragma unroll
  for (int o = 0; o < OUT; ++o)
#pragma unroll
    for (int i = 0; i < IN; ++i) dx[i] = fmaf(W[o * IN + i], dy[o], dx[i]);
}

// the cotangent of v given the cotangent du of u = v / |v|:  (du - u (u . du)) / |v|
template <int K>
__device__ __forceinline__ void ae_unit_bwd(const float (&u)[K], float n, float (&du)[K]) {
  float d = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) d = fmaf(u[k], du[k], d);
#pragma unroll
  for (int k = 0; k < K; ++k) du[k] = (du[k] - u[k] * d) / n;
}

__device__ __forceinline__ void ae_load_row(const float* __restrict__ features, int row, bool valid, bool vec4,
                                            float (&x)[AE_IN]) {
  if (!valid) {
#pragma unroll
    for (int k = 0; k < AE_IN; ++k) x[k] = 0.f;
  } else if (vec4) {
    const float4* p = reinterpret_cast<const float4*>(features + (size_t)row * AE_IN);
#pragma unroll
    for (int q = 0; q < AE_IN / 4; ++q) {
      const float4 v = p[q];
      x[4 * q] = v.x, x[4 * q + 1] = v.y, x[4 * q + 2] = v.z, x[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < AE_IN; ++k) x[k] = features[(size_t)row * AE_IN + k];
  }
}

// One layer's parameter gradient over the workgroup's rows.  Every lane stores {cot[OUT] | in[IN] | 1} of its row; thread t then
// owns elements e = t, t + 256, ... of [W (OUT x IN) | b (OUT)], which are contiguous in the flat array, and adds
// cot[row][o] * in[row][i] over the rows, each quarter of the rows in row order, the four quarters pairwise (the bias reads
// the 1).  Rows beyond N store zeros.
template <int OUT, int IN>
__device__ __forceinline__ void ae_param_grad(float* __restrict__ lds, const float (&cot)[OUT], const float (&in)[IN], bool valid,
                                              float* __restrict__ partial) {
  static_assert(OUT + IN + 1 <= AE_STRIDE, "LDS row");
  constexpr int E = OUT * (IN + 1), NE = (E + AE_ROWS - 1) / AE_ROWS;
  const int t = threadIdx.x;
  __syncthreads();  // the previous layer's walk is over
  float* mine = lds + t * AE_STRIDE;
#pragma unroll
  for (int o = 0; o < OUT; ++o) mine[o] = valid ? cot[o] : 0.f;
#pragma unroll
  for (int i = 0; i < IN; ++i) mine[OUT + i] = valid ? in[i] : 0.f;
  mine[OUT + IN] = 1.f;
  __syncthreads();
  int oc[NE], ic[NE];
  float acc[NE][4];  // four quarter sums (rows q * 64 ..): shorter rounding chains than one sum of 256, and independent fmas
#pragma unroll
  for (int j = 0; j < NE; ++j) {
    const int e = min(t + j * AE_ROWS, E - 1);
    oc[j] = e < OUT * IN ? e / IN : e - OUT * IN;
    ic[j] = OUT + (e < OUT * IN ? e % IN : IN);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[j][q] = 0.f;
  }
#pragma unroll 4
  for (int r = 0; r < AE_ROWS / 4; ++r) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float* row = lds + (q * (AE_ROWS / 4) + r) * AE_STRIDE;
#pragma unroll
      for (int j = 0; j < NE; ++j) acc[j][q] = fmaf(row[oc[j]], row[ic[j]], acc[j][q]);
    }
  }
#pragma unroll
  for (int j = 0; j < NE; ++j)
    if (t + j * AE_ROWS < E) partial[t + j * AE_ROWS] = (acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3]);
}

struct LangAeScalars {
  float k_l1, k_cos;  // 1 / (32 N), -0.6 / N: the cotangents of the two means
  float one_minus_beta1, beta2, one_minus_beta2, bias_correction2_sqrt, eps, neg_step;
  int step_on_device;
  double beta1_d, beta2_d, lr_d;
};

__global__ __launch_bounds__(AE_ROWS) void lang_ae_grad_kernel(int N, int vec4, const float* __restrict__ features,
                                                               const float* __restrict__ P, float k_l1, float k_cos,
                                                               float* __restrict__ codes, int code_layout,
                                                               float* __restrict__ partials, double* __restrict__ loss_partials,
                                                               int32_t* __restrict__ step_dev) {
  __shared__ float lds[AE_ROWS * AE_STRIDE];
  __shared__ double red[AE_ROWS / 64][2];
  const int t = threadIdx.x, row = blockIdx.x * AE_ROWS + t;
  const bool valid = row < N;
  if (blockIdx.x == 0 && t == 0 && step_dev != nullptr) step_dev[0] = step_dev[0] + 1;  // read by lang_ae_adam_kernel only
  float x[AE_IN], h1[AE_H], c[AE_C], h2[AE_H], r[AE_IN];
  ae_load_row(features, row, valid, vec4 != 0, x);
  const float nz = ae_encode(P, x, h1, c);
  if (valid && codes != nullptr) ae_store_codes(codes, code_layout, N, row, c);
  const float ny = ae_decode(P, c, h2, r);
  // loss of the row and d loss / d r
  float dr[AE_IN];
  float l1 = 0.f, cosv = 0.f;
  {
    const float nr_raw = lane_norm<AE_IN>(r), nx_raw = lane_norm<AE_IN>(x);
    const float nr = fmaxf(nr_raw, 1e-8f), nx = fmaxf(nx_raw, 1e-8f);
    float rn[AE_IN], xn[AE_IN];
#pragma unroll
    for (int k = 0; k < AE_IN; ++k) {
      rn[k] = r[k] / nr;
      xn[k] = x[k] / nx;
      cosv = fmaf(rn[k], xn[k], cosv);
      l1 += fabsf(r[k] - x[k]);
    }
#pragma unroll
    for (int k = 0; k < AE_IN; ++k) {
      const float d = r[k] - x[k];
      const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      dr[k] = fmaf(k_cos, (xn[k] - rn[k] * cosv) / nr, k_l1 * sg);
    }
  }
  float* partial = partials + (size_t)blockIdx.x * AE_PSTRIDE;
  // decoder, second layer:  y = W4 h2 + b4
  ae_unit_bwd<AE_IN>(r, ny, dr);  // dr is now d loss / d y
  ae_param_grad<AE_IN, AE_H>(lds, dr, h2, valid, partial + AE_W4);
  float dh[AE_H];
  ae_linear_t<AE_IN, AE_H>(P + AE_W4, dr, dh);
#pragma unroll
  for (int k = 0; k < AE_H; ++k) dh[k] = h2[k] > 0.f ? dh[k] : 0.f;
  // decoder, first layer:  a2 = W3 c + b3
  ae_param_grad<AE_H, AE_C>(lds, dh, c, valid, partial + AE_W3);
  float dc[AE_C];
  ae_linear_t<AE_H, AE_C>(P + AE_W3, dh, dc);
  // encoder, second layer:  z = W2 h1 + b2
  ae_unit_bwd<AE_C>(c, nz, dc);  // dc is now d loss / d z
  ae_param_grad<AE_C, AE_H>(lds, dc, h1, valid, partial + AE_W2);
  ae_linear_t<AE_C, AE_H>(P + AE_W2, dc, dh);
#pragma unroll
  for (int k = 0; k < AE_H; ++k) dh[k] = h1[k] > 0.f ? dh[k] : 0.f;
  // encoder, first layer:  a1 = W1 x + b1
  ae_param_grad<AE_H, AE_IN>(lds, dh, x, valid, partial + AE_W1);
  // the row's loss terms: wave tree, then the four waves in order
  double s_l1 = valid ? (double)l1 : 0.0, s_cos = valid ? (double)cosv : 0.0;
  s_l1 = wave_sum(s_l1);
  s_cos = wave_sum(s_cos);
  if ((t & 63) == 0) {
    red[t >> 6][0] = s_l1;
    red[t >> 6][1] = s_cos;
  }
  __syncthreads();
  if (t < 2) loss_partials[2 * (size_t)blockIdx.x + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

__global__ __launch_bounds__(256) void lang_ae_adam_kernel(int N, int nb, LangAeScalars hp, const float* __restrict__ partials,
                                                           const double* __restrict__ loss_partials,
                                                           const int32_t* __restrict__ step_dev, float* __restrict__ P,
                                                           float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                           float* __restrict__ grad_out, float* __restrict__ loss) {
  __shared__ double red[4][2];
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < AE_NP) {
    double g = 0.0;
    for (int b = 0; b < nb; ++b) g += (double)partials[(size_t)b * AE_PSTRIDE + e];
    const float grad = (float)g;
    if (grad_out != nullptr) grad_out[e] = grad;
    if (hp.step_on_device) {
      const double step = (double)step_dev[0];  // already counted by lang_ae_grad_kernel
      const double bc1 = 1.0 - pow(hp.beta1_d, step);
      const double bc2 = 1.0 - pow(hp.beta2_d, step);
      hp.bias_correction2_sqrt = (float)sqrt(bc2);
      hp.neg_step = (float)(-(hp.lr_d / bc1));
    }
    float m = exp_avg[e], v = exp_avg_sq[e];
    m = m + (grad - m) * hp.one_minus_beta1;              // exp_avg.lerp_(grad, 1 - beta1)
    v = v * hp.beta2 + hp.one_minus_beta2 * grad * grad;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / hp.bias_correction2_sqrt + hp.eps;
    P[e] = P[e] + hp.neg_step * (m / denom);              // param.addcdiv_(exp_avg, denom, value=-step_size)
    exp_avg[e] = m;
    exp_avg_sq[e] = v;
  }
  if (blockIdx.x != 0) return;
  double acc[2] = {0.0, 0.0};
  for (int b = threadIdx.x; b < nb; b += 256) {
    acc[0] += loss_partials[2 * (size_t)b];
    acc[1] += loss_partials[2 * (size_t)b + 1];
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double v = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double l1 = ((red[0][0] + red[1][0]) + (red[2][0] + red[3][0])) / ((double)N * AE_IN);
    const double cs = ((red[0][1] + red[1][1]) + (red[2][1] + red[3][1])) / (double)N;
    const double t_cos = 0.6 * (1.0 - cs);
    loss[0] = (float)(l1 + t_cos);
    loss[1] = (float)l1;
    loss[2] = (float)t_cos;
    loss[3] = (float)cs;
  }
}

__global__ __launch_bounds__(AE_ROWS) void lang_ae_encode_kernel(int N, int vec4, const float* __restrict__ features,
                                                                 const float* __restrict__ P, float* __restrict__ codes,
                                                                 int code_layout) {
  const int row = blockIdx.x * AE_ROWS + threadIdx.x;
  if (row >= N) return;
  float x[AE_IN], h1[AE_H], c[AE_C];
  ae_load_row(features, row, true, vec4 != 0, x);
  ae_encode(P, x, h1, c);
  ae_store_codes(codes, code_layout, N, row, c);
}

__global__ __launch_bounds__(AE_ROWS) void lang_ae_decode_kernel(int N, const float* __restrict__ codes, int code_layout,
                                                                 const float* __restrict__ P, float* __restrict__ recon) {
  const int row = blockIdx.x * AE_ROWS + threadIdx.x;
  if (row >= N) return;
  float c[AE_C], h2[AE_H], r[AE_IN];
#pragma unroll
  for (int k = 0; k < AE_C; ++k)
    c[k] = code_layout == OLSR_LANG_AE_CODES_CHANNELS ? codes[(size_t)k * N + row] : codes[(size_t)row * AE_C + k];
  ae_decode(P, c, h2, r);
#pragma unroll
  for (int k = 0; k < AE_IN; ++k) recon[(size_t)row * AE_IN + k] = r[k];
}

static inline int ae_blocks(int N) { return (N + AE_ROWS - 1) / AE_ROWS; }
static inline bool ae_vec4(const float* features) { return ((uintptr_t)features & 15u) == 0; }

struct AeScratch {
  float* partials;        // [blocks][AE_PSTRIDE] gradient partials
  double* loss_partials;  // [blocks][2]
  static AeScratch carve(void* buf, int N, size_t& bytes) {
    Carver c(buf);
    AeScratch s;
    s.partials = c.take<float>((size_t)ae_blocks(N) * AE_PSTRIDE);
    s.loss_partials = c.take<double>((size_t)ae_blocks(N) * 2);
    bytes = c.total();
    return s;
  }
};

size_t lang_ae_scratch_bytes(int N) {
  size_t bytes = 0;
  AeScratch::carve(nullptr, N > 0 ? N : 0, bytes);
  return bytes;
}

void launch_lang_ae_train_step(const olsr_lang_ae_params& p, int N, const float* features, float* params, float* exp_avg,
                               float* exp_avg_sq, int32_t* step_dev, float* loss, float* codes, float* grad_out, void* scratch,
                               hipStream_t st) {
  size_t bytes;
  const AeScratch sc = AeScratch::carve(scratch, N, bytes);
  float* partials = sc.partials;
  double* loss_partials = sc.loss_partials;
  const int nb = ae_blocks(N);
  LangAeScalars k{};
  k.k_l1 = (float)(1.0 / ((double)N * AE_IN));
  k.k_cos = (float)(-0.6 / (double)N);
  // torch/optim/adam.py, _single_tensor_adam: Python-float (double) arithmetic for every scalar
  const int step = p.step > 0 ? p.step : 1;
  const double bc1 = 1.0 - pow(p.beta1, (double)step);
  const double bc2 = 1.0 - pow(p.beta2, (double)step);
  k.one_minus_beta1 = (float)(1.0 - p.beta1);
  k.beta2 = (float)p.beta2;
  k.one_minus_beta2 = (float)(1.0 - p.beta2);
  k.bias_correction2_sqrt = (float)sqrt(bc2);
  k.eps = (float)p.eps;
  k.neg_step = (float)(-(p.lr / bc1));
  k.step_on_device = p.step <= 0 ? 1 : 0;
  k.beta1_d = p.beta1;
  k.beta2_d = p.beta2;
  k.lr_d = p.lr;
  lang_ae_grad_kernel<<<nb, AE_ROWS, 0, st>>>(N, ae_vec4(features) ? 1 : 0, features, params, k.k_l1, k.k_cos, codes,
                                              p.code_layout, partials, loss_partials, step_dev);
  lang_ae_adam_kernel<<<(AE_NP + 255) / 256, 256, 0, st>>>(N, nb, k, partials, loss_partials, step_dev, params, exp_avg,
                                                           exp_avg_sq, grad_out, loss);
}

void launch_lang_ae_encode(int N, const float* features, const float* params, int code_layout, float* codes, hipStream_t st) {
  lang_ae_encode_kernel<<<ae_blocks(N), AE_ROWS, 0, st>>>(N, ae_vec4(features) ? 1 : 0, features, params, codes, code_layout);
}

void launch_lang_ae_decode(int N, const float* codes, const float* params, int code_layout, float* recon, hipStream_t st) {
  lang_ae_decode_kernel<<<ae_blocks(N), AE_ROWS, 0, st>>>(N, codes, code_layout, params, recon);
}

}  // namespace olsr
