// k_hr_net.hip — the high-resolution language feature net (language/supervisedNet.py:6-109, HighResLanguageFeatureNet in eval()).
//
// The reference turns the backbone's three maps (clip_vis_dense [768,h,w], res3 [384,h3,w3], res2 [192,h2,w2]) into the
// [768,8h,8w] map the general encoder reads with thirteen convolutions in torch ops, two resized copies, two concatenated copies
// and a BatchNorm / ReLU / sigmoid / gate pass over every intermediate.  Here one implicit-GEMM kernel template on
// v_mfma_f32_16x16x4_f32, launched thirteen times:
//   hr_conv_kernel<TAPS, SRC, EPI>   a workgroup of four waves owns 64 output pixels x 64 output channels (16 per wave: four
//                         accumulator tiles that stay in registers across the whole K loop).  The weights are the A operand,
//                         one 16-byte load per lane and 16-deep k block straight from the packed array (a tap's [out][in] slab is
//                         contiguous), the next block's load issued ahead of the current block's MFMAs; the activations are the
//                         B operand out of an LDS image [pixel][32 channels + 4], double-buffered: the next chunk's global loads
//                         are issued before the current chunk's MFMAs and stored behind them (k_lang_encoder.hip's layer 1).  Operand
//                         layout and block: olsr_dense.h.
//     TAPS  1x1           64 consecutive pixels of the flattened plane.
//           3x3, pad 1    an 8 x 8 tile; a chunk of its 10 x 10 halo patch is staged once and the nine taps walk over it;
//                         what lies outside the image is staged as zeros.
//           transposed    one parity phase (py, px) of ConvTranspose2d(k 4, s 2, p 1) per workgroup (blockIdx.z): output
//                         (2m + py, 2n + px) is a 2x2 convolution of the input around (m, n).  From PyTorch's definition
//                         oy = 2 iy - 1 + ky:  iy = m + dy, ky = py + 1 - 2 dy, dy in {py - 1, py}; the same in x.  The tile is 8 x 8
//                         input pixels, the four phases together write every output pixel exactly once.
//     SRC   one tensor; two tensors one after the other along K (torch.cat([high, low], 1) without the copy); or one tensor
//           sampled bilinearly while it is staged (F.interpolate(mode='bilinear', align_corners=False) ahead of a 1x1: the
//           resize comes first, as in the reference, and no resized copy exists).
//     EPI   bias;  relu(fmaf(alpha, h, beta)) with BatchNorm2d's running statistics folded per channel as bn_fold does (in
//           double, rounded once; ReLU keeps a NaN);  or the gate fused * sigmoid(h) + fused as one fmaf, reading fused once.
// K order is fixed: chunks of 32 channels in order, inside a chunk the taps in order, inside a tap two 16-deep blocks.  No
// atomics, no split K: a value depends on its own receptive field only and a call is bit-reproducible.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_dense.h"

namespace olsr {

constexpr int HR_TP = 64;           // pixels per workgroup
constexpr int HR_TN = 64;           // output channels per workgroup, 16 per wave
constexpr int HR_THREADS = 256;
constexpr int HR_KC = 32;           // input channels per chunk
constexpr int HR_CS = HR_KC + 4;    // LDS floats per pixel (36: the float4 reads of 16 consecutive pixels hit 64 banks)

enum { HR_TAPS_1 = 0, HR_TAPS_3 = 1, HR_TAPS_T = 2 };
enum { HR_SRC_ONE = 0, HR_SRC_TWO = 1, HR_SRC_BILINEAR = 2 };
enum { HR_EPI_BIAS = 0, HR_EPI_BN = 1, HR_EPI_GATE = 2 };

// the packed array (include/olsr.h): per layer  taps x [out][in] | bias [out] | BatchNorm weight, bias, mean, var [4][out]
constexpr int HR_CV = 768, HR_C3 = 384, HR_C2 = 192, HR_A = 512, HR_B = 256, HR_C = 128, HR_CO = 768;
constexpr long long hr_layer(int taps, int out, int in, bool bn) { return (long long)taps * out * in + out + (bn ? 4 * out : 0); }
constexpr long long HR_L0 = 0;                                           // initial_conv
constexpr long long HR_L1 = HR_L0 + hr_layer(9, HR_A, HR_CV, true);      // upsample1
constexpr long long HR_L2 = HR_L1 + hr_layer(16, HR_A, HR_A, true);      // attention_fusion1.low_res_align
constexpr long long HR_L3 = HR_L2 + hr_layer(1, HR_A, HR_C3, false);     // attention_fusion1.fusion
constexpr long long HR_L4 = HR_L3 + hr_layer(9, HR_A, 2 * HR_A, true);   // attention_fusion1.attention.0
constexpr long long HR_L5 = HR_L4 + hr_layer(9, HR_A, HR_A, true);       // attention_fusion1.attention.3
constexpr long long HR_L6 = HR_L5 + hr_layer(1, HR_A, HR_A, false);      // upsample2
constexpr long long HR_L7 = HR_L6 + hr_layer(16, HR_B, HR_A, true);      // attention_fusion2.low_res_align
constexpr long long HR_L8 = HR_L7 + hr_layer(1, HR_B, HR_C2, false);     // attention_fusion2.fusion
constexpr long long HR_L9 = HR_L8 + hr_layer(9, HR_B, 2 * HR_B, true);   // attention_fusion2.attention.0
constexpr long long HR_L10 = HR_L9 + hr_layer(9, HR_B, HR_B, true);      // attention_fusion2.attention.3
constexpr long long HR_L11 = HR_L10 + hr_layer(1, HR_B, HR_B, false);    // upsample3
constexpr long long HR_L12 = HR_L11 + hr_layer(16, HR_C, HR_B, true);    // final_conv
constexpr long long HR_END = HR_L12 + hr_layer(1, HR_CO, HR_C, false);
static_assert(HR_END == OLSR_HR_NET_PARAMS, "packed layout of the HR net");

struct hr_conv_args {
  const float* src1;  // [C1] planes, ps1 apart
  const float* src2;  // [C2] planes behind them along K (HR_SRC_TWO)
  int ps1, ps2, C1, C2;
  int H, W;    // the grid the tiles walk: the output's (1x1, 3x3), the input's (transposed: the output is 2H x 2W)
  int sh, sw;  // the source's own size (HR_SRC_BILINEAR)
  const float* wt;    // taps x [OUT][C1 + C2]
  const float* bias;  // [OUT]
  const float* bn;    // [4][OUT] (HR_EPI_BN)
  double eps;
  const float* gate;  // [OUT] planes of the output's size (HR_EPI_GATE)
  int gate_ps;
  float* out;
  int out_ps, OUT;
};

template <int TAPS, int SRC, int EPI>
__global__ __launch_bounds__(HR_THREADS) void hr_conv_kernel(const hr_conv_args a) {
  static_assert(SRC != HR_SRC_BILINEAR || TAPS == HR_TAPS_1, "the resize is fused into a 1x1 only");
  constexpr int HALO = TAPS == HR_TAPS_1 ? 0 : 1;
  constexpr int TW = TAPS == HR_TAPS_1 ? HR_TP : 8, TH = HR_TP / TW;
  constexpr int PW = TW + 2 * HALO, PH = TH + 2 * HALO, HP = PW * PH;  // the staged patch
  constexpr int NE = (HP * HR_KC + HR_THREADS - 1) / HR_THREADS;       // staged elements per thread and chunk
  constexpr int NTAP = TAPS == HR_TAPS_1 ? 1 : TAPS == HR_TAPS_3 ? 9 : 4;
  __shared__ __attribute__((aligned(16))) float buf[2][HP * HR_CS];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, q = lane >> 4;
  const int NP = a.H * a.W, IN = a.C1 + a.C2;
  const int py = (int)(blockIdx.z >> 1), px = (int)(blockIdx.z & 1);
  int ty0 = 0, tx0 = 0;
  const int P0 = blockIdx.x * HR_TP;
  if (TAPS != HR_TAPS_1) {
    const int tiles_x = (a.W + TW - 1) / TW;
    ty0 = (blockIdx.x / tiles_x) * TH;
    tx0 = (blockIdx.x % tiles_x) * TW;
  }
  const int n0 = blockIdx.y * HR_TN + wave * 16;

  // ---- what this thread stages: element i is (patch pixel, channel) = (e % HP, e / HP), e = tid + 256 i -------------------
  int pix[NE];  // offset of the pixel inside a plane, -1: outside the image (a zero)
  int o00 = 0, o01 = 0, o10 = 0, o11 = 0;
  float ly = 0.f, lx = 0.f, hy = 1.f, hx = 1.f;
  if (SRC == HR_SRC_BILINEAR) {
    // upsample_bilinear2d, align_corners = False: src = max(scale (dst + 0.5) - 0.5, 0), scale = in / out in float
    const int P = P0 + (tid & (HR_TP - 1));
    pix[0] = P < NP ? 0 : -1;
    const int y = P < NP ? P / a.W : 0, x = P < NP ? P - y * a.W : 0;
    const float sy = fmaxf(((float)a.sh / (float)a.H) * ((float)y + 0.5f) - 0.5f, 0.f);
    const float sx = fmaxf(((float)a.sw / (float)a.W) * ((float)x + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)sy, a.sh - 1), x0 = min((int)sx, a.sw - 1);
    // (a dimension that keeps its size is copied, not interpolated, as torch does: the zero-weight neighbour is not read,
    // so a NaN stays in its own pixel)
    const int y1 = y0 + (a.sh != a.H && y0 < a.sh - 1 ? 1 : 0), x1 = x0 + (a.sw != a.W && x0 < a.sw - 1 ? 1 : 0);
    ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
    o00 = y0 * a.sw + x0, o01 = y0 * a.sw + x1, o10 = y1 * a.sw + x0, o11 = y1 * a.sw + x1;
  } else {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + HR_THREADS * i, hp = e % HP;
      if (TAPS == HR_TAPS_1) {
        pix[i] = P0 + hp < NP ? P0 + hp : -1;
      } else {
        const int yy = ty0 + hp / PW - HALO, xx = tx0 + hp % PW - HALO;
        pix[i] = (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ? yy * a.W + xx : -1;
      }
    }
  }
  float pre[NE];
  auto fetch = [&](int k0) {
    const float* s = a.src1;
    int ps = a.ps1;
    if (SRC == HR_SRC_TWO && k0 >= a.C1) s = a.src2, ps = a.ps2, k0 -= a.C1;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + HR_THREADS * i, c = e / HP;
      float v = 0.f;
      if (e < HP * HR_KC) {
        const float* p = s + (size_t)(k0 + c) * (size_t)ps;
        if (SRC == HR_SRC_BILINEAR) {
          if (pix[0] >= 0) v = hy * (hx * p[o00] + lx * p[o01]) + ly * (hx * p[o10] + lx * p[o11]);
        } else if (pix[i] >= 0) {
          v = p[pix[i]];
        }
      }
      pre[i] = v;
    }
  };
  auto park = [&](float* b) {
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int e = tid + HR_THREADS * i, c = e / HP, hp = e % HP;
      if (e < HP * HR_KC) b[hp * HR_CS + c] = pre[i];
    }
  };

  // ---- the taps: where in the patch a tap reads, and which [OUT][IN] slab of the packed weights it multiplies ------------------
  int tap_off[NTAP];   // in LDS floats
  int tap_slab[NTAP];
#pragma unroll
  for (int t = 0; t < NTAP; ++t) {
    int dy = 0, dx = 0, slab = 0;
    if (TAPS == HR_TAPS_3) dy = t / 3 - 1, dx = t % 3 - 1, slab = t;
    if (TAPS == HR_TAPS_T) {
      dy = (t >> 1) - 1 + py, dx = (t & 1) - 1 + px;
      slab = (py + 1 - 2 * dy) * 4 + (px + 1 - 2 * dx);
    }
    tap_off[t] = (dy * PW + dx) * HR_CS;
    tap_slab[t] = slab;
  }
  int base[4];  // the lane's pixel 16 pt + li inside the patch, in LDS floats, at its k offset 4 q
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int p = 16 * pt + li;
    base[pt] = ((p / TW + HALO) * PW + p % TW + HALO) * HR_CS + 4 * q;
  }

  // ---- K loop ----------------------------------------------------------------------------------------------------------------
  const size_t slab_stride = (size_t)a.OUT * (size_t)IN;
  const float* wp = a.wt + (size_t)(n0 + li) * (size_t)IN + 4 * q;
  f32x4 acc[1][4];
  {
    const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + n0 + 4 * q);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[0][pt] = bv;
  }
  const int nchunks = IN / HR_KC;
  f32x4 wa[1] = {*reinterpret_cast<const f32x4*>(wp + (size_t)tap_slab[0] * slab_stride)};
  fetch(0);
  park(buf[0]);
  __syncthreads();
#pragma unroll 1
  for (int ch = 0; ch < nchunks; ++ch) {
    const bool more = ch + 1 < nchunks;
    if (more) fetch((ch + 1) * HR_KC);
    const float* xb = buf[ch & 1];
#pragma unroll
    for (int t = 0; t < NTAP; ++t) {
#pragma unroll
      for (int kb = 0; kb < HR_KC; kb += 16) {
        // the next block's weights: the same tap's second half, the next tap, or the next chunk's first tap
        const bool last = t == NTAP - 1 && kb + 16 == HR_KC;
        const int tn = kb + 16 < HR_KC ? t : (t + 1 < NTAP ? t + 1 : 0);
        const int kn = last ? (more ? (ch + 1) * HR_KC : ch * HR_KC + kb) : ch * HR_KC + (kb + 16 < HR_KC ? kb + 16 : 0);
        const int tl = last && !more ? t : tn;
        const f32x4 wn = *reinterpret_cast<const f32x4*>(wp + (size_t)tap_slab[tl] * slab_stride + kn);
        f32x4 b[4];
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) b[pt] = *reinterpret_cast<const f32x4*>(xb + base[pt] + tap_off[t] + kb);
        dense_mfma_block<1>(wa, b, acc);
        wa[0] = wn;
      }
    }
    if (more) park(buf[(ch + 1) & 1]);  // last read before the previous barrier
    __syncthreads();
  }

  // ---- epilogue: lane (li, q) holds channels n0 + 4 q + {0..3} of pixel 16 pt + li ---------------------------------------------
  const int n = n0 + 4 * q;
  float al[4], be[4];
  if (EPI == HR_EPI_BN) {
    // bn_fold's arithmetic (olsr_dense.h), written out: through the call the compiler orders this epilogue's address
    // arithmetic differently, and upsample1 then measured 0.4 % slower (profiles/dense_core_ab.json)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double s = (double)a.bn[n + r] / sqrt((double)a.bn[3 * a.OUT + n + r] + a.eps);
      al[r] = (float)s;
      be[r] = (float)((double)a.bn[a.OUT + n + r] - (double)a.bn[2 * a.OUT + n + r] * s);
    }
  }
#pragma unroll
  for (int pt = 0; pt < 4; ++pt) {
    const int p = 16 * pt + li;
    int o = -1;  // the pixel's offset inside an output plane
    if (TAPS == HR_TAPS_1) {
      if (P0 + p < NP) o = P0 + p;
    } else {
      const int gy = ty0 + p / TW, gx = tx0 + p % TW;
      if (gy < a.H && gx < a.W) o = TAPS == HR_TAPS_3 ? gy * a.W + gx : (2 * gy + py) * (2 * a.W) + 2 * gx + px;
    }
    if (o < 0) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[0][pt][r];
      if (EPI == HR_EPI_BN) v = relu_keep_nan(fmaf(al[r], v, be[r]));
      if (EPI == HR_EPI_GATE) {
        const float f = a.gate[(size_t)(n + r) * (size_t)a.gate_ps + o];
        v = fmaf(f, 1.f / (1.f + expf(-v)), f);
      }
      a.out[(size_t)(n + r) * (size_t)a.out_ps + o] = v;
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------

// the workspace, in floats: X0 [512,h,w] | three buffers [512,2h,2w] | three buffers [256,4h,4w] | X3 [128,8h,8w]
size_t hr_net_workspace_bytes(long long h, long long w) {
  const long long hw = h * w;
  return (size_t)(HR_A * hw + 3 * HR_A * 4 * hw + 3 * HR_B * 16 * hw + HR_C * 64 * hw) * sizeof(float);
}

template <int TAPS, int SRC, int EPI>
static void hr_launch(const hr_conv_args& a, hipStream_t st) {
  dim3 grid;
  if (TAPS == HR_TAPS_1) grid = dim3((a.H * a.W + HR_TP - 1) / HR_TP, a.OUT / HR_TN, 1);
  else grid = dim3(((a.H + 7) / 8) * ((a.W + 7) / 8), a.OUT / HR_TN, TAPS == HR_TAPS_T ? 4 : 1);
  hr_conv_kernel<TAPS, SRC, EPI><<<grid, HR_THREADS, 0, st>>>(a);
}

static hr_conv_args hr_args(const float* src1, int ps1, int C1, const float* src2, int ps2, int C2, int H, int W, const float* P,
                            long long layer, int taps, int OUT, bool bn, double eps, float* out, int out_ps) {
  hr_conv_args a{};
  a.src1 = src1, a.ps1 = ps1, a.C1 = C1, a.src2 = src2, a.ps2 = ps2, a.C2 = C2, a.H = H, a.W = W, a.sh = H, a.sw = W;
  a.wt = P + layer;
  a.bias = a.wt + (size_t)taps * OUT * (C1 + C2);
  a.bn = bn ? a.bias + OUT : nullptr;
  a.eps = eps, a.out = out, a.out_ps = out_ps, a.OUT = OUT;
  return a;
}

void launch_hr_net(const olsr_hr_net_params& p, const float* fv, const float* f3, const float* f2, const float* P,
                   float* ws, float* out, hipStream_t st) {
  const int h = p.h, w = p.w, h1 = 2 * h, w1 = 2 * w, h2 = 4 * h, w2 = 4 * w, h3 = 8 * h, w3 = 8 * w;
  const int n0 = h * w, n1 = h1 * w1, n2 = h2 * w2, n3 = h3 * w3;
  float* X0 = ws;
  float* A1 = X0 + (size_t)HR_A * n0;
  float* B1 = A1 + (size_t)HR_A * n1;
  float* C1 = B1 + (size_t)HR_A * n1;
  float* A2 = C1 + (size_t)HR_A * n1;
  float* B2 = A2 + (size_t)HR_B * n2;
  float* C2 = B2 + (size_t)HR_B * n2;
  float* X3 = C2 + (size_t)HR_B * n2;
  const double eps = p.bn_eps;
  const uint32_t on = p.launches ? p.launches : 0xffffffffu;
  int k = 0;
  auto want = [&]() { return ((on >> k++) & 1u) != 0; };
  hr_conv_args a;
  // initial_conv: 3x3 768 -> 512, BN, ReLU
  a = hr_args(fv, (int)p.fv_stride, HR_CV, nullptr, 0, 0, h, w, P, HR_L0, 9, HR_A, true, eps, X0, n0);
  if (want()) hr_launch<HR_TAPS_3, HR_SRC_ONE, HR_EPI_BN>(a, st);
  // upsample1: ConvTranspose 512 -> 512, BN, ReLU
  a = hr_args(X0, n0, HR_A, nullptr, 0, 0, h, w, P, HR_L1, 16, HR_A, true, eps, A1, n1);
  if (want()) hr_launch<HR_TAPS_T, HR_SRC_ONE, HR_EPI_BN>(a, st);
  // attention_fusion1: low_res_align of the resized res3 | fusion of (x, aligned) | attention | gate
  a = hr_args(f3, (int)p.f3_stride, HR_C3, nullptr, 0, 0, h1, w1, P, HR_L2, 1, HR_A, false, eps, B1, n1);
  a.sh = p.h3, a.sw = p.w3;
  if (want()) hr_launch<HR_TAPS_1, HR_SRC_BILINEAR, HR_EPI_BIAS>(a, st);
  a = hr_args(A1, n1, HR_A, B1, n1, HR_A, h1, w1, P, HR_L3, 9, HR_A, true, eps, C1, n1);
  if (want()) hr_launch<HR_TAPS_3, HR_SRC_TWO, HR_EPI_BN>(a, st);
  a = hr_args(C1, n1, HR_A, nullptr, 0, 0, h1, w1, P, HR_L4, 9, HR_A, true, eps, A1, n1);
  if (want()) hr_launch<HR_TAPS_3, HR_SRC_ONE, HR_EPI_BN>(a, st);
  a = hr_args(A1, n1, HR_A, nullptr, 0, 0, h1, w1, P, HR_L5, 1, HR_A, false, eps, B1, n1);
  a.gate = C1, a.gate_ps = n1;
  if (want()) hr_launch<HR_TAPS_1, HR_SRC_ONE, HR_EPI_GATE>(a, st);
  // upsample2: ConvTranspose 512 -> 256
  a = hr_args(B1, n1, HR_A, nullptr, 0, 0, h1, w1, P, HR_L6, 16, HR_B, true, eps, A2, n2);
  if (want()) hr_launch<HR_TAPS_T, HR_SRC_ONE, HR_EPI_BN>(a, st);
  // attention_fusion2
  a = hr_args(f2, (int)p.f2_stride, HR_C2, nullptr, 0, 0, h2, w2, P, HR_L7, 1, HR_B, false, eps, B2, n2);
  a.sh = p.h2, a.sw = p.w2;
  if (want()) hr_launch<HR_TAPS_1, HR_SRC_BILINEAR, HR_EPI_BIAS>(a, st);
  a = hr_args(A2, n2, HR_B, B2, n2, HR_B, h2, w2, P, HR_L8, 9, HR_B, true, eps, C2, n2);
  if (want()) hr_launch<HR_TAPS_3, HR_SRC_TWO, HR_EPI_BN>(a, st);
  a = hr_args(C2, n2, HR_B, nullptr, 0, 0, h2, w2, P, HR_L9, 9, HR_B, true, eps, A2, n2);
  if (want()) hr_launch<HR_TAPS_3, HR_SRC_ONE, HR_EPI_BN>(a, st);
  a = hr_args(A2, n2, HR_B, nullptr, 0, 0, h2, w2, P, HR_L10, 1, HR_B, false, eps, B2, n2);
  a.gate = C2, a.gate_ps = n2;
  if (want()) hr_launch<HR_TAPS_1, HR_SRC_ONE, HR_EPI_GATE>(a, st);
  // upsample3: ConvTranspose 256 -> 128
  a = hr_args(B2, n2, HR_B, nullptr, 0, 0, h2, w2, P, HR_L11, 16, HR_C, true, eps, X3, n3);
  if (want()) hr_launch<HR_TAPS_T, HR_SRC_ONE, HR_EPI_BN>(a, st);
  // final_conv: 1x1 128 -> 768
  a = hr_args(X3, n3, HR_C, nullptr, 0, 0, h3, w3, P, HR_L12, 1, HR_CO, false, eps, out, (int)p.out_stride);
  if (want()) hr_launch<HR_TAPS_1, HR_SRC_ONE, HR_EPI_BIAS>(a, st);
}

}  // namespace olsr
