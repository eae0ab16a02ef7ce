// k_frontend.hip — the front end's once-per-frame work around the tracking loop (include/olsr.h, "front end: the frame step").
//
// The reference does it in PyTorch ops with host reads (utils/slam_frontend.py:577-676):
//   Camera.compute_grad_mask  utils/camera_utils.py:123-152   the tracking mask; on Replica a Python loop over 32 x 32 image
//                                                             blocks, five device operations each
//   get_median_depth          utils/slam_utils.py:168-179     boolean gather, median(), host read
//   is_keyframe, add_to_window, the small-window rule         utils/slam_frontend.py:279-430, 633-645: count_nonzero over
//                                                             P-long masks per window keyframe, 4 x 4 inverses, ~90 .item()s
// Here:
//   grad_mask_blocks   ONE launch: a workgroup per image block — the block's gray halo in LDS, its intensities written over the
//                      halo rows that are no longer read, the lower median by a radix select inside LDS, the 0 / 1 mask out;
//                      the margin pixels (raw intensity) in further workgroups of the same grid.  No global scratch.
//   grad_mask_global   intensities (as float bits) to scratch + first digit, the file's radix select, a threshold pass
//   median_depth       keys of the valid depths + first digit, the same select; median and count stay on the device
//   covisibility       one pass over n_touched and the K visibilities: |cur|, |cur & vis_k|, |vis_k| (integer atomics)
//   keyframe_decide    one wave: reads the counts and the median word on the device, writes one record for the host
// The select's steps — counting a key, flushing a histogram, narrowing to the rank's bucket — are olsr_select.h's, shared with
// k_keyframe_seed.hip.  Here they run in two forms: over keys in global scratch (select_hist_kernel / select_digit_kernel /
// launch_select, behind a key kernel that counts digit 0) and over a block's intensities in LDS (grad_mask_blocks_kernel).
// An element that takes no part is stored as FE_NO_KEY and kept out by select_count's `takes_part` argument.  The histograms
// are integer atomics — order-independent —, nothing else is atomic: two runs give the same bits.  The arithmetic is pinned
// statement by statement in include/olsr.h; the translation unit is compiled without FMA contraction (build.py).
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_select.h"

namespace olsr {

constexpr int FE_THREADS = 256;
constexpr int FE_WAVES = FE_THREADS / 64;
constexpr int FE_PER_THREAD = 16;                 // elements per thread of a pass over N
constexpr int FE_CHUNK = FE_THREADS * FE_PER_THREAD;
constexpr u32 FE_NO_KEY = 0xFFFFFFFFu;            // stored for an element that takes no part (no valid element's key: a NaN pattern)
constexpr int FE_GRID_BLOCKS = 32;                // the reference's 32 x 32 image blocks
constexpr int FE_COVIS_PER_THREAD = 8;

// ---- the radix select on float bits: the lower median (rank (n - 1) / 2) of the keys that take part ------------------------
// Keys are the bits of non-negative floats, whose unsigned order is the floats' order (+inf above every finite value).
struct SelectState {
  u32 prefix;   // the digits found so far (after the last pass: the selected key)
  u32 rank;     // rank of the selected element among the keys that share the prefix
  u32 n;        // keys that take part
  u32 pad;
};

struct FeScratch {
  SelectState* state;
  u32* hist;   // [SELECT_PASSES][256]
  u32* keys;   // [n]
  static FeScratch carve(void* buf, size_t n, size_t& bytes) {
    Carver c(buf);
    FeScratch s;
    s.state = c.take<SelectState>(1);
    s.hist = c.take<u32>(SELECT_PASSES * 256);
    s.keys = c.take<u32>(n);
    bytes = c.total();
    return s;
  }
};

size_t frontend_scratch_bytes(int64_t n) {
  size_t bytes = 0;
  FeScratch::carve(nullptr, (size_t)(n > 0 ? n : 0), bytes);
  return bytes;
}

// digit `pass` (1 ... 3) of the stored keys
__global__ __launch_bounds__(FE_THREADS) void select_hist_kernel(int64_t N, int pass, FeScratch sc) {
  __shared__ u32 h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const u32 prefix = sc.state->prefix;
  const int64_t base = (int64_t)blockIdx.x * FE_CHUNK;
  for (int r = 0; r < FE_PER_THREAD; ++r) {
    const int64_t i = base + (int64_t)r * FE_THREADS + threadIdx.x;
    if (i >= N) break;
    const u32 key = sc.keys[i];
    select_count(h, key != FE_NO_KEY, key, pass, prefix);
  }
  __syncthreads();
  select_flush(h, sc.hist + pass * 256);
}

// One workgroup: the digit whose bucket holds the rank.  Pass 0 counts the keys and sets the rank; the last pass writes the
// median (NaN when no key took part) and the count where the caller wants them.
__global__ __launch_bounds__(FE_THREADS) void select_digit_kernel(int pass, FeScratch sc, float* __restrict__ out_median,
                                                                  int32_t* __restrict__ out_count) {
  __shared__ u32 s_w[FE_WAVES];
  __shared__ u32 s_prefix, s_rank;
  const int t = threadIdx.x;
  u32 prefix = 0u, rank = 0u, n = 0u;
  if (pass > 0) {   // (read by every thread before the first barrier, written by thread 0 after the last)
    prefix = sc.state->prefix;
    rank = sc.state->rank;
    n = sc.state->n;
  }
  const u32 cnt = sc.hist[pass * 256 + t];
  u32 tot;
  const u32 excl = block_excl_scan<FE_WAVES>(cnt, s_w, &tot);
  if (pass == 0) {
    n = tot;
    rank = n > 0u ? (n - 1u) / 2u : 0u;
  }
  if (t == 0) {
    s_prefix = prefix;
    s_rank = rank;
  }
  __syncthreads();
  select_narrow(cnt, excl, prefix, rank, &s_prefix, &s_rank);   // one thread at most
  __syncthreads();
  if (t == 0) {
    sc.state->prefix = s_prefix;
    sc.state->rank = s_rank;
    sc.state->n = n;
    if (pass == SELECT_PASSES - 1) {
      if (out_median) out_median[0] = n > 0u ? bits2f(s_prefix) : __builtin_nanf("");
      if (out_count) out_count[0] = (int32_t)n;
    }
  }
}

// the passes after the caller's key kernel, which stored the keys and counted digit 0 into sc.hist[0 .. 256)
static void launch_select(int64_t N, const FeScratch& sc, float* out_median, int32_t* out_count, hipStream_t st) {
  const int hb = (int)((N + FE_CHUNK - 1) / FE_CHUNK);
  for (int pass = 0; pass < SELECT_PASSES; ++pass) {
    if (pass > 0) select_hist_kernel<<<hb, FE_THREADS, 0, st>>>(N, pass, sc);
    select_digit_kernel<<<1, FE_THREADS, 0, st>>>(pass, sc, out_median, out_count);
  }
}

// ---- the gradient intensity -------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect_index(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// gray of the reflect-padded image at (y, x), -1 <= y <= H, -1 <= x <= W
__device__ __forceinline__ float gray_at(const float* __restrict__ img, int64_t ps, int W, int H, int y, int x) {
  const int64_t i = (int64_t)reflect_index(y, H) * W + reflect_index(x, W);
  return ((img[i] + img[ps + i]) + img[2 * ps + i]) / 3.0f;
}

// the Scharr intensity of the centre of a 3 x 3 neighbourhood (rows a, b, c of the padded gray image)
__device__ __forceinline__ float intensity9(float a0, float a1, float a2, float b0, float b1, float b2, float c0, float c1,
                                            float c2) {
  const float gv = 0.03125f * (((3.0f * a0 + 10.0f * a1) + 3.0f * a2) - ((3.0f * c0 + 10.0f * c1) + 3.0f * c2));
  const float gh = 0.03125f * (((3.0f * a0 + 10.0f * b0) + 3.0f * c0) - ((3.0f * a2 + 10.0f * b2) + 3.0f * c2));
  const bool ok = fabsf(a0) > 0.01f && fabsf(a1) > 0.01f && fabsf(a2) > 0.01f && fabsf(b0) > 0.01f && fabsf(b1) > 0.01f &&
                  fabsf(b2) > 0.01f && fabsf(c0) > 0.01f && fabsf(c1) > 0.01f && fabsf(c2) > 0.01f;
  return ok ? sqrtf(gv * gv + gh * gh) : 0.0f;
}

__device__ __forceinline__ float intensity_global(const float* __restrict__ img, int64_t ps, int W, int H, int y, int x) {
  return intensity9(gray_at(img, ps, W, H, y - 1, x - 1), gray_at(img, ps, W, H, y - 1, x), gray_at(img, ps, W, H, y - 1, x + 1),
                    gray_at(img, ps, W, H, y, x - 1), gray_at(img, ps, W, H, y, x), gray_at(img, ps, W, H, y, x + 1),
                    gray_at(img, ps, W, H, y + 1, x - 1), gray_at(img, ps, W, H, y + 1, x), gray_at(img, ps, W, H, y + 1, x + 1));
}

// LDS floats of a block: bh + 3 rows of bw + 2 (the halo's bh + 2 rows, one row of slack for the intensities written over it)
__host__ __device__ inline int64_t grad_mask_block_floats(int W, int H) {
  return (int64_t)(H / FE_GRID_BLOCKS + 3) * (int64_t)(W / FE_GRID_BLOCKS + 2);
}

// Workgroups 0 ... 1023: image block (r, c) = (b / 32, b % 32).  Workgroups from 1024: 256 margin pixels each, the columns
// right of the blocks first (all rows), then the rows below them.
__global__ __launch_bounds__(FE_THREADS) void grad_mask_blocks_kernel(int W, int H, int64_t ps, float edge_threshold,
                                                                      const float* __restrict__ img, float* __restrict__ out) {
  extern __shared__ float s_p[];
  __shared__ u32 s_h[256];
  __shared__ u32 s_w[FE_WAVES];
  __shared__ u32 s_prefix, s_rank;
  const int t = threadIdx.x;
  const int bh = H / FE_GRID_BLOCKS, bw = W / FE_GRID_BLOCKS;
  if (blockIdx.x >= FE_GRID_BLOCKS * FE_GRID_BLOCKS) {
    int64_t j = (int64_t)(blockIdx.x - FE_GRID_BLOCKS * FE_GRID_BLOCKS) * FE_THREADS + t;
    const int wr = W - FE_GRID_BLOCKS * bw, wb = FE_GRID_BLOCKS * bw, hb = H - FE_GRID_BLOCKS * bh;
    const int64_t right = (int64_t)H * wr;
    int y, x;
    if (j < right) {
      y = (int)(j / wr);
      x = wb + (int)(j - (int64_t)y * wr);
    } else {
      j -= right;
      if (j >= (int64_t)hb * wb) return;
      y = (int)(j / wb);
      x = (int)(j - (int64_t)y * wb);
      y += FE_GRID_BLOCKS * bh;
    }
    out[(int64_t)y * W + x] = intensity_global(img, ps, W, H, y, x);   // the reference leaves the raw intensity here
    return;
  }
  const int y0 = (int)(blockIdx.x / FE_GRID_BLOCKS) * bh, x0 = (int)(blockIdx.x % FE_GRID_BLOCKS) * bw;
  const int pw = bw + 2, n = bh * bw;
  // gray row y0 + g (g = -1 ... bh) lies in LDS row g + 2, column x0 + h (h = -1 ... bw) in column h + 1
  for (int e = t; e < (bh + 2) * pw; e += FE_THREADS) {
    const int hy = e / pw, hx = e - hy * pw;
    s_p[(hy + 1) * pw + hx] = gray_at(img, ps, W, H, y0 + hy - 1, x0 + hx - 1);
  }
  __syncthreads();
  // Intensities, 256 pixels of the block at a time in row-major order.  Pixel (y, x) reads LDS rows y + 1 ... y + 3 and is
  // stored in LDS row y, which held gray row y - 2: that one is read only by pixel rows up to y - 1, all of them in this round
  // (read before the barrier) or an earlier one; the next round reads rows >= (its first pixel row) + 1 > every row written here.
  for (int base = 0; base < n; base += FE_THREADS) {
    const int i = base + t;
    int y = 0, x = 0;
    float I = 0.0f;
    if (i < n) {
      y = i / bw;
      x = i - y * bw;
      const float* q = s_p + (y + 1) * pw + x;
      I = intensity9(q[0], q[1], q[2], q[pw], q[pw + 1], q[pw + 2], q[2 * pw], q[2 * pw + 1], q[2 * pw + 2]);
    }
    __syncthreads();
    if (i < n) s_p[y * pw + x] = I;
  }
  __syncthreads();
  // the lower median of the n intensities: four 8-bit digits, most significant first
  u32 prefix = 0u, rank = (u32)((n - 1) / 2);
  for (int pass = 0; pass < SELECT_PASSES; ++pass) {
    s_h[t] = 0u;
    __syncthreads();
    for (int i = t; i < n; i += FE_THREADS) {
      const int y = i / bw;
      const u32 key = f2bits(s_p[y * pw + (i - y * bw)]);
      select_count(s_h, key != FE_NO_KEY, key, pass, prefix);
    }
    __syncthreads();
    const u32 cnt = s_h[t];
    const u32 excl = block_excl_scan<FE_WAVES>(cnt, s_w);
    select_narrow(cnt, excl, prefix, rank, &s_prefix, &s_rank);   // exactly one thread: n >= 1
    __syncthreads();
    prefix = s_prefix;
    rank = s_rank;
    __syncthreads();   // s_h, s_w, s_prefix and s_rank are rewritten by the next pass
  }
  const float th = bits2f(prefix) * edge_threshold;
  const bool wipe = 1.0f <= th;   // the reference's second masked write zeroes the ones of its first when th >= 1
  for (int i = t; i < n; i += FE_THREADS) {
    const int y = i / bw, x = i - y * bw;
    out[(int64_t)(y0 + y) * W + (x0 + x)] = (s_p[y * pw + x] > th && !wipe) ? 1.0f : 0.0f;
  }
}

// global mode: intensities as keys, digit 0
__global__ __launch_bounds__(FE_THREADS) void grad_intensity_keys_kernel(int W, int H, int64_t ps, const float* __restrict__ img,
                                                                         FeScratch sc) {
  __shared__ u32 h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t N = (int64_t)W * H, base = (int64_t)blockIdx.x * FE_CHUNK;
  for (int r = 0; r < FE_PER_THREAD; ++r) {
    const int64_t i = base + (int64_t)r * FE_THREADS + threadIdx.x;
    if (i >= N) break;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    const u32 key = f2bits(intensity_global(img, ps, W, H, y, x));
    sc.keys[i] = key;
    select_count(h, key != FE_NO_KEY, key, 0, 0u);
  }
  __syncthreads();
  select_flush(h, sc.hist);
}

__global__ __launch_bounds__(FE_THREADS) void grad_threshold_kernel(int64_t N, float edge_threshold, FeScratch sc,
                                                                    float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * FE_THREADS + threadIdx.x;
  if (i >= N) return;
  const float th = bits2f(sc.state->prefix) * edge_threshold;
  out[i] = bits2f(sc.keys[i]) > th ? 1.0f : 0.0f;
}

hipError_t launch_grad_mask(int W, int H, int64_t plane_stride, int mode, float edge_threshold, const float* image,
                            float* mask, void* scratch, hipStream_t st) {
  const int64_t N = (int64_t)W * H;
  if (mode == OLSR_GRAD_MASK_BLOCKS) {
    const int bh = H / FE_GRID_BLOCKS, bw = W / FE_GRID_BLOCKS;
    const int64_t margin = N - (int64_t)FE_GRID_BLOCKS * bh * FE_GRID_BLOCKS * bw;
    const int grid = FE_GRID_BLOCKS * FE_GRID_BLOCKS + (int)((margin + FE_THREADS - 1) / FE_THREADS);
    const size_t lds = (size_t)grad_mask_block_floats(W, H) * sizeof(float);
    grad_mask_blocks_kernel<<<grid, FE_THREADS, lds, st>>>(W, H, plane_stride, edge_threshold, image, mask);
    return hipSuccess;
  }
  size_t bytes;
  const FeScratch sc = FeScratch::carve(scratch, (size_t)N, bytes);
  const hipError_t e = hipMemsetAsync(sc.hist, 0, (size_t)SELECT_PASSES * 256 * sizeof(u32), st);
  if (e != hipSuccess) return e;
  grad_intensity_keys_kernel<<<(int)((N + FE_CHUNK - 1) / FE_CHUNK), FE_THREADS, 0, st>>>(W, H, plane_stride, image, sc);
  launch_select(N, sc, nullptr, nullptr, st);
  grad_threshold_kernel<<<(int)((N + FE_THREADS - 1) / FE_THREADS), FE_THREADS, 0, st>>>(N, edge_threshold, sc, mask);
  return hipSuccess;
}

// ---- median depth -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FE_THREADS) void median_depth_keys_kernel(int64_t N, const float* __restrict__ depth,
                                                                       const float* __restrict__ opacity,
                                                                       const uint8_t* __restrict__ mask, FeScratch sc) {
  __shared__ u32 h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * FE_CHUNK;
  for (int r = 0; r < FE_PER_THREAD; ++r) {
    const int64_t i = base + (int64_t)r * FE_THREADS + threadIdx.x;
    if (i >= N) break;
    const float d = depth[i];
    const bool valid = d > 0.0f && opacity[i] > 0.95f && (mask == nullptr || mask[i] != 0);   // NaN > 0 is false
    const u32 key = valid ? f2bits(d) : FE_NO_KEY;
    sc.keys[i] = key;
    select_count(h, key != FE_NO_KEY, key, 0, 0u);
  }
  __syncthreads();
  select_flush(h, sc.hist);
}

hipError_t launch_median_depth(int64_t N, const float* depth, const float* opacity, const uint8_t* mask, void* scratch,
                               float* median, int32_t* count, hipStream_t st) {
  size_t bytes;
  const FeScratch sc = FeScratch::carve(scratch, (size_t)N, bytes);
  const hipError_t e = hipMemsetAsync(sc.hist, 0, (size_t)SELECT_PASSES * 256 * sizeof(u32), st);
  if (e != hipSuccess) return e;
  median_depth_keys_kernel<<<(int)((N + FE_CHUNK - 1) / FE_CHUNK), FE_THREADS, 0, st>>>(N, depth, opacity, mask, sc);
  launch_select(N, sc, median, count, st);
  return hipSuccess;
}

// ---- covisibility counts ------------------------------------------------------------------------------------------------------
// counts[0] = |cur|, counts[1 + 2 k] = |cur & vis_k|, counts[2 + 2 k] = |vis_k|
__global__ __launch_bounds__(FE_THREADS) void covisibility_kernel(int64_t P, const int32_t* __restrict__ n_touched,
                                                                  olsr_covis_views v, uint8_t* __restrict__ cur_out,
                                                                  unsigned long long* __restrict__ counts) {
  __shared__ u32 s_c[1 + 2 * OLSR_COVIS_MAX_VIEWS];
  const int t = threadIdx.x;
  if (t < 1 + 2 * OLSR_COVIS_MAX_VIEWS) s_c[t] = 0u;
  __syncthreads();
  u32 c_cur = 0u, c_in[OLSR_COVIS_MAX_VIEWS], c_vis[OLSR_COVIS_MAX_VIEWS];   // wave-uniform
#pragma unroll
  for (int k = 0; k < OLSR_COVIS_MAX_VIEWS; ++k) c_in[k] = c_vis[k] = 0u;
  const int64_t base = (int64_t)blockIdx.x * (FE_THREADS * FE_COVIS_PER_THREAD);
  for (int r = 0; r < FE_COVIS_PER_THREAD; ++r) {
    const int64_t i = base + (int64_t)r * FE_THREADS + t;
    const bool in = i < P;
    const bool cur = in && n_touched[i] > 0;
    if (in && cur_out) cur_out[i] = cur ? 1 : 0;
    c_cur += (u32)__popcll(ballot(cur));
#pragma unroll
    for (int k = 0; k < OLSR_COVIS_MAX_VIEWS; ++k) {
      if (k < v.K) {
        const bool vk = in && v.vis[k][i] != 0;
        c_vis[k] += (u32)__popcll(ballot(vk));
        c_in[k] += (u32)__popcll(ballot(vk && cur));
      }
    }
  }
  if (lane_id() == 0) {
    if (c_cur) atomicAdd(&s_c[0], c_cur);
#pragma unroll
    for (int k = 0; k < OLSR_COVIS_MAX_VIEWS; ++k) {
      if (k < v.K) {
        if (c_in[k]) atomicAdd(&s_c[1 + 2 * k], c_in[k]);
        if (c_vis[k]) atomicAdd(&s_c[2 + 2 * k], c_vis[k]);
      }
    }
  }
  __syncthreads();
  if (t < 1 + 2 * v.K && s_c[t]) atomicAdd(&counts[t], (unsigned long long)s_c[t]);
}

hipError_t launch_covisibility(int64_t P, const int32_t* n_touched, const olsr_covis_views& views, uint8_t* cur_out,
                               int64_t* counts, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)OLSR_COVIS_COUNTS * sizeof(int64_t), st);
  if (e != hipSuccess) return e;
  const int64_t per = (int64_t)FE_THREADS * FE_COVIS_PER_THREAD;
  covisibility_kernel<<<(int)((P + per - 1) / per), FE_THREADS, 0, st>>>(P, n_touched, views, cur_out,
                                                                        reinterpret_cast<unsigned long long*>(counts));
  return hipSuccess;
}

// ---- the keyframe decision ----------------------------------------------------------------------------------------------------
// camera centre c = -(R^-1 t) of a row-major world-to-camera pose, in double from its float32 entries; R^-1 by cofactors
__device__ __forceinline__ void pose_centre(const float* __restrict__ T, double* c) {
  const double r00 = T[0], r01 = T[1], r02 = T[2], r10 = T[4], r11 = T[5], r12 = T[6], r20 = T[8], r21 = T[9], r22 = T[10];
  const double c00 = r11 * r22 - r12 * r21, c01 = r12 * r20 - r10 * r22, c02 = r10 * r21 - r11 * r20;
  const double det = (r00 * c00 + r01 * c01) + r02 * c02;
  const double id = 1.0 / det;
  const double i00 = c00 * id, i01 = (r02 * r21 - r01 * r22) * id, i02 = (r01 * r12 - r02 * r11) * id;
  const double i10 = c01 * id, i11 = (r00 * r22 - r02 * r20) * id, i12 = (r02 * r10 - r00 * r12) * id;
  const double i20 = c02 * id, i21 = (r01 * r20 - r00 * r21) * id, i22 = (r00 * r11 - r01 * r10) * id;
  const double t0 = T[3], t1 = T[7], t2 = T[11];
  c[0] = -((i00 * t0 + i01 * t1) + i02 * t2);
  c[1] = -((i10 * t0 + i11 * t1) + i12 * t2);
  c[2] = -((i20 * t0 + i21 * t1) + i22 * t2);
}

// || translation of A B^-1 || = || R_A c_B + t_A ||: the vector in double, narrowed once, its norm in float32
__device__ __forceinline__ float rel_dist(const float* __restrict__ A, const double* cB) {
  float tv[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    tv[r] = (float)((((double)A[4 * r] * cB[0] + (double)A[4 * r + 1] * cB[1]) + (double)A[4 * r + 2] * cB[2]) +
                    (double)A[4 * r + 3]);
  return sqrtf((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]);
}

__global__ __launch_bounds__(64) void keyframe_decide_kernel(olsr_keyframe_decide_params p, const long long* __restrict__ counts,
                                                             const float* __restrict__ median_dev,
                                                             const float* __restrict__ cur_pose,
                                                             const float* __restrict__ kf_poses, int32_t* __restrict__ rec_i,
                                                             float* __restrict__ rec_f) {
  __shared__ double s_c[OLSR_COVIS_MAX_VIEWS + 1][3];   // camera centres: keyframes 0 ... K - 1, then the tracked frame
  __shared__ float s_ratio[OLSR_COVIS_MAX_VIEWS];
  __shared__ double s_score[OLSR_COVIS_MAX_VIEWS];
  __shared__ int s_rem_a;
  const int l = threadIdx.x, K = p.window_len;
  const float nan = __builtin_nanf("");
  if (l < K) pose_centre(kf_poses + 16 * l, s_c[l]);
  if (l == OLSR_COVIS_MAX_VIEWS) pose_centre(cur_pose, s_c[OLSR_COVIS_MAX_VIEWS]);
  const long long n_cur = counts[0];
  // the cut-off ratio of window position l >= 1 (position l + 1 >= 2 of [cur] + window)
  if (l < OLSR_COVIS_MAX_VIEWS) {
    float ratio = nan;
    if (l >= 1 && l < K) {
      const long long inter = counts[1 + 2 * l], nv = counts[2 + 2 * l];
      ratio = (float)inter / (float)(n_cur < nv ? n_cur : nv);
    }
    s_ratio[l] = ratio;
    s_score[l] = (double)nan;
  }
  __syncthreads();
  if (l == 0) {
    int a = -1;
    for (int k = 1; k < K; ++k)
      if (s_ratio[k] <= p.kf_cutoff) a = k;   // the last candidate
    s_rem_a = a;
  }
  __syncthreads();
  const int rem_a = s_rem_a;
  // the score of window position l among the positions >= 1 that are left
  if (l >= 1 && l < K && l != rem_a) {
    const float* Ti = kf_poses + 16 * l;
    const double k0 = (double)sqrtf(rel_dist(Ti, s_c[OLSR_COVIS_MAX_VIEWS]));
    double sum = 0.0;
    for (int j = 1; j < K; ++j) {
      if (j == l || j == rem_a) continue;
      sum = sum + 1.0 / (double)(rel_dist(Ti, s_c[j]) + 1e-6f);
    }
    s_score[l] = k0 * sum;
  }
  __syncthreads();
  if (l != 0) return;
  const float median = median_dev[0];
  float dist = nan, ratio_u = nan;
  long long inter0 = 0, vis0 = 0;
  if (K > 0) {
    inter0 = counts[1];
    vis0 = counts[2];
    dist = rel_dist(cur_pose, s_c[0]);
    ratio_u = (float)inter0 / (float)(n_cur + vis0 - inter0);
  }
  const bool is_kf = (ratio_u < p.kf_overlap && dist > p.kf_min_translation * median) || dist > p.kf_translation * median;
  bool create = is_kf;
  if (p.window_len < p.window_size) create = p.check_time != 0 && ratio_u < p.kf_overlap;
  if (p.single_thread) create = p.check_time != 0 && create;
  int rem_b = -1;
  if (K + 1 - (rem_a >= 0 ? 1 : 0) > p.window_size) {
    double best = 0.0;
    for (int k = 1; k < K; ++k) {
      if (k == rem_a) continue;
      if (rem_b < 0 || s_score[k] > best) {   // the first maximum wins
        rem_b = k;
        best = s_score[k];
      }
    }
  }
  rec_i[0] = create ? 1 : 0;
  rec_i[1] = (rem_a >= 0 ? 1 : 0) + (rem_b >= 0 ? 1 : 0);
  rec_i[2] = rem_a;
  rec_i[3] = rem_b;
  rec_i[4] = is_kf ? 1 : 0;
  rec_i[5] = (int32_t)n_cur;
  rec_i[6] = (int32_t)inter0;
  rec_i[7] = (int32_t)vis0;
  rec_f[0] = dist;
  rec_f[1] = median;
  rec_f[2] = ratio_u;
  rec_f[3] = 0.0f;
  for (int k = 0; k < OLSR_COVIS_MAX_VIEWS; ++k) {
    rec_f[4 + k] = s_ratio[k];
    rec_f[4 + OLSR_COVIS_MAX_VIEWS + k] = (float)s_score[k];
  }
  for (int k = 4 + 2 * OLSR_COVIS_MAX_VIEWS; k < OLSR_KEYFRAME_RECORD_FLOATS; ++k) rec_f[k] = 0.0f;
}

void launch_keyframe_decide(const olsr_keyframe_decide_params& p, const int64_t* counts, const float* median,
                            const float* cur_pose, const float* kf_poses, void* record, hipStream_t st) {
  int32_t* rec_i = reinterpret_cast<int32_t*>(record);
  keyframe_decide_kernel<<<1, 64, 0, st>>>(p, reinterpret_cast<const long long*>(counts), median, cur_pose, kf_poses, rec_i,
                                           reinterpret_cast<float*>(rec_i + 8));
}

}  // namespace olsr
