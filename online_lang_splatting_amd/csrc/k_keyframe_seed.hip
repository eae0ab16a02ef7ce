// k_keyframe_seed.hip — the rows of a keyframe's new Gaussians from its RGB-D image (include/olsr.h, "keyframe seeding").
//
// The reference builds them on the host for every keyframe (FrontEnd.add_new_keyframe utils/slam_frontend.py:106-132,
// BackEnd.add_next_kf utils/slam_backend.py:187-202, GaussianModel.create_pcd_from_image / _and_depth
// gaussian_splatting/scene/gaussian_model.py:135-281): image and depth to the host, Open3D's RGBD image, back-projection and
// random_down_sample, np.median(depth), and the points back to the GPU for distCUDA2.  Here the frame stays on the device:
//
//   plan    one memset and eleven dependent launches, no host read in between:
//             seed_hist<0>            d' = rgb_ok ? depth : 0 per pixel, its median key (the float bits; non-finite, negative
//                                     and zero count as 0) stored once; first digit of the three radix selects
//             seed_select x 4         one workgroup: scans the 256 counts of a pass, narrows each select by one digit
//             seed_hist<1> x 3        the next digit of the pixels that still match a select's prefix
//             seed_count, _prefix     kept pixels per block of SEED_PIX, prefixed over the blocks in block order
//             seed_emit               ranks the kept pixels of a block (wave ballots) and writes their rows, in pixel order
//           The three selects share the passes: the lower and the upper middle element of d' over all W H pixels (the median,
//           np.median at gaussian_model.py:204) and the n_keep-th smallest sampling key among the valid pixels.  The
//           select's steps are olsr_select.h's (shared with k_frontend.hip); which pixels take part is said here, per
//           select, and by no reserved key: fmix32 is a bijection, so 0xFFFFFFFF is the sampling key of one pixel index
//           per seed.  The histograms are integer atomics — order-independent —, nothing else is atomic: two runs give
//           the same bits.
//   finish  olsr_knn_mean_dist2 on the n new points alone (as the reference does per keyframe), then
//           scale = logf(sqrtf(max(d2, 1e-7f) * ps)) on all three axes.
//
// The arithmetic is pinned statement by statement in include/olsr.h; the translation unit is compiled without FMA
// contraction (build.py), so the double back-projection and the exposure line are the operations the source writes.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_select.h"

namespace olsr {

constexpr int SEED_THREADS = 256;
constexpr int SEED_WAVES = SEED_THREADS / 64;
constexpr int SEED_PIX = SEED_THREADS;        // pixels per block of count / emit (one per thread)
constexpr int SEED_HIST_PER_THREAD = 16;      // pixels per thread of a histogram pass
constexpr int SEED_HIST_PIX = SEED_THREADS * SEED_HIST_PER_THREAD;
constexpr int SEED_SELECTS = 3;               // lower middle, upper middle of d'; the sampling key threshold
constexpr int SEED_PREFIX_THREADS = 1024;

// what the select kernels carry from pass to pass and hand to count / emit
struct SeedState {
  u32 prefix[SEED_SELECTS];   // the digits found so far (after the last pass: the selected key)
  u32 rank[SEED_SELECTS];     // rank of the selected element among the keys that share the prefix
  int32_t n_valid, n_keep;
};

__host__ __device__ inline size_t seed_blocks(size_t N) { return (N + SEED_PIX - 1) / SEED_PIX; }

struct SeedScratch {
  SeedState* state;
  u32* hist;       // [SELECT_PASSES][SEED_SELECTS][256]
  u32* mkey;       // [N rounded up to 4] median key of d' per pixel; finish reuses the words as mean_dist2 [n]
  int32_t* counts; // [blocks of SEED_PIX]
  int32_t* offsets;
  static SeedScratch carve(void* buf, size_t N, size_t& bytes) {
    Carver c(buf);
    SeedScratch s;
    s.state = c.take<SeedState>(1);
    s.hist = c.take<u32>(SELECT_PASSES * SEED_SELECTS * 256);
    s.mkey = c.take<u32>((N + 3) / 4 * 4);
    s.counts = c.take<int32_t>(seed_blocks(N));
    s.offsets = c.take<int32_t>(seed_blocks(N));
    bytes = c.total();
    return s;
  }
};

size_t keyframe_seed_scratch_bytes(int W, int H) {
  size_t bytes = 0;
  SeedScratch::carve(nullptr, (W > 0 && H > 0) ? (size_t)W * (size_t)H : 0, bytes);
  return bytes;
}

// murmur3's finaliser: a bijection of 32 bits
__device__ __forceinline__ u32 fmix32(u32 x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ u32 seed_sample_key(u32 i, u32 seed) { return fmix32(i ^ (seed * 0x9E3779B9u)); }

// a pixel is valid iff 0 < d' < depth_trunc; the median key of a valid pixel is the bits of d' itself
__device__ __forceinline__ bool seed_valid(u32 mkey, float depth_trunc) { return mkey != 0u && bits2f(mkey) < depth_trunc; }

// One digit of the three selects.  PASS0: computes d' and stores its median key; every pixel takes part in the two median
// selects, every valid pixel in the sampling select.  Later passes: the pixels whose higher digits equal the select's prefix.
template <bool PASS0>
__global__ __launch_bounds__(SEED_THREADS) void seed_hist(int64_t N, int pass, olsr_keyframe_seed_params p,
                                                          const float* __restrict__ image, const float* __restrict__ depth,
                                                          SeedScratch sc) {
  __shared__ u32 h[SEED_SELECTS][256];
  for (int s = 0; s < SEED_SELECTS; ++s) h[s][threadIdx.x] = 0u;
  __syncthreads();
  u32 prefix[SEED_SELECTS] = {0u, 0u, 0u};
  bool live[SEED_SELECTS] = {true, true, true};
  if (!PASS0) {
    __builtin_assume(pass > 0);   // (passes 1 ... 3, launch_keyframe_seed_plan: select_count's pass-0 case folds away)
    for (int s = 0; s < SEED_SELECTS; ++s) prefix[s] = sc.state->prefix[s];
    live[2] = sc.state->n_keep > 0;
  }
  const int64_t base = (int64_t)blockIdx.x * SEED_HIST_PIX;
  for (int r = 0; r < SEED_HIST_PER_THREAD; ++r) {
    const int64_t i = base + (int64_t)r * SEED_THREADS + threadIdx.x;
    if (i >= N) break;
    u32 mk;
    if (PASS0) {
      const float sum = (image[i] + image[p.plane_stride + i]) + image[2 * p.plane_stride + i];
      const float d = sum > p.rgb_boundary_threshold ? depth[i] : 0.0f;
      mk = (d > 0.0f && d < __builtin_inff()) ? f2bits(d) : 0u;   // NaN, negative, zero and +inf count as 0
      sc.mkey[i] = mk;
    } else {
      mk = sc.mkey[i];
    }
    const u32 keys[SEED_SELECTS] = {mk, mk, seed_sample_key((u32)i, p.seed)};
    const bool in[SEED_SELECTS] = {true, true, seed_valid(mk, p.depth_trunc)};
#pragma unroll
    for (int s = 0; s < SEED_SELECTS; ++s) select_count(h[s], in[s] && live[s], keys[s], PASS0 ? 0 : pass, prefix[s]);
  }
  __syncthreads();
  u32* g = sc.hist + (size_t)pass * SEED_SELECTS * 256;
  for (int s = 0; s < SEED_SELECTS; ++s) select_flush(h[s], g + s * 256);
}

// One workgroup: for each select, the digit whose bucket holds the rank; after the last pass the status and aux words.
__global__ __launch_bounds__(SEED_THREADS) void seed_select(int64_t N, int pass, olsr_keyframe_seed_params p, SeedScratch sc,
                                                            int32_t* __restrict__ status, float* __restrict__ aux) {
  __shared__ u32 s_w[SEED_WAVES];
  __shared__ u32 s_prefix[SEED_SELECTS], s_rank[SEED_SELECTS];
  __shared__ int32_t s_nvalid, s_nkeep;
  const int t = threadIdx.x;
  const u32* g = sc.hist + (size_t)pass * SEED_SELECTS * 256;
  // the state as the pass before left it (read by every thread before the first barrier, written after it)
  u32 prefix[SEED_SELECTS], rank[SEED_SELECTS];
  int32_t n_valid = 0, n_keep = 0;
  if (pass == 0) {
    prefix[0] = prefix[1] = prefix[2] = 0u;
    rank[0] = (u32)((N - 1) / 2);
    rank[1] = (u32)(N / 2);
    rank[2] = 0u;
  } else {
    for (int s = 0; s < SEED_SELECTS; ++s) { prefix[s] = sc.state->prefix[s]; rank[s] = sc.state->rank[s]; }
    n_valid = sc.state->n_valid;
    n_keep = sc.state->n_keep;
  }
  if (t < SEED_SELECTS) { s_prefix[t] = prefix[t]; s_rank[t] = rank[t]; }
  for (int s = 0; s < SEED_SELECTS; ++s) {
    const u32 cnt = g[s * 256 + t];
    u32 tot;
    const u32 excl = block_excl_scan<SEED_WAVES>(cnt, s_w, &tot);
    if (s == 2 && pass == 0) {
      // the sampling select starts here: its first histogram counted the valid pixels
      n_valid = (int32_t)tot;
      n_keep = (int32_t)((double)n_valid * (1.0 / (double)p.downsample));
      if (n_keep > p.capacity) n_keep = p.capacity;   // (never: capacity >= W H / downsample is an argument check)
      rank[2] = n_keep > 0 ? (u32)(n_keep - 1) : 0u;
    }
    if (s < 2 || n_keep > 0) select_narrow(cnt, excl, prefix[s], rank[s], &s_prefix[s], &s_rank[s]);   // (live selects only)
    __syncthreads();   // s_w is rewritten by the next scan; s_prefix / s_rank are read below
  }
  if (t == 0) {
    s_nvalid = n_valid;
    s_nkeep = n_keep;
    for (int s = 0; s < SEED_SELECTS; ++s) { sc.state->prefix[s] = s_prefix[s]; sc.state->rank[s] = s_rank[s]; }
    sc.state->n_valid = n_valid;
    sc.state->n_keep = n_keep;
    if (pass == SELECT_PASSES - 1) {
      const float a = bits2f(s_prefix[0]), b = bits2f(s_prefix[1]);
      float median = a;                       // odd N: the middle element
      if ((N & 1) == 0) { const float ab = a + b; median = ab / 2.0f; }
      float ps = (float)p.point_size;
      if (p.adaptive_pointsize) {
        // numpy 1.x evaluates python_float * np.float32 in double; min(0.05, .) in double; narrowed once
        const double prod = p.point_size * (double)median;
        ps = (float)(0.05 < prod ? 0.05 : prod);
      }
      aux[0] = median;
      aux[1] = ps;
      aux[2] = aux[3] = 0.0f;
      status[0] = n_valid;
      status[1] = n_keep;
      for (int k = 2; k < 8; ++k) status[k] = 0;
    }
  }
}

__device__ __forceinline__ bool seed_kept(int64_t i, int64_t N, const olsr_keyframe_seed_params& p, const SeedScratch& sc,
                                          u32* mkey_out) {
  if (i >= N) return false;
  const u32 mk = sc.mkey[i];
  *mkey_out = mk;
  return sc.state->n_keep > 0 && seed_valid(mk, p.depth_trunc) && seed_sample_key((u32)i, p.seed) <= sc.state->prefix[2];
}

__global__ __launch_bounds__(SEED_THREADS) void seed_count(int64_t N, olsr_keyframe_seed_params p, SeedScratch sc) {
  u32 mk;
  const bool kept = seed_kept((int64_t)blockIdx.x * SEED_PIX + threadIdx.x, N, p, sc, &mk);
  const int n = __syncthreads_count(kept);
  if (threadIdx.x == 0) sc.counts[blockIdx.x] = n;
}

__global__ __launch_bounds__(SEED_PREFIX_THREADS) void seed_prefix(int nb, SeedScratch sc) {
  __shared__ int32_t s_w[SEED_PREFIX_THREADS / 64];
  single_block_excl_scan<SEED_PREFIX_THREADS / 64>(nb, sc.counts, sc.offsets, s_w);
}

// colour of one channel -> its SH dc coefficient (RGB2SH of the byte image the reference hands Open3D)
__device__ __forceinline__ float seed_f_dc(float v, bool has_exposure, float ea, float eb) {
  float c = v;
  if (has_exposure) {
    c = ea * v + eb;                          // (torch.exp(a)) * image + b, two roundings
    c = fminf(fmaxf(c, 0.0f), 1.0f);
  }
  const uint8_t byte = (uint8_t)(c * 255.0f);  // .byte(): truncation
  const float colour = (float)byte / 255.0f;   // Open3D's colours / 255 in float32, as RGB2SH receives them after .float()
  return (colour - 0.5f) / 0.28209479177387814f;
}

__global__ __launch_bounds__(SEED_THREADS) void seed_emit(int64_t N, olsr_keyframe_seed_params p,
                                                          const float* __restrict__ image,
                                                          const float* __restrict__ exposure, const float* __restrict__ w2c,
                                                          olsr_map_buffers rows, int32_t* __restrict__ pix_index,
                                                          SeedScratch sc) {
  __shared__ u32 s_w[SEED_WAVES];
  const int64_t i = (int64_t)blockIdx.x * SEED_PIX + threadIdx.x;
  u32 mk = 0u;
  const bool kept = seed_kept(i, N, p, sc, &mk);
  const u32 r = block_rank<SEED_WAVES>(kept, s_w);
  if (!kept) return;
  const int64_t k = (int64_t)sc.offsets[blockIdx.x] + (int64_t)r;
  if (k >= (int64_t)p.capacity) return;
  pix_index[k] = (int32_t)i;

  // colour
  const bool has_exposure = exposure != nullptr;
  const float ea = has_exposure ? pinned_expf(exposure[0]) : 1.0f, eb = has_exposure ? exposure[1] : 0.0f;
  const int M = p.M;
  float* sh = rows.shs + (size_t)k * M * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) sh[c] = seed_f_dc(image[(int64_t)c * p.plane_stride + i], has_exposure, ea, eb);
  for (int e = 3; e < 3 * M; ++e) sh[e] = 0.0f;

  // back-projection in double (Open3D), then Rt (p - t); no contraction: the translation unit is built with it off
  const int u = (int)(i % p.W), v = (int)(i / p.W);
  const double z = (double)bits2f(mk);
  const double x = ((double)u - p.cx) * z / p.fx;
  const double y = ((double)v - p.cy) * z / p.fy;
  const double q0 = x - (double)w2c[3], q1 = y - (double)w2c[7], q2 = z - (double)w2c[11];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double wc = ((double)w2c[c] * q0 + (double)w2c[4 + c] * q1) + (double)w2c[8 + c] * q2;
    rows.means3D[3 * k + c] = (float)wc;
  }
  rows.opacities[k] = 0.0f;   // inverse_sigmoid(0.5)
  rows.rotations[4 * k] = 1.0f;
  rows.rotations[4 * k + 1] = rows.rotations[4 * k + 2] = rows.rotations[4 * k + 3] = 0.0f;
}

__global__ __launch_bounds__(SEED_THREADS) void seed_scales(int n, const float* __restrict__ d2, const float* __restrict__ aux,
                                                            float* __restrict__ scales) {
  const int i = blockIdx.x * SEED_THREADS + threadIdx.x;
  if (i >= n) return;
  const float ps = aux[1];
  const float s = logf(sqrtf(fmaxf(d2[i], 1e-7f) * ps));   // torch.log(torch.sqrt(clamp_min(dist2, 1e-7) * point_size))
  scales[3 * i] = s;
  scales[3 * i + 1] = s;
  scales[3 * i + 2] = s;
}

hipError_t launch_keyframe_seed_plan(const olsr_keyframe_seed_params& p, const float* image, const float* depth,
                                     const float* exposure, const float* w2c, const olsr_map_buffers& rows,
                                     int32_t* pix_index, void* scratch, int32_t* status, float* aux, hipStream_t st) {
  const int64_t N = (int64_t)p.W * p.H;
  size_t bytes;
  const SeedScratch sc = SeedScratch::carve(scratch, (size_t)N, bytes);
  const hipError_t e = hipMemsetAsync(sc.hist, 0, (size_t)SELECT_PASSES * SEED_SELECTS * 256 * sizeof(u32), st);
  if (e != hipSuccess) return e;
  const int hb = (int)((N + SEED_HIST_PIX - 1) / SEED_HIST_PIX), nb = (int)seed_blocks((size_t)N);
  for (int pass = 0; pass < SELECT_PASSES; ++pass) {
    if (pass == 0) seed_hist<true><<<hb, SEED_THREADS, 0, st>>>(N, pass, p, image, depth, sc);
    else seed_hist<false><<<hb, SEED_THREADS, 0, st>>>(N, pass, p, image, depth, sc);
    seed_select<<<1, SEED_THREADS, 0, st>>>(N, pass, p, sc, status, aux);
  }
  seed_count<<<nb, SEED_THREADS, 0, st>>>(N, p, sc);
  seed_prefix<<<1, SEED_PREFIX_THREADS, 0, st>>>(nb, sc);
  seed_emit<<<nb, SEED_THREADS, 0, st>>>(N, p, image, exposure, w2c, rows, pix_index, sc);
  return hipSuccess;
}

void launch_keyframe_seed_finish(const olsr_keyframe_seed_params& p, int n, const olsr_map_buffers& rows, const float* aux,
                                 void* scratch, void* knn_scratch, hipStream_t st) {
  size_t bytes;
  const SeedScratch sc = SeedScratch::carve(scratch, (size_t)p.W * (size_t)p.H, bytes);
  float* d2 = reinterpret_cast<float*>(sc.mkey);   // n <= W H words; the plan is done with them
  launch_knn(n, rows.means3D, d2, knn_scratch, st);
  seed_scales<<<(n + SEED_THREADS - 1) / SEED_THREADS, SEED_THREADS, 0, st>>>(n, d2, aux, rows.scales);
}

}  // namespace olsr
