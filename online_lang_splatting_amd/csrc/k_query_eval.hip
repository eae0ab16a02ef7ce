// k_query_eval.hip — the 2-D evaluation behind a text query (include/olsr.h, "scoring text queries"): the 7 x 7 majority
// vote the reference runs over a phrase's mask (eval/utils.py:47-56, `smooth`), the IoU against the annotated mask
// (eval/evaluate_onlinelangslam.py:160-161), the localisation test of every pixel that attains the smoothed relevancy's
// maximum (:203-223), and the masked PSNR of a rendered frame (utils/eval_utils.py:171-173).
//
// mask_smooth_kernel: one launch, a workgroup of four waves per 64 x 64 output tile and plane.
//   stage   a wave takes an input row of the tile plus its 3-pixel halo, 70 columns: every lane loads one byte (and lanes 0..5
//           a second one), and two ballots turn the row into 70 bits in LDS.  A pixel outside the image, in the LAST ROW or in
//           the LAST COLUMN is a zero bit: the reference clamps the slice's upper bound to H - 1 / W - 1, so neither ever
//           enters a window, and a window is the plain 7 x 7 square cut to [0, H - 2] x [0, W - 2].  Each byte is read once
//           per tile that needs it; nothing but these bits is kept.
//   count   lane l owns column x0 + l.  A row's horizontal count is the popcount of bits l .. l + 6 of its 70 (the words are
//           read as LDS broadcasts); a wave walks its 16 output rows with a running sum over 7 of those counts.
//   vote    1 iff 2 ones > area, area = rows x columns of the cut window (a tie is 0: np.argmax takes the first maximum).
//   EVAL    the epilogue of the same launch: per row the ballots of out & gt, out | gt and smoothed == score are counted,
//           a pixel that attains the maximum is tested against its phrase's boxes, and the workgroup leaves four int32
//           partials.  query_eval_final adds them per phrase.  The smoothed mask is never read back.
// Integers only, no atomics: the same bits on every run.
//
// psnr_partial / psnr_final: sum over the elements with gt > 0 of (clamp(image, 0, 1) - gt)^2 and their number.  The
// difference is float32 (as the reference's), its square and every sum double; a thread's elements, the grid and the order of
// every sum depend on the element count alone.
#include "olsr_device.h"
#include "olsr_kernels.h"

namespace olsr {

constexpr int QE_TILE = 64;                      // output tile edge: a wave's lanes along x
constexpr int QE_R = 3;                          // the window's radius
constexpr int QE_ROWS = QE_TILE + 2 * QE_R;      // staged rows (and columns) per tile
constexpr int QE_WAVES = 4;
constexpr int QE_THREADS = 64 * QE_WAVES;
constexpr int QE_OWN = QE_TILE / QE_WAVES;       // output rows per wave
constexpr int QE_WALK = QE_OWN + 2 * QE_R;       // staged rows a wave walks
constexpr int QE_STAGE = (QE_ROWS + QE_WAVES - 1) / QE_WAVES;   // rows a wave stages

struct QueryEvalArgs {
  const float* smoothed;       // [P,H,W]
  const float* score;          // [P]
  const uint8_t* gt;           // [P,H,W]
  const float* boxes;          // [B,4]
  const int32_t* box_offsets;  // [P+1], device
  int32_t* partials;           // [P][4][tiles]
};

// python's min(a, b) / max(a, b) of the reference (:214-215): the second only if it compares strictly
__device__ __forceinline__ float py_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float py_max(float a, float b) { return b > a ? b : a; }

template <bool EVAL>
__global__ __launch_bounds__(QE_THREADS) void mask_smooth_kernel(int H, int W, const uint8_t* __restrict__ in,
                                                                 uint8_t* __restrict__ out, QueryEvalArgs e) {
  __shared__ u64 s_a[QE_ROWS];   // columns x0 - 3 .. x0 + 60 of a staged row
  __shared__ u32 s_b[QE_ROWS];   // columns x0 + 61 .. x0 + 66
  __shared__ int s_part[QE_WAVES][4];
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
  const int x0 = (int)blockIdx.x * QE_TILE, y0 = (int)blockIdx.y * QE_TILE, p = (int)blockIdx.z;
  const size_t plane = (size_t)p * (size_t)H * (size_t)W;
  const uint8_t* src = in + plane;

  const int j = x0 + lane, t0 = wave * QE_OWN;
  // every load of this workgroup is issued before the first is waited for: the epilogue's operands ...
  float sv[QE_OWN];
  uint8_t gv[QE_OWN];
  if constexpr (EVAL) {
#pragma unroll
    for (int t = 0; t < QE_OWN; ++t) {
      const int i = y0 + t0 + t;
      const bool ok = i < H && j < W;
      const size_t at = plane + (size_t)(ok ? i : 0) * (size_t)W + (size_t)(ok ? j : 0);
      sv[t] = ok ? e.smoothed[at] : 0.0f;
      gv[t] = ok ? e.gt[at] : (uint8_t)0;
    }
  }
  // ... and the staged rows k = wave, wave + 4, ...
  uint8_t va[QE_STAGE], vb[QE_STAGE];
  const int ca = x0 - QE_R + lane, cb = x0 + QE_TILE - QE_R + lane;
  const bool ca_ok = ca >= 0 && ca <= W - 2, cb_ok = lane < 2 * QE_R && cb <= W - 2;
#pragma unroll
  for (int q = 0; q < QE_STAGE; ++q) {
    const int k = wave + q * QE_WAVES, r = y0 - QE_R + k;
    const bool row_ok = k < QE_ROWS && r >= 0 && r <= H - 2;   // (the same in every lane)
    const uint8_t* row = src + (size_t)(row_ok ? r : 0) * (size_t)W;
    va[q] = row_ok && ca_ok ? row[ca] : (uint8_t)0;
    vb[q] = row_ok && cb_ok ? row[cb] : (uint8_t)0;
  }
#pragma unroll
  for (int q = 0; q < QE_STAGE; ++q) {
    const int k = wave + q * QE_WAVES;
    const u64 ma = ballot(va[q] != 0), mb = ballot(vb[q] != 0);
    if (k < QE_ROWS && lane == 0) {
      s_a[k] = ma;
      s_b[k] = (u32)mb;
    }
  }
  __syncthreads();

  int h[QE_WALK];
#pragma unroll
  for (int q = 0; q < QE_WALK; ++q) {
    const u64 lo = s_a[t0 + q] >> lane;
    const u64 hi = lane ? ((u64)s_b[t0 + q] << (64 - lane)) : 0ull;
    h[q] = __popcll((lo | hi) & 0x7full);
  }
  const int cols = min(j + QE_R, W - 2) - max(j - QE_R, 0) + 1;
  float sc = 0.0f;
  int b0 = 0, b1 = 0;
  if constexpr (EVAL) {
    sc = e.score[p];
    b0 = e.box_offsets[p];
    b1 = e.box_offsets[p + 1];
  }
  int n_inter = 0, n_union = 0, n_max = 0;
  bool hit = false;
  int ones = h[0] + h[1] + h[2] + h[3] + h[4] + h[5];
#pragma unroll
  for (int t = 0; t < QE_OWN; ++t) {
    ones += h[t + 2 * QE_R];
    if (t > 0) ones -= h[t - 1];
    const int i = y0 + t0 + t;
    if (i < H) {   // (the same in every lane)
      const bool ok = j < W;
      const int rows = min(i + QE_R, H - 2) - max(i - QE_R, 0) + 1;
      const bool o = ok && 2 * ones > rows * cols;
      const size_t at = plane + (size_t)i * (size_t)W + (size_t)(ok ? j : 0);
      if (out && ok) out[at] = o ? 1 : 0;
      if constexpr (EVAL) {
        const bool g = ok && gv[t] != 0;
        const bool top = ok && sv[t] == sc;
        n_inter += __popcll(ballot(o && g));
        n_union += __popcll(ballot(o || g));
        n_max += __popcll(ballot(top));
        if (top && !hit) {
          const float x = (float)j, y = (float)i;   // (exact: both are below 2^24)
          for (int b = b0; b < b1; ++b) {
            const float x1 = e.boxes[4 * (size_t)b], y1 = e.boxes[4 * (size_t)b + 1];
            const float x2 = e.boxes[4 * (size_t)b + 2], y2 = e.boxes[4 * (size_t)b + 3];
            if (x >= py_min(x1, x2) && x <= py_max(x1, x2) && y >= py_min(y1, y2) && y <= py_max(y1, y2)) hit = true;
          }
        }
      }
    }
  }
  if constexpr (EVAL) {
    const bool any_hit = wave_any(hit);
    if (lane == 0) {
      s_part[wave][0] = n_inter;
      s_part[wave][1] = n_union;
      s_part[wave][2] = n_max;
      s_part[wave][3] = any_hit ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
      const int c = (int)threadIdx.x;
      const size_t tiles = (size_t)gridDim.x * gridDim.y, tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
      int v = 0;
#pragma unroll
      for (int w = 0; w < QE_WAVES; ++w) v += s_part[w][c];
      e.partials[((size_t)p * 4 + c) * tiles + tile] = v;
    }
  }
}

// result[p] = {intersection, union, n_max, hit}: the tiles' partials added up; one workgroup per phrase
__global__ __launch_bounds__(QE_THREADS) void query_eval_final(int tiles, const int32_t* __restrict__ partials,
                                                               int32_t* __restrict__ result) {
  __shared__ int s_w[QE_WAVES];
  const int p = (int)blockIdx.x;
  for (int c = 0; c < 4; ++c) {
    const int v = single_block_sum<QE_WAVES>(tiles, partials + ((size_t)p * 4 + c) * (size_t)tiles, s_w);
    if (threadIdx.x == 0) result[4 * (size_t)p + c] = c == 3 ? (v > 0 ? 1 : 0) : v;
    __syncthreads();   // (s_w is rewritten by the next sum)
  }
}

size_t query_eval_tiles(int H, int W) {
  return (size_t)((H + QE_TILE - 1) / QE_TILE) * (size_t)((W + QE_TILE - 1) / QE_TILE);
}

struct QueryEvalScratch {
  int32_t* offsets;    // [P + 1]: where the entry parks offsets that arrived in host memory
  int32_t* partials;   // [P][4][tiles]
  static QueryEvalScratch carve(void* buf, int P, int H, int W, size_t& bytes) {
    Carver c(buf);
    QueryEvalScratch s;
    s.offsets = c.take<int32_t>((size_t)P + 1);
    s.partials = c.take<int32_t>((size_t)P * 4 * query_eval_tiles(H, W));
    bytes = c.total();
    return s;
  }
};

size_t query_eval_scratch_bytes(int P, int H, int W) {
  size_t bytes = 0;
  QueryEvalScratch::carve(nullptr, P > 0 ? P : 0, H > 0 ? H : 0, W > 0 ? W : 0, bytes);
  return bytes;
}
int32_t* query_eval_scratch_offsets(void* scratch, int P, int H, int W) {
  size_t bytes;
  return QueryEvalScratch::carve(scratch, P, H, W, bytes).offsets;
}

static dim3 smooth_grid(int P, int H, int W) {
  return dim3((W + QE_TILE - 1) / QE_TILE, (H + QE_TILE - 1) / QE_TILE, P);
}

void launch_mask_smooth(int P, int H, int W, const uint8_t* mask_in, uint8_t* mask_out, hipStream_t st) {
  mask_smooth_kernel<false><<<smooth_grid(P, H, W), QE_THREADS, 0, st>>>(H, W, mask_in, mask_out, QueryEvalArgs{});
}

void launch_query_eval(int P, int H, int W, const uint8_t* mask, const float* smoothed, const float* score,
                       const uint8_t* gt_mask, const float* boxes, const int32_t* box_offsets_dev, int32_t* result,
                       uint8_t* mask_smoothed, void* scratch, hipStream_t st) {
  size_t bytes;
  const QueryEvalScratch s = QueryEvalScratch::carve(scratch, P, H, W, bytes);
  QueryEvalArgs e;
  e.smoothed = smoothed, e.score = score, e.gt = gt_mask, e.boxes = boxes, e.box_offsets = box_offsets_dev;
  e.partials = s.partials;
  mask_smooth_kernel<true><<<smooth_grid(P, H, W), QE_THREADS, 0, st>>>(H, W, mask, mask_smoothed, e);
  query_eval_final<<<P, QE_THREADS, 0, st>>>((int)query_eval_tiles(H, W), s.partials, result);
}

// --------------------------------------------------------------------------------------------------------------- masked PSNR
constexpr int PS_WAVES = 4;
constexpr int PS_THREADS = 64 * PS_WAVES;
constexpr int PS_MAX_BLOCKS = 1024;

static int psnr_blocks(long long n) {
  const long long chunks = (n + 3) / 4, nb = (chunks + PS_THREADS - 1) / PS_THREADS;
  return (int)(nb < 1 ? 1 : (nb < PS_MAX_BLOCKS ? nb : PS_MAX_BLOCKS));
}

// thread c, c + threads, ... takes the elements 4 c .. 4 c + 3 (one 16-byte load where both arrays allow it: `vec`)
__global__ __launch_bounds__(PS_THREADS) void psnr_partial(long long n, int vec, const float* __restrict__ image,
                                                           const float* __restrict__ gt, double* __restrict__ partials) {
  __shared__ double s_sum[PS_WAVES];
  __shared__ long long s_cnt[PS_WAVES];
  const long long chunks = (n + 3) / 4, step = (long long)gridDim.x * PS_THREADS;
  double sum = 0.0;
  long long cnt = 0;
  for (long long c = (long long)blockIdx.x * PS_THREADS + threadIdx.x; c < chunks; c += step) {
    const long long base = 4 * c;
    float a[4], g[4];
    if (vec && base + 4 <= n) {
      const float4 av = *reinterpret_cast<const float4*>(image + base), gv = *reinterpret_cast<const float4*>(gt + base);
      a[0] = av.x, a[1] = av.y, a[2] = av.z, a[3] = av.w;
      g[0] = gv.x, g[1] = gv.y, g[2] = gv.z, g[3] = gv.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = base + k < n;
        a[k] = ok ? image[base + k] : 0.0f;
        g[k] = ok ? gt[base + k] : 0.0f;   // (0: not in the mask)
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (g[k] > 0.0f) {
        const float v = a[k] < 0.0f ? 0.0f : (a[k] > 1.0f ? 1.0f : a[k]);   // torch.clamp: a NaN stays
        const float d = v - g[k];
        sum += (double)d * (double)d;
        ++cnt;
      }
    }
  }
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  if (lane_id() == 0) {
    s_sum[threadIdx.x >> 6] = sum;
    s_cnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = s_sum[0];
    long long m = s_cnt[0];
#pragma unroll
    for (int w = 1; w < PS_WAVES; ++w) s += s_sum[w], m += s_cnt[w];
    partials[blockIdx.x] = s;
    partials[gridDim.x + blockIdx.x] = (double)m;
  }
}

__global__ __launch_bounds__(PS_THREADS) void psnr_final(int nb, const double* __restrict__ partials, double* __restrict__ out) {
  __shared__ double s_w[PS_WAVES];
  const double s = single_block_sum<PS_WAVES>(nb, partials, s_w);
  __syncthreads();   // (s_w is rewritten by the next sum)
  const double m = single_block_sum<PS_WAVES>(nb, partials + nb, s_w);
  if (threadIdx.x == 0) out[0] = s, out[1] = m;
}

size_t image_psnr_scratch_bytes() {
  Carver c(nullptr);
  c.take<double>(2 * (size_t)PS_MAX_BLOCKS);
  return c.total();
}

void launch_image_psnr(long long n, const float* image, const float* gt, double* out, void* scratch, hipStream_t st) {
  Carver c(scratch);
  double* partials = c.take<double>(2 * (size_t)PS_MAX_BLOCKS);
  const int nb = psnr_blocks(n);
  const int vec = ((reinterpret_cast<uintptr_t>(image) | reinterpret_cast<uintptr_t>(gt)) & 15u) == 0 ? 1 : 0;
  psnr_partial<<<nb, PS_THREADS, 0, st>>>(n, vec, image, gt, partials);
  psnr_final<<<1, PS_THREADS, 0, st>>>(nb, partials, out);
}

}  // namespace olsr
