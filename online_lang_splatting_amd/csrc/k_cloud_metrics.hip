// k_cloud_metrics.hip — Chamfer distance and the approximate earth mover's distance between point clouds (include/olsr.h,
// "point-cloud metrics"): the two numbers the reference's 3-D evaluation reports per queried class
// (tsdf-fusion/3d_evaluation_and_visualize_langslam_dim15.py:396-423; chamfer_distance :235-274, earth_mover_distance of
// tsdf-fusion/emd.py over PyTorchEMD's approxmatch / matchcost).
//
// The reference's approxmatch gives a batch item ONE 512-thread block and writes a dense match[m,n] matrix that only matchcost
// reads again.  Here the matching is matrix-free — step 3 adds d * w where the reference adds w into the matrix — and both
// axes are split over workgroups:
//
//   all-pairs skeleton   a 256-thread workgroup keeps CM_OWN "own" points per thread in registers (a tile of 512) and streams
//                        a chunk of the other cloud through LDS, 256 records {x, y, z, weight} of 16 bytes at a time.  Every
//                        lane reads the same record (one ds_read_b128, a broadcast, no bank conflict) and uses it for its
//                        CM_OWN points, so a pair costs half an LDS read (by the instruction counts; not measured).
//   ragged batches       B segments given by int32[B+1] offsets into packed point arrays; blockIdx.z is the segment,
//                        blockIdx.x the own tile, blockIdx.y the chunk of the streamed axis.  A workgroup beyond its segment's
//                        sizes returns at once.  Tile and chunk bounds depend on the segment's own sizes only, so a segment's
//                        bits do not depend on what else is in the batch.
//   chunks               the streamed axis of s points is cut into at most CM_MAX_CHUNKS chunks of cm_chunk_len(s) points (a
//                        multiple of 256); each chunk leaves a float32 partial per own point, and whoever reads the sum next adds
//                        the partials in chunk order.  No floating-point atomics anywhere.
//
// EMD, per level (level = -4^j, j = 7 .. -1, then 0; c = level * log2(e) in float32; e = v_exp_f32(c * d)):
//   emd_cols   step 2, column-parallel.  While it stages the rows it finishes the row state of the level before:
//              remainL = max(0, remainL - sum of the step-3 partials), ratioL = remainL / (1e-9 + sum of the step-1 partials),
//              and the row's cost so far (double) takes the d * w partials.  Writes, per column and row chunk, sum_k e * ratioL.
//   emd_rows   step 3 of this level and the sum of step 1 of the next in one walk of a row tile over a column chunk.  While it
//              stages the columns it finishes step 2: sumr = (sum of emd_cols' partials) * remainR, ratioR, remainR.  Writes
//              per row and column chunk: sum_l w, sum_l d * w (float32, as the reference's per-thread sums) and sum_l e' * remainR.
// remainL and remainR are double-buffered by the level's parity: the workgroups of own tile 0 write the new values while the
// others still read the old ones.  One emd_rows in front (step 1 of the first level), emd_final behind (last remainL, the
// residuals, the cost over rows in double, fixed order): 1 + 1 + 2 * 10 + 1 = 23 launches for any B and any sizes, nothing
// read back in between.
// Exact skips: an LDS tile whose weights are all exactly zero adds exact zeros (e is finite, in [0, 1]) and is not walked.
//
// Chamfer: chamfer_pairs keeps, per own point and chunk, the least d = (dx dx + dy dy) + dz dz (no contraction: build.py) and
// the lowest index attaining it; chamfer_final takes the least over the chunks (lower chunk first, strict <), writes min_d2
// and nn, and sums sqrt in double per segment and direction in a fixed order.  Two launches.  Brute force: n * m pairs.
#include "olsr_device.h"
#include "olsr_kernels.h"

namespace olsr {

constexpr int CM_THREADS = 256;
constexpr int CM_OWN = 2;                       // own points per thread
constexpr int CM_TILE = CM_THREADS * CM_OWN;    // own points per workgroup
constexpr int CM_LDS = 256;                     // streamed points per LDS tile
constexpr int CM_MAX_CHUNKS = 16;               // chunks of the streamed axis (partials kept per own point)
constexpr int CM_LEVELS = 10;

// the chunk length of a streamed axis of s >= 1 points (a multiple of CM_LDS) and the number of chunks it makes (<= 16)
__host__ __device__ __forceinline__ int cm_chunk_len(int s) {
  const int tiles = (s + CM_LDS - 1) / CM_LDS;
  const int chunks = tiles < CM_MAX_CHUNKS ? tiles : CM_MAX_CHUNKS;
  return ((tiles + chunks - 1) / chunks) * CM_LDS;
}
__host__ __device__ __forceinline__ int cm_chunks(int s) {
  const int len = cm_chunk_len(s);
  return (s + len - 1) / len;
}

struct EmdArgs {
  const int32_t *off1, *off2;
  const float *xyz1, *xyz2;
  long long total1, total2;   // strides of the partial arrays
  float *remainL, *remainR;   // [2][total]
  float* ratioL;              // [total1]
  float *PA, *PC, *PD;        // [16][total1]: step-1 sums, step-3 sums, d * w sums, per column chunk
  float* PB;                  // [16][total2]: step-2 sums per row chunk
  double* rowcost;            // [total1]
};

struct Segment {
  int o1, n, o2, m;
  __device__ __forceinline__ bool live() const { return n > 0 && m > 0; }
};
__device__ __forceinline__ Segment segment_of(const int32_t* off1, const int32_t* off2, int b) {
  Segment s;
  s.o1 = off1[b];
  s.n = off1[b + 1] - s.o1;
  s.o2 = off2[b];
  s.m = off2[b + 1] - s.o2;
  return s;
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = bx - ax, dy = by - ay, dz = bz - az;
  return (dx * dx + dy * dy) + dz * dz;
}
// the reference's __expf(level * d): the hardware's 2^x on level * log2(e) * d
__device__ __forceinline__ float exp_level(float c, float d) { return __builtin_amdgcn_exp2f(c * d); }

__device__ __forceinline__ float sum_partials(const float* __restrict__ p, long long stride, int chunks) {
  float s = p[0];
  for (int c = 1; c < chunks; ++c) s += p[(long long)c * stride];
  return s;
}

// remainL = multiL, remainR = multiR (buffer 0), the rows' cost = 0
__global__ __launch_bounds__(CM_THREADS) void emd_init(EmdArgs a) {
  const Segment s = segment_of(a.off1, a.off2, blockIdx.y);
  if (!s.live()) return;
  const float multiL = s.n >= s.m ? 1.0f : (float)(s.m / s.n);
  const float multiR = s.n >= s.m ? (float)(s.n / s.m) : 1.0f;
  for (int k = blockIdx.x * CM_THREADS + threadIdx.x; k < s.n; k += gridDim.x * CM_THREADS) {
    a.remainL[s.o1 + k] = multiL;
    a.rowcost[s.o1 + k] = 0.0;
  }
  for (int l = blockIdx.x * CM_THREADS + threadIdx.x; l < s.m; l += gridDim.x * CM_THREADS) a.remainR[s.o2 + l] = multiR;
}

// step 2: own = columns, streamed = rows with weight ratioL.  first: no level before this one.  par: which remainL is current.
__global__ __launch_bounds__(CM_THREADS) void emd_cols(EmdArgs a, float c, int first, int par) {
  const Segment s = segment_of(a.off1, a.off2, blockIdx.z);
  if (!s.live()) return;
  const int l_tile = blockIdx.x * CM_TILE;
  if (l_tile >= s.m) return;
  const int len = cm_chunk_len(s.n);
  const int k0 = blockIdx.y * len;
  if (k0 >= s.n) return;
  const int k1 = min(s.n, k0 + len);
  const int col_chunks = cm_chunks(s.m);   // partials per row
  const bool writer = blockIdx.x == 0;

  float x[CM_OWN], y[CM_OWN], z[CM_OWN], acc[CM_OWN];
  bool ok[CM_OWN];
#pragma unroll
  for (int r = 0; r < CM_OWN; ++r) {
    const int l = l_tile + r * CM_THREADS + threadIdx.x;
    ok[r] = l < s.m;
    const float* p = a.xyz2 + 3 * (size_t)(s.o2 + (ok[r] ? l : 0));
    x[r] = p[0], y[r] = p[1], z[r] = p[2];
    acc[r] = 0.0f;
  }
  __shared__ float4 rec[CM_LDS];
  const float* remain_in = a.remainL + (size_t)par * a.total1;
  float* remain_out = a.remainL + (size_t)(par ^ 1) * a.total1;
  for (int kt = k0; kt < k1; kt += CM_LDS) {
    const int k = kt + threadIdx.x;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < k1) {
      const size_t g = (size_t)(s.o1 + k);
      const float* p = a.xyz1 + 3 * g;
      float rem = remain_in[g];
      if (!first) rem = fmaxf(0.0f, rem - sum_partials(a.PC + g, a.total1, col_chunks));
      const float ratio = rem / (1e-9f + sum_partials(a.PA + g, a.total1, col_chunks));
      q = make_float4(p[0], p[1], p[2], ratio);
      if (writer) {
        remain_out[g] = rem;
        a.ratioL[g] = ratio;
        if (!first) {
          double cost = a.rowcost[g];
          for (int cc = 0; cc < col_chunks; ++cc) cost += (double)a.PD[(long long)cc * a.total1 + g];
          a.rowcost[g] = cost;
        }
      }
    }
    // (also: everyone is done with the tile before)
    if (!__syncthreads_or(q.w != 0.0f)) continue;   // a tile of exact zeros adds exact zeros
    rec[threadIdx.x] = q;
    __syncthreads();
    const int cnt = min(CM_LDS, k1 - kt);
    for (int i = 0; i < cnt; ++i) {
      const float4 t = rec[i];
#pragma unroll
      for (int r = 0; r < CM_OWN; ++r) acc[r] += exp_level(c, dist2(t.x, t.y, t.z, x[r], y[r], z[r])) * t.w;
    }
  }
#pragma unroll
  for (int r = 0; r < CM_OWN; ++r)
    if (ok[r]) a.PB[(long long)blockIdx.y * a.total2 + s.o2 + l_tile + r * CM_THREADS + threadIdx.x] = acc[r];
}

// step 3 of the level c3 (DO3) and the sum of step 1 of the level c1 (DO1): own = rows, streamed = columns.
// par: which remainR is current.
template <bool DO3, bool DO1>
__global__ __launch_bounds__(CM_THREADS) void emd_rows(EmdArgs a, float c3, float c1, int par) {
  const Segment s = segment_of(a.off1, a.off2, blockIdx.z);
  if (!s.live()) return;
  const int k_tile = blockIdx.x * CM_TILE;
  if (k_tile >= s.n) return;
  const int len = cm_chunk_len(s.m);
  const int l0 = blockIdx.y * len;
  if (l0 >= s.m) return;
  const int l1 = min(s.m, l0 + len);
  const int row_chunks = cm_chunks(s.n);   // partials per column
  const bool writer = blockIdx.x == 0;

  float x[CM_OWN], y[CM_OWN], z[CM_OWN], rl[CM_OWN], sw[CM_OWN], sd[CM_OWN], sa[CM_OWN];
  bool ok[CM_OWN];
#pragma unroll
  for (int r = 0; r < CM_OWN; ++r) {
    const int k = k_tile + r * CM_THREADS + threadIdx.x;
    ok[r] = k < s.n;
    const size_t g = (size_t)(s.o1 + (ok[r] ? k : 0));
    const float* p = a.xyz1 + 3 * g;
    x[r] = p[0], y[r] = p[1], z[r] = p[2];
    rl[r] = (DO3 && ok[r]) ? a.ratioL[g] : 0.0f;
    sw[r] = sd[r] = sa[r] = 0.0f;
  }
  __shared__ float4 rec[CM_LDS];   // x, y, z, ratioR
  __shared__ float next_w[CM_LDS];  // remainR of the next level
  const float* remain_in = a.remainR + (size_t)par * a.total2;
  float* remain_out = a.remainR + (size_t)(par ^ 1) * a.total2;
  for (int lt = l0; lt < l1; lt += CM_LDS) {
    const int l = lt + threadIdx.x;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    float w1 = 0.0f;
    if (l < l1) {
      const size_t g = (size_t)(s.o2 + l);
      const float* p = a.xyz2 + 3 * g;
      const float rem = remain_in[g];
      q = make_float4(p[0], p[1], p[2], 0.0f);
      w1 = rem;
      if constexpr (DO3) {
        const float sumr = sum_partials(a.PB + g, a.total2, row_chunks) * rem;
        q.w = fminf(rem / (sumr + 1e-9f), 1.0f) * rem;
        w1 = fmaxf(0.0f, rem - sumr);
        if (writer) remain_out[g] = w1;
      }
    }
    if (!__syncthreads_or(q.w != 0.0f || (DO1 && w1 != 0.0f))) continue;
    rec[threadIdx.x] = q;
    if constexpr (DO1) next_w[threadIdx.x] = w1;
    __syncthreads();
    const int cnt = min(CM_LDS, l1 - lt);
    for (int i = 0; i < cnt; ++i) {
      const float4 t = rec[i];
      float tw = 0.0f;
      if constexpr (DO1) tw = next_w[i];
#pragma unroll
      for (int r = 0; r < CM_OWN; ++r) {
        const float d = dist2(x[r], y[r], z[r], t.x, t.y, t.z);
        if constexpr (DO3) {
          const float w = exp_level(c3, d) * rl[r] * t.w;
          sw[r] += w;
          sd[r] += d * w;
        }
        if constexpr (DO1) sa[r] += exp_level(c1, d) * tw;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < CM_OWN; ++r) {
    if (!ok[r]) continue;
    const long long at = (long long)blockIdx.y * a.total1 + s.o1 + k_tile + r * CM_THREADS + threadIdx.x;
    if constexpr (DO3) a.PC[at] = sw[r], a.PD[at] = sd[r];
    if constexpr (DO1) a.PA[at] = sa[r];
  }
}

// fixed-order sum of one double per thread over the workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int h = CM_THREADS / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  return red[0];
}

// the last level's remainL, the residuals and the cost; one workgroup per segment.  par: the buffers the last level read.
__global__ __launch_bounds__(CM_THREADS) void emd_final(EmdArgs a, int par, double* __restrict__ cost,
                                                        float* __restrict__ residual, int32_t* __restrict__ valid) {
  const int b = blockIdx.x;
  const Segment s = segment_of(a.off1, a.off2, b);
  __shared__ double red[CM_THREADS];
  if (!s.live()) {
    if (threadIdx.x == 0) {
      cost[b] = __builtin_nan("");
      if (residual) residual[2 * b] = residual[2 * b + 1] = __builtin_nanf("");
      valid[b] = 0;
    }
    return;
  }
  const int col_chunks = cm_chunks(s.m);
  const float* remL = a.remainL + (size_t)(par ^ 1) * a.total1;   // what emd_cols left: before the last step 3
  const float* remR = a.remainR + (size_t)(par ^ 1) * a.total2;   // what the last emd_rows left
  double c = 0.0, rL = 0.0, rR = 0.0;
  for (int k = threadIdx.x; k < s.n; k += CM_THREADS) {
    const size_t g = (size_t)(s.o1 + k);
    double ck = a.rowcost[g];
    for (int cc = 0; cc < col_chunks; ++cc) ck += (double)a.PD[(long long)cc * a.total1 + g];
    c += ck;
    rL += (double)fmaxf(0.0f, remL[g] - sum_partials(a.PC + g, a.total1, col_chunks));
  }
  for (int l = threadIdx.x; l < s.m; l += CM_THREADS) rR += (double)remR[s.o2 + l];
  c = block_sum(c, red);
  rL = block_sum(rL, red);
  rR = block_sum(rR, red);
  if (threadIdx.x == 0) {
    cost[b] = c;
    if (residual) residual[2 * b] = (float)rL, residual[2 * b + 1] = (float)rR;
    valid[b] = 1;
  }
}

struct EmdScratch {
  int32_t *off1, *off2;
  EmdArgs a;
  static EmdScratch carve(void* buf, int B, size_t t1, size_t t2, size_t& bytes) {
    Carver c(buf);
    EmdScratch e;
    e.off1 = c.take<int32_t>((size_t)B + 1);
    e.off2 = c.take<int32_t>((size_t)B + 1);
    e.a.rowcost = c.take<double>(t1);
    e.a.remainL = c.take<float>(2 * t1);
    e.a.remainR = c.take<float>(2 * t2);
    e.a.ratioL = c.take<float>(t1);
    e.a.PA = c.take<float>(CM_MAX_CHUNKS * t1);
    e.a.PC = c.take<float>(CM_MAX_CHUNKS * t1);
    e.a.PD = c.take<float>(CM_MAX_CHUNKS * t1);
    e.a.PB = c.take<float>(CM_MAX_CHUNKS * t2);
    e.a.total1 = (long long)t1;
    e.a.total2 = (long long)t2;
    bytes = c.total();
    return e;
  }
};

size_t emd_scratch_bytes(int B, long long total1, long long total2) {
  size_t bytes = 0;
  EmdScratch::carve(nullptr, B > 0 ? B : 0, (size_t)(total1 > 0 ? total1 : 0), (size_t)(total2 > 0 ? total2 : 0), bytes);
  return bytes;
}
int32_t* emd_scratch_offsets(void* scratch, int B, long long total1, long long total2, int which) {
  size_t bytes;
  const EmdScratch e = EmdScratch::carve(scratch, B, (size_t)total1, (size_t)total2, bytes);
  return which ? e.off2 : e.off1;
}

static int tiles_of(int n) { return n > 0 ? (n + CM_TILE - 1) / CM_TILE : 1; }
// the grid's chunk axis: cm_chunks is not monotonic in the size (4 096 points make 16 chunks, 4 100 make 9), so the axis is
// sized by a bound that holds for every segment of at most n points; workgroups beyond a segment's own count return
static int chunks_of(int n) {
  const int tiles = (n + CM_LDS - 1) / CM_LDS;
  return tiles < 1 ? 1 : (tiles < CM_MAX_CHUNKS ? tiles : CM_MAX_CHUNKS);
}

void launch_emd_cost(int B, const int32_t* off1, const int32_t* off2, long long total1, long long total2, int max_n1,
                     int max_n2, const float* xyz1, const float* xyz2, double* cost, float* residual, int32_t* valid,
                     void* scratch, hipStream_t st) {
  size_t bytes;
  EmdArgs a = EmdScratch::carve(scratch, B, (size_t)total1, (size_t)total2, bytes).a;
  a.off1 = off1, a.off2 = off2, a.xyz1 = xyz1, a.xyz2 = xyz2;
  if (max_n1 > 0 && max_n2 > 0) {
    const dim3 rows(tiles_of(max_n1), chunks_of(max_n2), B), cols(tiles_of(max_n2), chunks_of(max_n1), B);
    const int longest = max_n1 > max_n2 ? max_n1 : max_n2;
    emd_init<<<dim3(min(64, (longest + CM_THREADS - 1) / CM_THREADS), B), CM_THREADS, 0, st>>>(a);
    float c[CM_LEVELS];
    for (int i = 0; i < CM_LEVELS; ++i) {
      const int j = 7 - i;
      c[i] = j == -2 ? 0.0f : (float)(-ldexp(1.0, 2 * j) * 1.4426950408889634);   // level * log2(e)
    }
    emd_rows<false, true><<<rows, CM_THREADS, 0, st>>>(a, 0.0f, c[0], 0);
    for (int i = 0; i < CM_LEVELS; ++i) {
      emd_cols<<<cols, CM_THREADS, 0, st>>>(a, c[i], i == 0, i & 1);
      if (i + 1 < CM_LEVELS)
        emd_rows<true, true><<<rows, CM_THREADS, 0, st>>>(a, c[i], c[i + 1], i & 1);
      else
        emd_rows<true, false><<<rows, CM_THREADS, 0, st>>>(a, c[i], 0.0f, i & 1);
    }
  }
  emd_final<<<B, CM_THREADS, 0, st>>>(a, (CM_LEVELS - 1) & 1, cost, residual, valid);
}

// ---------------------------------------------------------------------------------------------------------------- Chamfer
struct ChamferArgs {
  const int32_t *off1, *off2;
  const float *xyz1, *xyz2;
  long long total1, total2;
  float *pd1, *pd2;     // [16][total]: the least d per chunk of the other cloud
  int32_t *pi1, *pi2;   // and the lowest segment-local index attaining it
};

// blockIdx.z = 2 * segment + direction (0: own = cloud 1, streamed = cloud 2)
__global__ __launch_bounds__(CM_THREADS) void chamfer_pairs(ChamferArgs a) {
  const int dir = blockIdx.z & 1;
  const Segment s0 = segment_of(a.off1, a.off2, blockIdx.z >> 1);
  if (!s0.live()) return;
  const int oo = dir ? s0.o2 : s0.o1, no = dir ? s0.m : s0.n;   // own
  const int os = dir ? s0.o1 : s0.o2, ns = dir ? s0.n : s0.m;   // streamed
  const float* own = dir ? a.xyz2 : a.xyz1;
  const float* str = dir ? a.xyz1 : a.xyz2;
  const int tile = blockIdx.x * CM_TILE;
  if (tile >= no) return;
  const int len = cm_chunk_len(ns);
  const int l0 = blockIdx.y * len;
  if (l0 >= ns) return;
  const int l1 = min(ns, l0 + len);
  float x[CM_OWN], y[CM_OWN], z[CM_OWN], best[CM_OWN];
  int at[CM_OWN];
  bool ok[CM_OWN];
#pragma unroll
  for (int r = 0; r < CM_OWN; ++r) {
    const int k = tile + r * CM_THREADS + threadIdx.x;
    ok[r] = k < no;
    const float* p = own + 3 * (size_t)(oo + (ok[r] ? k : 0));
    x[r] = p[0], y[r] = p[1], z[r] = p[2];
    best[r] = __builtin_inff();
    at[r] = l0;
  }
  __shared__ float4 rec[CM_LDS];
  for (int lt = l0; lt < l1; lt += CM_LDS) {
    const int l = lt + threadIdx.x;
    __syncthreads();
    if (l < l1) {
      const float* p = str + 3 * (size_t)(os + l);
      rec[threadIdx.x] = make_float4(p[0], p[1], p[2], 0.0f);
    }
    __syncthreads();
    const int cnt = min(CM_LDS, l1 - lt);
    for (int i = 0; i < cnt; ++i) {
      const float4 t = rec[i];
#pragma unroll
      for (int r = 0; r < CM_OWN; ++r) {
        const float d = dist2(x[r], y[r], z[r], t.x, t.y, t.z);
        if (d < best[r]) best[r] = d, at[r] = lt + i;
      }
    }
  }
  float* pd = dir ? a.pd2 : a.pd1;
  int32_t* pi = dir ? a.pi2 : a.pi1;
  const long long stride = dir ? a.total2 : a.total1;
#pragma unroll
  for (int r = 0; r < CM_OWN; ++r) {
    if (!ok[r]) continue;
    const long long g = (long long)blockIdx.y * stride + oo + tile + r * CM_THREADS + threadIdx.x;
    pd[g] = best[r];
    pi[g] = at[r];
  }
}

// one workgroup per segment and direction: the least over the chunks, sqrt, the mean
__global__ __launch_bounds__(CM_THREADS) void chamfer_final(ChamferArgs a, float* __restrict__ min1, int32_t* __restrict__ nn1,
                                                            float* __restrict__ min2, int32_t* __restrict__ nn2,
                                                            double* __restrict__ mean, int32_t* __restrict__ valid) {
  const int dir = blockIdx.x & 1, b = blockIdx.x >> 1;
  const Segment s0 = segment_of(a.off1, a.off2, b);
  const int oo = dir ? s0.o2 : s0.o1, no = dir ? s0.m : s0.n, ns = dir ? s0.n : s0.m;
  float* mind = dir ? min2 : min1;
  int32_t* nn = dir ? nn2 : nn1;
  __shared__ double red[CM_THREADS];
  if (!s0.live()) {
    for (int k = threadIdx.x; k < no; k += CM_THREADS) {
      mind[oo + k] = __builtin_nanf("");
      nn[oo + k] = -1;
    }
    if (threadIdx.x == 0) {
      mean[2 * b + dir] = __builtin_nan("");
      if (dir == 0) valid[b] = 0;
    }
    return;
  }
  const float* pd = dir ? a.pd2 : a.pd1;
  const int32_t* pi = dir ? a.pi2 : a.pi1;
  const long long stride = dir ? a.total2 : a.total1;
  const int chunks = cm_chunks(ns);
  double sum = 0.0;
  for (int k = threadIdx.x; k < no; k += CM_THREADS) {
    const long long g = oo + k;
    float d = pd[g];
    int i = pi[g];
    for (int c = 1; c < chunks; ++c) {
      const float dc = pd[(long long)c * stride + g];
      if (dc < d) d = dc, i = pi[(long long)c * stride + g];
    }
    mind[g] = d;
    nn[g] = i;
    sum += sqrt((double)d);
  }
  sum = block_sum(sum, red);
  if (threadIdx.x == 0) {
    mean[2 * b + dir] = sum / (double)no;
    if (dir == 0) valid[b] = 1;
  }
}

struct ChamferScratch {
  int32_t *off1, *off2;
  ChamferArgs a;
  static ChamferScratch carve(void* buf, int B, size_t t1, size_t t2, size_t& bytes) {
    Carver c(buf);
    ChamferScratch e;
    e.off1 = c.take<int32_t>((size_t)B + 1);
    e.off2 = c.take<int32_t>((size_t)B + 1);
    e.a.pd1 = c.take<float>(CM_MAX_CHUNKS * t1);
    e.a.pi1 = c.take<int32_t>(CM_MAX_CHUNKS * t1);
    e.a.pd2 = c.take<float>(CM_MAX_CHUNKS * t2);
    e.a.pi2 = c.take<int32_t>(CM_MAX_CHUNKS * t2);
    e.a.total1 = (long long)t1;
    e.a.total2 = (long long)t2;
    bytes = c.total();
    return e;
  }
};

size_t chamfer_scratch_bytes(int B, long long total1, long long total2) {
  size_t bytes = 0;
  ChamferScratch::carve(nullptr, B > 0 ? B : 0, (size_t)(total1 > 0 ? total1 : 0), (size_t)(total2 > 0 ? total2 : 0), bytes);
  return bytes;
}
int32_t* chamfer_scratch_offsets(void* scratch, int B, long long total1, long long total2, int which) {
  size_t bytes;
  const ChamferScratch e = ChamferScratch::carve(scratch, B, (size_t)total1, (size_t)total2, bytes);
  return which ? e.off2 : e.off1;
}

void launch_chamfer(int B, const int32_t* off1, const int32_t* off2, long long total1, long long total2, int max_n1, int max_n2,
                    const float* xyz1, const float* xyz2, float* min_d2_1, int32_t* nn_1, float* min_d2_2, int32_t* nn_2,
                    double* mean, int32_t* valid, void* scratch, hipStream_t st) {
  size_t bytes;
  ChamferArgs a = ChamferScratch::carve(scratch, B, (size_t)total1, (size_t)total2, bytes).a;
  a.off1 = off1, a.off2 = off2, a.xyz1 = xyz1, a.xyz2 = xyz2;
  if (max_n1 > 0 && max_n2 > 0) {
    const int longest = max_n1 > max_n2 ? max_n1 : max_n2;
    chamfer_pairs<<<dim3(tiles_of(longest), chunks_of(longest), 2 * B), CM_THREADS, 0, st>>>(a);
  }
  chamfer_final<<<2 * B, CM_THREADS, 0, st>>>(a, min_d2_1, nn_1, min_d2_2, nn_2, mean, valid);
}

}  // namespace olsr
