// k_map_edit.hip — densify, prune and extend the Gaussian map on the fused buffers (include/olsr.h, "map edits").
//
// The reference changes the number of Gaussians in its back end all the time (gaussian_splatting/scene/gaussian_model.py:
// densify_and_clone :912-946, densify_and_split :855-910, prune_points :751-777, densification_postfix :813-853,
// extend_from_pcd :283-350): every edit rebuilds each parameter, both Adam moments and the accumulators with torch.cat and
// boolean indexing — a dozen passes over the map per edit and a host round trip per mask.  Here every edit is one primitive:
//
//   plan   (two launches)  map_edit_classify: one byte per source row (keep / clone / split / drop) and per block of
//                          ME_ROWS rows the counts of the three output segments; map_edit_prefix: one block prefixes those
//                          counts over the blocks (in block order: deterministic, no atomics) and writes the status.
//   apply  (one launch)    map_edit_apply: a block re-reads its rows' classes, ranks them inside the block (wave ballots),
//                          computes the split children in registers, then streams every source element once — parameters
//                          and moments in the bucket layout [11 + 3M + F] — to its one, two or three destination rows.
//
// Output order is the reference's: kept originals, kept clones, kept children k = 0, kept children k = 1 (`.repeat(N, 1)`),
// appended rows; every segment in source order.  Split children follow the torch expressions operation for operation (the
// translation unit is compiled without FMA contraction, build.py): build_rotation (general_utils.py:113-135), bmm as the
// three-term sum left to right, log(exp(s) / 1.6).  The only host synchronisation of an edit is the caller's read of
// status[0] = P_new between plan and apply, which sizes the destination.
//
// HBM-bound: the apply reads 3 (11 + 3M + F) + 6 floats per source row and writes the same per destination row.
#include "olsr_device.h"
#include "olsr_kernels.h"

namespace olsr {

constexpr int ME_ROWS = 256;  // rows per block, plan and apply alike (one thread per row in the per-row phases)
constexpr int ME_WAVES = ME_ROWS / 64;
constexpr int ME_PREFIX_THREADS = 1024;

// class byte of a source row
constexpr uint8_t ME_KEEP = 1, ME_CLONE = 2, ME_CHILD = 4;

__host__ __device__ inline int me_blocks(int P) { return (P + ME_ROWS - 1) / ME_ROWS; }

struct MeScratch {
  uint8_t* cls;      // [P rounded up to 16] class bytes
  int32_t* counts;   // [3 x nb] block counts
  int32_t* offsets;  // [3 x nb] block offsets
  static MeScratch carve(void* buf, int P, size_t& bytes) {
    Carver c(buf);
    const size_t nb = (size_t)me_blocks(P);
    MeScratch s;
    s.cls = c.take<uint8_t>(((size_t)P + 15) / 16 * 16);
    s.counts = c.take<int32_t>(3 * nb);
    s.offsets = c.take<int32_t>(3 * nb);
    bytes = c.total();
    return s;
  }
};

size_t map_edit_scratch_bytes(int P) {
  size_t bytes = 0;
  MeScratch::carve(nullptr, P > 0 ? P : 0, bytes);
  return bytes;
}

__device__ inline float me_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// the class of source row j in densify mode
__device__ inline uint8_t me_densify_class(const olsr_map_edit_params& p, const olsr_map_buffers& src, int j) {
  const float accum = src.stats[2 * j], denom = src.stats[2 * j + 1];
  float g = accum / denom;                   // grads = xyz_gradient_accum / denom
  if (g != g) g = 0.0f;                      // grads[grads.isnan()] = 0.0
  const float s0 = expf(src.scales[3 * j]), s1 = expf(src.scales[3 * j + 1]), s2 = expf(src.scales[3 * j + 2]);
  const float smax = me_max3(s0, s1, s2);    // torch.max(get_scaling, dim=1).values
  const bool clone = fabsf(g) >= p.max_grad && smax <= p.clone_max_scale;  // torch.norm over a [P,1] row: |g|
  const bool split = g >= p.max_grad && smax > p.clone_max_scale;          // padded_grad: clones never split
  const bool low_opacity = act_sigmoid(src.opacities[j]) < p.min_opacity;
  const bool big = p.screen_size_term && smax > p.big_scale;
  uint8_t c = 0;
  if (split) {
    // the children carry scaling log(exp(s) / (0.8 N)) and the original's opacity; prune_points judges them by their own
    // scaling (both children alike)
    const float c0 = expf(logf(s0 / 1.6f)), c1 = expf(logf(s1 / 1.6f)), c2 = expf(logf(s2 / 1.6f));
    const bool child_big = p.screen_size_term && me_max3(c0, c1, c2) > p.big_scale;
    if (!(low_opacity || child_big)) c |= ME_CHILD;
  } else if (!(low_opacity || big)) {
    c |= ME_KEEP;
    if (clone) c |= ME_CLONE;  // a clone is a raw copy: dropped exactly when its original is
  }
  return c;
}

__global__ __launch_bounds__(ME_ROWS) void map_edit_classify(int P, olsr_map_edit_params p, olsr_map_buffers src,
                                                             const uint8_t* __restrict__ drop_mask, MeScratch sc) {
  const int j = blockIdx.x * ME_ROWS + threadIdx.x;
  uint8_t c = 0;
  if (j < P) {
    if (p.mode == OLSR_MAP_EDIT_DENSIFY) c = me_densify_class(p, src, j);
    else c = (drop_mask && drop_mask[j]) ? 0 : ME_KEEP;
    sc.cls[j] = c;
  }
  const int nk = __syncthreads_count(c & ME_KEEP);
  const int nc = __syncthreads_count(c & ME_CLONE);
  const int ns = __syncthreads_count(c & ME_CHILD);
  if (threadIdx.x == 0) {
    const size_t nb = gridDim.x;
    sc.counts[blockIdx.x] = nk;
    sc.counts[nb + blockIdx.x] = nc;
    sc.counts[2 * nb + blockIdx.x] = ns;
  }
}

// exclusive prefix of the three per-block counts over the blocks, in block order; status = segment totals
__global__ __launch_bounds__(ME_PREFIX_THREADS) void map_edit_prefix(int nb, int n_append, MeScratch sc,
                                                                      int32_t* __restrict__ status) {
  __shared__ int32_t s_w[ME_PREFIX_THREADS / 64];
  int32_t totals[3];
  for (int seg = 0; seg < 3; ++seg)
    totals[seg] = single_block_excl_scan<ME_PREFIX_THREADS / 64>(nb, sc.counts + (size_t)seg * nb,
                                                                 sc.offsets + (size_t)seg * nb, s_w);
  if (threadIdx.x == 0) {
    status[0] = totals[0] + totals[1] + 2 * totals[2] + n_append;
    status[1] = totals[0];
    status[2] = totals[1];
    status[3] = totals[2];
    status[4] = n_append;
    status[5] = status[6] = status[7] = 0;
  }
}

__global__ __launch_bounds__(ME_ROWS) void map_edit_apply(int P, int M, int F, int nb_src, olsr_map_edit_params p,
                                                          olsr_map_buffers src, const float* __restrict__ z,
                                                          olsr_map_buffers app, MeScratch sc,
                                                          const int32_t* __restrict__ status, int dst_capacity,
                                                          olsr_map_buffers dst, int32_t* __restrict__ src_index) {
  __shared__ int32_t dest[4][ME_ROWS];         // destination row per segment (keep, clone, child 0, child 1), -1 = none
  __shared__ float child_xyz[2][3][ME_ROWS];   // split children, [k][axis][row]
  __shared__ float child_scale[3][ME_ROWS];
  __shared__ u32 wave_counts[ME_WAVES];
  const int width = 11 + 3 * M + F, sh_w = 3 * M;
  const int32_t n_keep = status[1], n_clone = status[2], n_child = status[3];
  const bool zero_acc = (p.mode == OLSR_MAP_EDIT_DENSIFY) || p.n_append > 0;
  const int t = threadIdx.x;

  if ((int)blockIdx.x >= nb_src) {
    // ---- appended rows (extend_from_pcd): row k goes to n_keep + k (mask / append mode: no clones, no children) ----
    const int k0 = (blockIdx.x - nb_src) * ME_ROWS;
    const int nk = min(ME_ROWS, p.n_append - k0);
    const int base_dst = n_keep + n_clone + 2 * n_child + k0;
    if (t < nk) {
      const int d = base_dst + t;
      if (d < dst_capacity) {
        src_index[d] = -(k0 + t + 1);
        dst.kf_id[d] = p.append_kf_id;
        dst.n_obs[d] = 0;
        dst.stats[2 * d] = 0.0f;
        dst.stats[2 * d + 1] = 0.0f;
        dst.max_radii[d] = 0;
      }
    }
    const int count = nk * width;
    for (int e = t; e < count; e += ME_ROWS) {
      const int r = e / width, c = e - r * width;
      const size_t k = (size_t)(k0 + r);
      const size_t d = (size_t)(base_dst + r);
      if (d >= (size_t)dst_capacity) continue;
      float v;
      if (c < 3) { v = app.means3D[3 * k + c]; dst.means3D[3 * d + c] = v; }
      else if (c < 3 + sh_w) { v = app.shs[k * sh_w + (c - 3)]; dst.shs[d * sh_w + (c - 3)] = v; }
      else if (c < 4 + sh_w) { v = app.opacities[k]; dst.opacities[d] = v; }
      else if (c < 7 + sh_w) { v = app.scales[3 * k + (c - 4 - sh_w)]; dst.scales[3 * d + (c - 4 - sh_w)] = v; }
      else if (c < 11 + sh_w) { v = app.rotations[4 * k + (c - 7 - sh_w)]; dst.rotations[4 * d + (c - 7 - sh_w)] = v; }
      else dst.language[d * F + (c - 11 - sh_w)] = 0.0f;  // language starts at zero (:300-306)
      dst.exp_avg[d * width + c] = 0.0f;
      dst.exp_avg_sq[d * width + c] = 0.0f;
    }
    return;
  }

  // ---- source rows: ranks inside the block, destinations, split children ----
  const int j0 = blockIdx.x * ME_ROWS;
  const int j = j0 + t;
  const uint8_t c = j < P ? sc.cls[j] : 0;
  const size_t nb = (size_t)nb_src;
  // ranks of this row among the block's rows of each class (wave_counts is reused: a barrier in between)
  const int rk = (int)block_rank<ME_WAVES>(c & ME_KEEP, wave_counts);
  __syncthreads();
  const int rc = (int)block_rank<ME_WAVES>(c & ME_CLONE, wave_counts);
  __syncthreads();
  const int rs = (int)block_rank<ME_WAVES>(c & ME_CHILD, wave_counts);
  dest[0][t] = (c & ME_KEEP) ? sc.offsets[blockIdx.x] + rk : -1;
  dest[1][t] = (c & ME_CLONE) ? n_keep + sc.offsets[nb + blockIdx.x] + rc : -1;
  dest[2][t] = (c & ME_CHILD) ? n_keep + n_clone + sc.offsets[2 * nb + blockIdx.x] + rs : -1;
  dest[3][t] = (c & ME_CHILD) ? n_keep + n_clone + n_child + sc.offsets[2 * nb + blockIdx.x] + rs : -1;
  if (c & ME_CHILD) {
    // build_rotation(r) (general_utils.py:113-135)
    const float r0 = src.rotations[4 * j], r1 = src.rotations[4 * j + 1], r2 = src.rotations[4 * j + 2],
                r3 = src.rotations[4 * j + 3];
    const float norm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const float qr = r0 / norm, x = r1 / norm, y = r2 / norm, zq = r3 / norm;
    float R[3][3];
    R[0][0] = 1.0f - 2.0f * (y * y + zq * zq);
    R[0][1] = 2.0f * (x * y - qr * zq);
    R[0][2] = 2.0f * (x * zq + qr * y);
    R[1][0] = 2.0f * (x * y + qr * zq);
    R[1][1] = 1.0f - 2.0f * (x * x + zq * zq);
    R[1][2] = 2.0f * (y * zq - qr * x);
    R[2][0] = 2.0f * (x * zq - qr * y);
    R[2][1] = 2.0f * (y * zq + qr * x);
    R[2][2] = 1.0f - 2.0f * (x * x + y * y);
    float stdv[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      stdv[a] = expf(src.scales[3 * j + a]);                // get_scaling
      child_scale[a][t] = logf(stdv[a] / 1.6f);             // scaling_inverse_activation(get_scaling / (0.8 * N))
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float smp[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) smp[a] = stdv[a] * z[(size_t)j * 6 + 3 * k + a];  // torch.normal(0, std) = std * z
#pragma unroll
      for (int a = 0; a < 3; ++a)
        child_xyz[k][a][t] = ((R[a][0] * smp[0] + R[a][1] * smp[1]) + R[a][2] * smp[2]) + src.means3D[3 * j + a];
    }
  }
  // per-row integer fields and accumulators
  if (j < P) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int d = dest[s][t];
      if (d < 0 || d >= dst_capacity) continue;
      src_index[d] = j;
      dst.kf_id[d] = src.kf_id[j];
      dst.n_obs[d] = src.n_obs[j];
      dst.stats[2 * d] = zero_acc ? 0.0f : src.stats[2 * j];
      dst.stats[2 * d + 1] = zero_acc ? 0.0f : src.stats[2 * j + 1];
      dst.max_radii[d] = zero_acc ? 0 : src.max_radii[j];
    }
  }
  __syncthreads();

  // ---- every element of the block's rows once: parameters and moments to each destination ----
  const int nrows = min(ME_ROWS, P - j0);
  const int count = nrows * width;
  const size_t base = (size_t)j0 * width;
  for (int e = t; e < count; e += ME_ROWS) {
    const int r = e / width, col = e - r * width;
    const uint8_t rc_ = sc.cls[j0 + r];
    if (!rc_) continue;
    const size_t js = (size_t)(j0 + r);
    float v;
    int kind = 0;  // 0 plain, 1 xyz axis, 2 scale axis
    int axis = 0;
    if (col < 3) { v = src.means3D[3 * js + col]; kind = 1; axis = col; }
    else if (col < 3 + sh_w) v = src.shs[js * sh_w + (col - 3)];
    else if (col < 4 + sh_w) v = src.opacities[js];
    else if (col < 7 + sh_w) { axis = col - 4 - sh_w; v = src.scales[3 * js + axis]; kind = 2; }
    else if (col < 11 + sh_w) v = src.rotations[4 * js + (col - 7 - sh_w)];
    else v = src.language[js * F + (col - 11 - sh_w)];
    const float m = src.exp_avg[base + e], sq = src.exp_avg_sq[base + e];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int d_ = dest[s][r];
      if (d_ < 0 || d_ >= dst_capacity) continue;
      const size_t d = (size_t)d_;
      float w = v;
      if (s >= 2 && kind == 1) w = child_xyz[s - 2][axis][r];
      if (s >= 2 && kind == 2) w = child_scale[axis][r];
      if (col < 3) dst.means3D[3 * d + col] = w;
      else if (col < 3 + sh_w) dst.shs[d * sh_w + (col - 3)] = w;
      else if (col < 4 + sh_w) dst.opacities[d] = w;
      else if (col < 7 + sh_w) dst.scales[3 * d + (col - 4 - sh_w)] = w;
      else if (col < 11 + sh_w) dst.rotations[4 * d + (col - 7 - sh_w)] = w;
      else dst.language[d * F + (col - 11 - sh_w)] = w;
      dst.exp_avg[d * width + col] = s == 0 ? m : 0.0f;     // survivors keep their moments, new rows start at zero
      dst.exp_avg_sq[d * width + col] = s == 0 ? sq : 0.0f;
    }
  }
}

void launch_map_edit_plan(int P, const olsr_map_edit_params& p, const olsr_map_buffers& src, const uint8_t* drop_mask,
                          void* scratch, int32_t* status, hipStream_t st) {
  const int nb = me_blocks(P);
  size_t bytes;
  MeScratch sc = MeScratch::carve(scratch, P, bytes);
  if (nb > 0) map_edit_classify<<<nb, ME_ROWS, 0, st>>>(P, p, src, drop_mask, sc);
  map_edit_prefix<<<1, ME_PREFIX_THREADS, 0, st>>>(nb, p.n_append, sc, status);
}

void launch_map_edit_apply(int P, int M, int F, const olsr_map_edit_params& p, const olsr_map_buffers& src, const float* z,
                           const olsr_map_buffers* append, const void* scratch, const int32_t* status, int dst_capacity,
                           const olsr_map_buffers& dst, int32_t* src_index, hipStream_t st) {
  const int nb = me_blocks(P);
  const int na = p.n_append > 0 ? (p.n_append + ME_ROWS - 1) / ME_ROWS : 0;
  if (nb + na == 0) return;
  size_t bytes;
  MeScratch sc = MeScratch::carve(const_cast<void*>(scratch), P, bytes);
  olsr_map_buffers app{};
  if (append) app = *append;
  map_edit_apply<<<nb + na, ME_ROWS, 0, st>>>(P, M, F, nb, p, src, z, app, sc, status, dst_capacity, dst, src_index);
}

}  // namespace olsr
