// k_tsdf.hip — TSDF fusion of depth and feature images into a voxel volume, its surface point cloud and mesh (include/olsr.h,
// "TSDF fusion").
//
// The reference (tsdf-fusion/fusion.py, fusion2.py, fusion3.py) launches one `integrate` kernel per frame after uploading the
// depth image and up to 15 feature images from the host, keeps 15 separate feature volumes, and extracts the surface on the
// host.  Here
//
//   tsdf_integrate<F, PACKED>  one launch for up to OLSR_TSDF_MAX_VIEWS views.  A thread owns a voxel (z fastest: consecutive
//                              lanes are consecutive addresses of every plane of the volume), walks the views in index order
//                              and keeps tsdf, weight and the F feature means in registers from the first view that reaches
//                              the voxel to one store at the end.  The views (intrinsics, pose, image pointers) are kernel
//                              arguments: scalar loads, no device-side table.
//   tsdf_surface_count / tsdf_surface_prefix / tsdf_surface_emit
//                              count the zero crossings each voxel owns, prefix the block counts in block order, write the
//                              points: the pattern of k_map_edit.hip, no atomics, output in voxel order then axis.
//   tsdf_mesh_count / tsdf_mesh_prefix / tsdf_mesh_emit
//                              the same vertices with their normals and the triangles between them, from the generated table of
//                              olsr_mc_table.h: the same pattern, one 32-bit word per voxel between the passes.
//
// Per voxel and view the float32 expressions are the reference kernel's, in its order (fusion.py:93-139, fusion3.py:181-290);
// the translation unit is compiled without FMA contraction (build.py) and float division is correctly rounded, so the volume
// equals a float32 restatement of those statements (tests/tsdf_ref.py) bit for bit.  Divergences from the reference kernel,
// each on purpose (include/olsr.h lists them for callers):
//   - voxel coordinates come from integer division of the linear index (the reference divides (float)voxel_idx: wrong above
//     2^24 voxels);
//   - the bound is idx < N (the reference tests voxel_idx > N);
//   - !(cam_z > 0) skips the voxel (the reference kernel skips cam_z < 0 only and converts the pixel coordinate of a voxel in
//     the camera plane, an infinity or a NaN, to int; its CPU path tests pix_z > 0);
//   - the rounded pixel coordinate is compared with the image size as a float, then converted;
//   - rounding is roundf, half away from zero, as in the reference kernel (its CPU path: np.round, half to even);
//   - an optional opacity plane masks pixels no Gaussian covers.
//
// HBM-bound.  Per batch the volume traffic is one read and one write of (2 + F) floats per touched voxel, whatever the number
// of views; the image gathers of neighbouring voxels fall on neighbouring pixels and are served by the caches.
#include "olsr_device.h"
#include "olsr_kernels.h"
#include "olsr_mc_table.h"

namespace olsr {

constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_MAX_BLOCKS = 256 * 8;  // integrate and init walk the volume with a grid stride beyond this
constexpr int TS_PREFIX_THREADS = 1024;

struct TsdfViews {
  olsr_tsdf_view v[OLSR_TSDF_MAX_VIEWS];
};

__global__ __launch_bounds__(TS_THREADS) void tsdf_init(olsr_tsdf_volume vol, int planes) {
  const size_t N = (size_t)vol.X * vol.Y * vol.Z;
  for (size_t i = (size_t)blockIdx.x * TS_THREADS + threadIdx.x; i < N; i += (size_t)gridDim.x * TS_THREADS) {
    vol.tsdf[i] = 1.0f;
    vol.weight[i] = 0.0f;
    for (int c = 0; c < planes; ++c) vol.feat[(size_t)c * N + i] = 0.0f;
  }
}

template <int F, bool PACKED>
__global__ __launch_bounds__(TS_THREADS) void tsdf_integrate(olsr_tsdf_volume vol, int n_views, TsdfViews vs) {
  constexpr int PLANES = PACKED ? 1 : F;
  const size_t N = (size_t)vol.X * vol.Y * vol.Z;
  const int YZ = vol.Y * vol.Z;
  for (size_t idx = (size_t)blockIdx.x * TS_THREADS + threadIdx.x; idx < N; idx += (size_t)gridDim.x * TS_THREADS) {
    const int i = (int)idx;
    const int x = i / YZ, rem = i - x * YZ;
    const int y = rem / vol.Z, z = rem - y * vol.Z;
    // voxel grid coordinates to world coordinates
    const float pt_x = vol.origin[0] + (float)x * vol.voxel_size;
    const float pt_y = vol.origin[1] + (float)y * vol.voxel_size;
    const float pt_z = vol.origin[2] + (float)z * vol.voxel_size;
    bool loaded = false;
    float tsdf = 0.0f, w = 0.0f;
    float feat[PLANES > 0 ? PLANES : 1];
    for (int v = 0; v < n_views; ++v) {
      const olsr_tsdf_view& c = vs.v[v];
      // world coordinates to camera coordinates
      const float tmp_x = pt_x - c.pose[0 * 4 + 3];
      const float tmp_y = pt_y - c.pose[1 * 4 + 3];
      const float tmp_z = pt_z - c.pose[2 * 4 + 3];
      const float cam_x = c.pose[0 * 4 + 0] * tmp_x + c.pose[1 * 4 + 0] * tmp_y + c.pose[2 * 4 + 0] * tmp_z;
      const float cam_y = c.pose[0 * 4 + 1] * tmp_x + c.pose[1 * 4 + 1] * tmp_y + c.pose[2 * 4 + 1] * tmp_z;
      const float cam_z = c.pose[0 * 4 + 2] * tmp_x + c.pose[1 * 4 + 2] * tmp_y + c.pose[2 * 4 + 2] * tmp_z;
      if (!(cam_z > 0.0f)) continue;
      // camera coordinates to image pixels
      const float px = roundf(c.fx * (cam_x / cam_z) + c.cx);
      const float py = roundf(c.fy * (cam_y / cam_z) + c.cy);
      if (!(px >= 0.0f && px < (float)c.W && py >= 0.0f && py < (float)c.H)) continue;  // (a NaN fails every comparison)
      const int pix = (int)py * c.W + (int)px;
      const float depth_value = c.depth[pix];
      if (depth_value == 0.0f) continue;
      if (c.opacity && c.opacity[pix] < c.min_opacity) continue;
      const float depth_diff = depth_value - cam_z;
      if (depth_diff < -vol.trunc_margin) continue;
      const float dist = fminf(1.0f, depth_diff / vol.trunc_margin);
      if (!loaded) {
        loaded = true;
        tsdf = vol.tsdf[idx];
        w = vol.weight[idx];
#pragma unroll
        for (int k = 0; k < PLANES; ++k) feat[k] = vol.feat[(size_t)k * N + idx];
      }
      const float w_old = w, obs_weight = c.obs_weight;
      const float w_new = w_old + obs_weight;
      w = w_new;
      tsdf = (tsdf * w_old + obs_weight * dist) / w_new;
      if constexpr (PACKED) {
        const float old_color = feat[0];
        const float old_b = floorf(old_color / 65536.0f);
        const float old_g = floorf((old_color - old_b * 65536.0f) / 256.0f);
        const float old_r = old_color - old_b * 65536.0f - old_g * 256.0f;
        const float new_color = c.feat[pix];
        float new_b = floorf(new_color / 65536.0f);
        float new_g = floorf((new_color - new_b * 65536.0f) / 256.0f);
        float new_r = new_color - new_b * 65536.0f - new_g * 256.0f;
        new_b = fminf(roundf((old_b * w_old + obs_weight * new_b) / w_new), 255.0f);
        new_g = fminf(roundf((old_g * w_old + obs_weight * new_g) / w_new), 255.0f);
        new_r = fminf(roundf((old_r * w_old + obs_weight * new_r) / w_new), 255.0f);
        feat[0] = new_b * 65536.0f + new_g * 256.0f + new_r;
      } else if constexpr (F > 0) {
        const bool rows = c.feat_layout == OLSR_TSDF_IMAGE_ROWS;
        const size_t base = rows ? (size_t)pix * F : (size_t)pix;
        const size_t step = rows ? (size_t)1 : (size_t)c.H * c.W;
#pragma unroll
        for (int k = 0; k < F; ++k) feat[k] = (feat[k] * w_old + obs_weight * c.feat[base + k * step]) / w_new;
      }
    }
    if (loaded) {
      vol.tsdf[idx] = tsdf;
      vol.weight[idx] = w;
#pragma unroll
      for (int k = 0; k < PLANES; ++k) vol.feat[(size_t)k * N + idx] = feat[k];
    }
  }
}

// ---- the surface point cloud -----------------------------------------------------------------------------------------------
__host__ __device__ inline size_t ts_blocks(size_t N) { return (N + TS_THREADS - 1) / TS_THREADS; }
static size_t ts_voxels(int X, int Y, int Z) { return (size_t)(X > 0 ? X : 0) * (size_t)(Y > 0 ? Y : 0) * (size_t)(Z > 0 ? Z : 0); }

struct TsSurfaceScratch {
  int32_t *counts, *offsets;  // [nb] each, nb = blocks of TS_THREADS voxels
  static TsSurfaceScratch carve(void* buf, size_t N, size_t& bytes) {
    Carver c(buf);
    TsSurfaceScratch s;
    s.counts = c.take<int32_t>(ts_blocks(N));
    s.offsets = c.take<int32_t>(ts_blocks(N));
    bytes = c.total();
    return s;
  }
};

size_t tsdf_surface_scratch_bytes(int X, int Y, int Z) {
  size_t bytes = 0;
  TsSurfaceScratch::carve(nullptr, ts_voxels(X, Y, Z), bytes);
  return bytes;
}

// bit a of the result: the edge from voxel i = (x, y, z) along axis a (0 x, 1 y, 2 z) is owned by it and crosses zero
__device__ inline int ts_crossings(const olsr_tsdf_volume& vol, float min_weight, int i, int x, int y, int z, float t0) {
  const int YZ = vol.Y * vol.Z;
  const bool use_w = min_weight > 0.0f;
  if (use_w && !(vol.weight[i] >= min_weight)) return 0;
  const bool neg0 = t0 < 0.0f;
  int bits = 0;
  const int stride[3] = {YZ, vol.Z, 1};
  const bool inside[3] = {x + 1 < vol.X, y + 1 < vol.Y, z + 1 < vol.Z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!inside[a]) continue;
    const int j = i + stride[a];
    if ((vol.tsdf[j] < 0.0f) != neg0 && (!use_w || vol.weight[j] >= min_weight)) bits |= 1 << a;
  }
  return bits;
}

// vertex k: the zero crossing of the edge from voxel i = (x, y, z) along axis a (its other end: i + stride); t0 = tsdf[i]
__device__ __forceinline__ void ts_write_vertex(const olsr_tsdf_volume& vol, int N, int i, int a, int stride, int x, int y, int z, float t0,
                                       int k, float* __restrict__ points, float* __restrict__ feats,
                                       int32_t* __restrict__ voxel_index) {
  const int planes = vol.feat_mode == OLSR_TSDF_FEAT_PACKED_RGB ? 3 : vol.F;
  const float t1 = vol.tsdf[i + stride];
  const float v[3] = {(float)x, (float)y, (float)z};
  float pos[3] = {v[0], v[1], v[2]};
  pos[a] = v[a] + t0 / (t0 - t1);
  // the voxel the reference reads the vertex's colour from: np.round(verts).astype(int) — the owner or its neighbour
  // (a NaN position, from a NaN or infinite distance, stays with the owner)
  const int nearest = rintf(pos[a]) == v[a] + 1.0f ? i + stride : i;
#pragma unroll
  for (int d = 0; d < 3; ++d) points[(size_t)3 * k + d] = pos[d] * vol.voxel_size + vol.origin[d];
  if (voxel_index) voxel_index[k] = i;
  if (feats) {
    if (vol.feat_mode == OLSR_TSDF_FEAT_PACKED_RGB) {
      const float rgb_val = vol.feat[nearest];
      const float b = floorf(rgb_val / 65536.0f);
      const float g = floorf((rgb_val - b * 65536.0f) / 256.0f);
      const float r = rgb_val - b * 65536.0f - g * 256.0f;
      feats[(size_t)3 * k] = r;
      feats[(size_t)3 * k + 1] = g;
      feats[(size_t)3 * k + 2] = b;
    } else {
      for (int c = 0; c < planes; ++c) feats[(size_t)planes * k + c] = vol.feat[(size_t)c * N + nearest];
    }
  }
}

template <bool EMIT>
__global__ __launch_bounds__(TS_THREADS) void tsdf_surface(olsr_tsdf_volume vol, float min_weight, int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ offsets, int capacity,
                                                           float* __restrict__ points, float* __restrict__ feats,
                                                           int32_t* __restrict__ voxel_index) {
  __shared__ int32_t wave_sums[TS_WAVES];
  const int N = vol.X * vol.Y * vol.Z;
  const int YZ = vol.Y * vol.Z;
  const int i = blockIdx.x * TS_THREADS + threadIdx.x;
  int x = 0, y = 0, z = 0, bits = 0;
  float t0 = 0.0f;
  if (i < N) {
    x = i / YZ;
    const int rem = i - x * YZ;
    y = rem / vol.Z;
    z = rem - y * vol.Z;
    t0 = vol.tsdf[i];
    bits = ts_crossings(vol, min_weight, i, x, y, z, t0);
  }
  int32_t total;
  const int rank = block_excl_scan<TS_WAVES>((int32_t)__popc(bits), wave_sums, &total);
  if constexpr (!EMIT) {
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
    return;
  } else {
    if (!bits) return;
    int k = offsets[blockIdx.x] + rank;
    const int stride[3] = {YZ, vol.Z, 1};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(bits & (1 << a))) continue;
      if (k >= capacity) return;
      ts_write_vertex(vol, N, i, a, stride[a], x, y, z, t0, k, points, feats, voxel_index);
      ++k;
    }
  }
}

// exclusive prefix of the block counts in block order; status = {N, 0}
__global__ __launch_bounds__(TS_PREFIX_THREADS) void tsdf_surface_prefix(int nb, const int32_t* __restrict__ counts,
                                                                          int32_t* __restrict__ offsets,
                                                                          int32_t* __restrict__ status) {
  __shared__ int32_t s_w[TS_PREFIX_THREADS / 64];
  const int32_t total = single_block_excl_scan<TS_PREFIX_THREADS / 64>(nb, counts, offsets, s_w);
  if (threadIdx.x == 0) {
    status[0] = total;
    status[1] = 0;
  }
}

// ---- the mesh: the same vertices, their normals, and the triangles between them ------------------------------------------------
// One thread per voxel, as above.  A voxel owns up to three vertices (ts_crossings' rule) and, when x + 1 < X, y + 1 < Y and
// z + 1 < Z, the cube whose lowest corner it is.  The count pass leaves one word per voxel,
//   bits 0-9 the rank of its first vertex within its block (< 3 * 256), 10-12 its crossing bits,
//   13-23 the rank of its cube's first face within the block (<= 5 * 256), 24-31 the cube's sign configuration (0: no faces),
// and the per-block totals; after the prefix a vertex's id is offsets[block] + rank + popc(crossing bits below its axis), for
// the voxel's own edges and for the neighbours' edges a cube's faces name alike.  The emit pass reads that word first: a voxel
// away from the surface costs it 4 bytes.  The triangle table (olsr_mc_table.h, 2 KiB) is copied to LDS by every workgroup:
// each lane indexes it with its own configuration, which through the scalar constant path would be one load per lane.
static_assert(TS_THREADS == 256, "the table copy and the word's rank fields assume 256 voxels per block");

struct TsMeshScratch {
  u32 *vcounts, *voffsets, *fcounts, *foffsets;  // [nb] each: vertices and faces per block, and their prefixes
  u32* words;                                    // [X * Y * Z] the voxel words
  static TsMeshScratch carve(void* buf, size_t N, size_t& bytes) {
    Carver c(buf);
    TsMeshScratch s;
    s.vcounts = c.take<u32>(ts_blocks(N));
    s.voffsets = c.take<u32>(ts_blocks(N));
    s.fcounts = c.take<u32>(ts_blocks(N));
    s.foffsets = c.take<u32>(ts_blocks(N));
    s.words = c.take<u32>(N);
    bytes = c.total();
    return s;
  }
};

size_t tsdf_mesh_scratch_bytes(int X, int Y, int Z) {
  size_t bytes = 0;
  TsMeshScratch::carve(nullptr, ts_voxels(X, Y, Z), bytes);
  return bytes;
}

// bits: ts_crossings' result for voxel i; config: bit c set when corner c = (c & 1, c >> 1 & 1, c >> 2 & 1) of the cube the
// voxel owns is negative, 0 when it owns none or (min_weight > 0) a corner has less than that weight.  A NaN is not negative.
__device__ inline void ts_mesh_voxel(const olsr_tsdf_volume& vol, float min_weight, int i, int x, int y, int z, int* bits,
                                     int* config) {
  const int YZ = vol.Y * vol.Z;
  const bool use_w = min_weight > 0.0f;
  const bool inside[3] = {x + 1 < vol.X, y + 1 < vol.Y, z + 1 < vol.Z};
  int neg = 0, seen = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    if ((dx && !inside[0]) || (dy && !inside[1]) || (dz && !inside[2])) continue;
    const int j = i + dx * YZ + dy * vol.Z + dz;
    if (vol.tsdf[j] < 0.0f) neg |= 1 << c;
    if (!use_w || vol.weight[j] >= min_weight) seen |= 1 << c;
  }
  int b = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int c = 1 << a;  // the corner one step along axis a
    if (inside[a] && (seen & 1) && (seen & (1 << c)) && ((neg >> c) & 1) != (neg & 1)) b |= 1 << a;
  }
  *bits = b;
  *config = (inside[0] && inside[1] && inside[2] && seen == 0xff) ? neg : 0;
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_mesh_count(olsr_tsdf_volume vol, float min_weight, u32* __restrict__ vcounts,
                                                              u32* __restrict__ fcounts, u32* __restrict__ words) {
  __shared__ u32 wave_sums[TS_WAVES];
  __shared__ u64 table[256];
  table[threadIdx.x] = MC_TABLE[threadIdx.x];
  const int N = vol.X * vol.Y * vol.Z;
  const int YZ = vol.Y * vol.Z;
  const int i = blockIdx.x * TS_THREADS + threadIdx.x;
  int bits = 0, config = 0;
  if (i < N) {
    const int x = i / YZ, rem = i - x * YZ;
    const int y = rem / vol.Z, z = rem - y * vol.Z;
    ts_mesh_voxel(vol, min_weight, i, x, y, z, &bits, &config);
  }
  __syncthreads();
  const u32 n_faces = (u32)(table[config] & 15u);
  if (!n_faces) config = 0;
  // one scan for both counts: the vertices in the low half (<= 768 per block), the faces in the high half (<= 1280)
  u32 total;
  const u32 rank = block_excl_scan<TS_WAVES>((u32)__popc(bits) | n_faces << 16, wave_sums, &total);
  if (i < N) words[i] = (rank & 0xffffu) | (u32)bits << 10 | (rank >> 16) << 13 | (u32)config << 24;
  if (threadIdx.x == 0) {
    vcounts[blockIdx.x] = total & 0xffffu;
    fcounts[blockIdx.x] = total >> 16;
  }
}

// exclusive prefixes of the vertex and the face counts in block order; status = {vertices, faces, 0, 0}.  The faces are summed
// without sign (up to 5 per voxel: beyond 2^31 in the largest volumes) and reported clamped; the emit entry refuses a
// face_capacity whose 3-fold does not fit an int32.
__global__ __launch_bounds__(TS_PREFIX_THREADS) void tsdf_mesh_prefix(int nb, const u32* __restrict__ vcounts,
                                                                       u32* __restrict__ voffsets,
                                                                       const u32* __restrict__ fcounts,
                                                                       u32* __restrict__ foffsets,
                                                                       int32_t* __restrict__ status) {
  __shared__ u32 s_w[TS_PREFIX_THREADS / 64];
  const u32 n_verts = single_block_excl_scan<TS_PREFIX_THREADS / 64>(nb, vcounts, voffsets, s_w);
  const u32 n_faces = single_block_excl_scan<TS_PREFIX_THREADS / 64>(nb, fcounts, foffsets, s_w);
  if (threadIdx.x == 0) {
    status[0] = (int32_t)n_verts;
    status[1] = (int32_t)(n_faces < 0x7fffffffu ? n_faces : 0x7fffffffu);
    status[2] = 0;
    status[3] = 0;
  }
}

// d tsdf / d axis at voxel j, whose coordinate along that axis is c of n: central, one-sided on the border
__device__ __forceinline__ float ts_gradient(const float* __restrict__ t, int j, int c, int n, int stride) {
  if (n < 2) return 0.0f;
  if (c == 0) return t[j + stride] - t[j];
  if (c == n - 1) return t[j] - t[j - stride];
  return 0.5f * (t[j + stride] - t[j - stride]);
}

__global__ __launch_bounds__(TS_THREADS) void tsdf_mesh_emit(olsr_tsdf_volume vol, const u32* __restrict__ voffsets,
                                                             const u32* __restrict__ foffsets,
                                                             const u32* __restrict__ words, int vert_capacity, int face_capacity, float* __restrict__ points,
                                                             float* __restrict__ normals, float* __restrict__ feats,
                                                             int32_t* __restrict__ voxel_index, int32_t* __restrict__ faces) {
  __shared__ u64 table[256];
  table[threadIdx.x] = MC_TABLE[threadIdx.x];
  __syncthreads();
  const int N = vol.X * vol.Y * vol.Z;
  const int YZ = vol.Y * vol.Z;
  const int i = blockIdx.x * TS_THREADS + threadIdx.x;
  if (i >= N) return;
  const u32 word = words[i];
  const int bits = (word >> 10) & 7, config = word >> 24;
  if (!bits && !config) return;
  const int stride[3] = {YZ, vol.Z, 1};
  if (bits) {
    const int x = i / YZ, rem = i - x * YZ;
    const int y = rem / vol.Z, z = rem - y * vol.Z;
    const int coord[3] = {x, y, z}, dim[3] = {vol.X, vol.Y, vol.Z};
    const float t0 = vol.tsdf[i];
    float g0[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) g0[d] = ts_gradient(vol.tsdf, i, coord[d], dim[d], stride[d]);
    int k = (int)(voffsets[blockIdx.x] + (word & 1023u));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!(bits & (1 << a))) continue;
      if (k >= vert_capacity) break;
      ts_write_vertex(vol, N, i, a, stride[a], x, y, z, t0, k, points, feats, voxel_index);
      // the normal: the two voxels' gradients, interpolated with the vertex's own mu, over their length
      const int j = i + stride[a];
      const float mu = t0 / (t0 - vol.tsdf[j]);
      float n[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float g1 = ts_gradient(vol.tsdf, j, coord[d] + (d == a ? 1 : 0), dim[d], stride[d]);
        n[d] = g0[d] + (g1 - g0[d]) * mu;
      }
      const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
      for (int d = 0; d < 3; ++d) normals[(size_t)3 * k + d] = len == 0.0f ? 0.0f : n[d] / len;
      ++k;
    }
  }
  if (config) {
    const u64 entry = table[config];
    const u32 n_faces = (u32)(entry & 15u);
    const u32 f0 = foffsets[blockIdx.x] + ((word >> 13) & 2047u);
    for (u32 t = 0; t < n_faces; ++t) {
      const u32 f = f0 + t;
      if (f >= (u32)face_capacity) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        // edge 4 * axis + k: owned by the corner whose two other coordinates, in ascending axis order, are (k & 1, k >> 1)
        const int e = (int)(entry >> (4 + 4 * (3 * t + c))) & 15;
        const int axis = e >> 2, lo = e & 1, hi = (e >> 1) & 1;
        const int owner = i + lo * (axis == 0 ? vol.Z : YZ) + hi * (axis == 2 ? vol.Z : 1);
        const u32 w = words[owner];
        faces[(size_t)3 * f + c] = (int32_t)(voffsets[owner / TS_THREADS] + (w & 1023u) + __popc((w >> 10) & ((1u << axis) - 1u)));
      }
    }
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static int ts_grid(size_t N) {
  const size_t nb = ts_blocks(N);
  return (int)(nb < (size_t)TS_MAX_BLOCKS ? nb : (size_t)TS_MAX_BLOCKS);
}

void launch_tsdf_init(const olsr_tsdf_volume& vol, hipStream_t st) {
  const size_t N = (size_t)vol.X * vol.Y * vol.Z;
  const int planes = vol.feat_mode == OLSR_TSDF_FEAT_PACKED_RGB ? 1 : vol.F;
  tsdf_init<<<ts_grid(N), TS_THREADS, 0, st>>>(vol, planes);
}

void launch_tsdf_integrate(const olsr_tsdf_volume& vol, int n_views, const olsr_tsdf_view* views, hipStream_t st) {
  TsdfViews vs{};
  for (int v = 0; v < n_views; ++v) vs.v[v] = views[v];
  const size_t N = (size_t)vol.X * vol.Y * vol.Z;
  const int grid = ts_grid(N);
#define OLSR_TSDF_LAUNCH(F_, PACKED_) tsdf_integrate<F_, PACKED_><<<grid, TS_THREADS, 0, st>>>(vol, n_views, vs)
  if (vol.feat_mode == OLSR_TSDF_FEAT_PACKED_RGB) OLSR_TSDF_LAUNCH(1, true);
  else if (vol.F == 0) OLSR_TSDF_LAUNCH(0, false);
  else if (vol.F == 3) OLSR_TSDF_LAUNCH(3, false);
  else if (vol.F == 15) OLSR_TSDF_LAUNCH(15, false);
  else if (vol.F == 16) OLSR_TSDF_LAUNCH(16, false);
  else OLSR_TSDF_LAUNCH(32, false);
#undef OLSR_TSDF_LAUNCH
}

void launch_tsdf_surface_plan(const olsr_tsdf_volume& vol, float min_weight, void* scratch, int32_t* status, hipStream_t st) {
  const size_t N = (size_t)vol.X * vol.Y * vol.Z;
  const int nb = (int)ts_blocks(N);
  size_t bytes;
  const TsSurfaceScratch sc = TsSurfaceScratch::carve(scratch, N, bytes);
  tsdf_surface<false><<<nb, TS_THREADS, 0, st>>>(vol, min_weight, sc.counts, nullptr, 0, nullptr, nullptr, nullptr);
  tsdf_surface_prefix<<<1, TS_PREFIX_THREADS, 0, st>>>(nb, sc.counts, sc.offsets, status);
}

void launch_tsdf_surface_emit(const olsr_tsdf_volume& vol, float min_weight, const void* scratch, int capacity, float* points,
                              float* feats, int32_t* voxel_index, hipStream_t st) {
  const size_t N = (size_t)vol.X * vol.Y * vol.Z;
  const int nb = (int)ts_blocks(N);
  size_t bytes;
  const TsSurfaceScratch sc = TsSurfaceScratch::carve(const_cast<void*>(scratch), N, bytes);
  tsdf_surface<true><<<nb, TS_THREADS, 0, st>>>(vol, min_weight, nullptr, sc.offsets, capacity, points, feats, voxel_index);
}

void launch_tsdf_mesh_plan(const olsr_tsdf_volume& vol, float min_weight, void* scratch, int32_t* status, hipStream_t st) {
  const size_t N = (size_t)vol.X * vol.Y * vol.Z;
  const int nb = (int)ts_blocks(N);
  size_t bytes;
  const TsMeshScratch sc = TsMeshScratch::carve(scratch, N, bytes);
  tsdf_mesh_count<<<nb, TS_THREADS, 0, st>>>(vol, min_weight, sc.vcounts, sc.fcounts, sc.words);
  tsdf_mesh_prefix<<<1, TS_PREFIX_THREADS, 0, st>>>(nb, sc.vcounts, sc.voffsets, sc.fcounts, sc.foffsets, status);
}

void launch_tsdf_mesh_emit(const olsr_tsdf_volume& vol, const void* scratch, int vert_capacity, int face_capacity, float* points,
                           float* normals, float* feats, int32_t* voxel_index, int32_t* faces, hipStream_t st) {
  const size_t N = (size_t)vol.X * vol.Y * vol.Z;
  size_t bytes;
  const TsMeshScratch sc = TsMeshScratch::carve(const_cast<void*>(scratch), N, bytes);
  tsdf_mesh_emit<<<(int)ts_blocks(N), TS_THREADS, 0, st>>>(vol, sc.voffsets, sc.foffsets, sc.words, vert_capacity, face_capacity,
                                                           points, normals, feats, voxel_index, faces);
}

}  // namespace olsr
