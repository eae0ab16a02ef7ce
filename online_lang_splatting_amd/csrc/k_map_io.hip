// k_map_io.hip — the Gaussian map <-> the reference's point_cloud.ply record array (include/olsr_map_io.h), one launch each
// way.  Pure data movement on 32-bit words: no value is ever a float in a register, so every bit pattern survives.
//
// A workgroup takes a block of consecutive rows.  For such a block every array of the map contributes ONE contiguous span
// (rows r0 .. r0 + n of a [P, c] array are the n c words from r0 c), and so does the record array.  A span is walked by
// span_walk: a scalar head up to the first 16-byte boundary, 16-byte accesses over the body, a scalar tail — consecutive lanes
// on consecutive addresses in each part.  The two layouts meet in an LDS image of the RECORD side:
//   pack     the six spans of the map are loaded and scattered into the image (row * width + record column; the f_rest
//            transposition is this index), the three normals are stored as zeros, then the image is copied out as one span;
//   unpack   the file's span is copied into the image, then each of the six spans of the map is stored, every word
//            gathered from image[row * n_cols + col[record column]] (an absent language channel: 0).
// The image starts (address / 4) % 4 words into the LDS array, so that a 16-byte access of the record span is a 16-byte
// access of the image.  64 rows of the widest record (94 words) are 23.5 KiB; a file with more columns gets fewer rows per
// block (6016 / n_cols).  Element offsets are 64-bit before a span starts and below 6016 inside it.  No atomics, no scratch.
#include "olsr_kernels.h"

namespace olsr {

constexpr int MIO_THREADS = 256;
constexpr int MIO_ROWS = OLSR_MAP_PLY_BLOCK_ROWS;
constexpr int MIO_IMAGE_WORDS = OLSR_MAP_PLY_MAX_COLS;   // = MIO_ROWS * OLSR_MAP_PLY_MAX_WIDTH
static_assert(MIO_ROWS * OLSR_MAP_PLY_MAX_WIDTH <= MIO_IMAGE_WORDS, "the widest record's block must fit the image");

struct MioCols {
  int16_t c[OLSR_MAP_PLY_MAX_WIDTH + 2];   // file column per record column (< OLSR_MAP_PLY_MAX_COLS), -1: absent
};

// Walks the `count` words from g: visit(e, p, n) is called once for every piece [e, e + n) of the span, p = g + e, with n = 4
// and p 16-byte aligned over the body, n = 1 over the head and the tail.
template <typename Visit>
__device__ inline void span_walk(uint32_t* g, int count, Visit&& visit) {
  const int t = (int)threadIdx.x;
  int head = (int)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(g) >> 2) & 3u)) & 3u);
  if (head > count) head = count;
  const int body = (count - head) >> 2;
  const int tail0 = head + 4 * body;
  if (t < head) visit(t, g + t, 1);
  for (int q = t; q < body; q += MIO_THREADS) visit(head + 4 * q, g + head + 4 * q, 4);
  if (t < count - tail0) visit(tail0 + t, g + tail0 + t, 1);
}

// Loads the span of a [rows, c] array and hands every word to put(row, k, word), k the word's index in its row.
template <typename Put>
__device__ inline void span_scatter(const uint32_t* g, int c, int count, Put&& put) {
  span_walk(const_cast<uint32_t*>(g), count, [&](int e, uint32_t* p, int n) {
    uint32_t v[4];
    if (n == 4) {
      const uint4 q = *reinterpret_cast<const uint4*>(p);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
      v[0] = *p;
    }
    int row = e / c, k = e - row * c;
    for (int i = 0; i < n; ++i) {
      put(row, k, v[i]);
      if (++k == c) k = 0, ++row;
    }
  });
}

// Stores the span of a [rows, c] array, every word from get(row, k).
template <typename Get>
__device__ inline void span_gather(uint32_t* g, int c, int count, Get&& get) {
  span_walk(g, count, [&](int e, uint32_t* p, int n) {
    uint32_t v[4];
    int row = e / c, k = e - row * c;
    for (int i = 0; i < n; ++i) {
      v[i] = get(row, k);
      if (++k == c) k = 0, ++row;
    }
    if (n == 4)
      *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    else
      *p = v[0];
  });
}

// the record column of word k = 3 m + ch of a row of shs [M, 3]: f_dc_ch, or f_rest_{ch (M - 1) + m - 1}
__device__ inline int mio_sh_column(int k, int M) {
  const int m = k / 3, ch = k - 3 * m;
  return m == 0 ? 6 + ch : 9 + ch * (M - 1) + (m - 1);
}

__device__ inline const uint32_t* mio_words(const float* p, int64_t first) {
  return reinterpret_cast<const uint32_t*>(p) + first;
}
__device__ inline uint32_t* mio_words(float* p, int64_t first) { return reinterpret_cast<uint32_t*>(p) + first; }

__global__ __launch_bounds__(MIO_THREADS) void map_ply_pack_kernel(int P, int M, int F, olsr_map_buffers src,
                                                                   float* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[MIO_IMAGE_WORDS + 4];
  const int width = 14 + 3 * M + F;
  const int64_t r0 = (int64_t)blockIdx.x * MIO_ROWS;
  const int n = (int64_t)P - r0 < MIO_ROWS ? (int)((int64_t)P - r0) : MIO_ROWS;
  uint32_t* out = mio_words(rows, r0 * width);
  uint32_t* image = lds + ((reinterpret_cast<uintptr_t>(out) >> 2) & 3u);
  const int oc = 9 + 3 * (M - 1) + F;   // the opacity's column
  for (int i = (int)threadIdx.x; i < 3 * n; i += MIO_THREADS) image[(i / 3) * width + 3 + i % 3] = 0u;
  span_scatter(mio_words(src.means3D, r0 * 3), 3, 3 * n, [&](int row, int k, uint32_t w) { image[row * width + k] = w; });
  span_scatter(mio_words(src.shs, r0 * 3 * M), 3 * M, 3 * M * n,
               [&](int row, int k, uint32_t w) { image[row * width + mio_sh_column(k, M)] = w; });
  if (F > 0)
    span_scatter(mio_words(src.language, r0 * F), F, F * n,
                 [&](int row, int k, uint32_t w) { image[row * width + 6 + 3 * M + k] = w; });
  span_scatter(mio_words(src.opacities, r0), 1, n, [&](int row, int, uint32_t w) { image[row * width + oc] = w; });
  span_scatter(mio_words(src.scales, r0 * 3), 3, 3 * n, [&](int row, int k, uint32_t w) { image[row * width + oc + 1 + k] = w; });
  span_scatter(mio_words(src.rotations, r0 * 4), 4, 4 * n,
               [&](int row, int k, uint32_t w) { image[row * width + oc + 4 + k] = w; });
  __syncthreads();
  span_walk(out, n * width, [&](int e, uint32_t* p, int cnt) {
    if (cnt == 4)
      *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(image + e);
    else
      *p = image[e];
  });
}

__global__ __launch_bounds__(MIO_THREADS) void map_ply_unpack_kernel(int P, int M, int F, int n_cols, int block_rows,
                                                                     MioCols col, const float* __restrict__ rows,
                                                                     olsr_map_buffers dst) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[MIO_IMAGE_WORDS + 4];
  __shared__ int lcol[OLSR_MAP_PLY_MAX_WIDTH + 2];
  const int width = 14 + 3 * M + F;
  const int64_t r0 = (int64_t)blockIdx.x * block_rows;
  const int n = (int64_t)P - r0 < block_rows ? (int)((int64_t)P - r0) : block_rows;
  const uint32_t* in = mio_words(rows, r0 * n_cols);
  uint32_t* image = lds + ((reinterpret_cast<uintptr_t>(in) >> 2) & 3u);
  if ((int)threadIdx.x < width) lcol[threadIdx.x] = col.c[threadIdx.x];
  span_walk(const_cast<uint32_t*>(in), n * n_cols, [&](int e, uint32_t* p, int cnt) {
    if (cnt == 4)
      *reinterpret_cast<uint4*>(image + e) = *reinterpret_cast<const uint4*>(p);
    else
      image[e] = *p;
  });
  __syncthreads();
  const int oc = 9 + 3 * (M - 1) + F;
  auto field = [&](int row, int j) { return image[row * n_cols + lcol[j]]; };
  span_gather(mio_words(dst.means3D, r0 * 3), 3, 3 * n, [&](int row, int k) { return field(row, k); });
  span_gather(mio_words(dst.shs, r0 * 3 * M), 3 * M, 3 * M * n, [&](int row, int k) { return field(row, mio_sh_column(k, M)); });
  if (F > 0)
    span_gather(mio_words(dst.language, r0 * F), F, F * n, [&](int row, int k) {
      const int fc = lcol[6 + 3 * M + k];
      return fc < 0 ? 0u : image[row * n_cols + fc];
    });
  span_gather(mio_words(dst.opacities, r0), 1, n, [&](int row, int) { return field(row, oc); });
  span_gather(mio_words(dst.scales, r0 * 3), 3, 3 * n, [&](int row, int k) { return field(row, oc + 1 + k); });
  span_gather(mio_words(dst.rotations, r0 * 4), 4, 4 * n, [&](int row, int k) { return field(row, oc + 4 + k); });
}

void launch_map_ply_pack(int P, int M, int F, const olsr_map_buffers& src, float* rows, hipStream_t st) {
  const unsigned blocks = (unsigned)(((int64_t)P + MIO_ROWS - 1) / MIO_ROWS);
  map_ply_pack_kernel<<<blocks, MIO_THREADS, 0, st>>>(P, M, F, src, rows);
}

void launch_map_ply_unpack(int P, int M, int F, int n_cols, const int32_t* col, const float* rows, const olsr_map_buffers& dst,
                           hipStream_t st) {
  MioCols c{};
  const int width = 14 + 3 * M + F;
  for (int j = 0; j < width; ++j) c.c[j] = (int16_t)col[j];
  int block_rows = MIO_IMAGE_WORDS / n_cols;
  if (block_rows > MIO_ROWS) block_rows = MIO_ROWS;
  const unsigned blocks = (unsigned)(((int64_t)P + block_rows - 1) / block_rows);
  map_ply_unpack_kernel<<<blocks, MIO_THREADS, 0, st>>>(P, M, F, n_cols, block_rows, c, rows, dst);
}

}  // namespace olsr
