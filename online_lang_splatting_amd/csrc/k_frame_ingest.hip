// k_frame_ingest.hip — a frame's ingest (include/olsr_frame_ingest.h): uint8 [H,W,3] + uint16 / float32 depth [H,W] ->
// float32 image [3,H,W] and float32 depth [H,W], the statements of the reference's datasets (utils/dataset.py:316-350) in one
// launch.
//
// The planes of the image and the depth are contiguous over the N = W H pixels, so the kernel works on the flat pixel index
// and knows no rows: a lane takes the four pixels 4 q .. 4 q + 3 (the last lane of the frame fewer), i.e. 12 consecutive
// bytes of the pixel stream, 4 depth elements, and writes 4 consecutive floats per plane.
//   bytes in   the 12 bytes start at any address.  They are fetched as the three or four ALIGNED 32-bit words that hold them
//              and lined up with v_alignbyte — when those words lie inside rgb[0, 3 N); the lanes at the two ends of the
//              stream, whose words would stick out, read their bytes one by one.  Nothing outside the stream is read.
//   colour     byte -> float through a 256-entry LDS table that every workgroup fills with the pinned expression
//              (float) min(max((double) b / 255.0, 0.0), 1.0): the double division runs 256 times per workgroup, not 3 N times.
//   depth      (float) ((double) d / depth_scale), an IEEE double division per pixel.
//   floats out one 16-byte store per plane when the address is 16-byte aligned and the lane has four pixels, else 4-byte stores.
// Memory-bound: 3 N + 2 N (or 4 N) bytes in, 16 N bytes out; a grid-stride loop over at most 2048 workgroups.  No atomics, no
// scratch: the same bits every run.
#include "olsr_kernels.h"

namespace olsr {

constexpr int INGEST_THREADS = 256;
constexpr int INGEST_MAX_BLOCKS = 2048;

__device__ inline void ingest_store4(float* dst, const float v[4], int n) {
  if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < n; ++k) dst[k] = v[k];
  }
}

template <typename D>
__global__ __launch_bounds__(INGEST_THREADS) void frame_ingest_kernel(int64_t N, int64_t plane_stride, double depth_scale,
                                                                      const uint8_t* __restrict__ rgb,
                                                                      const D* __restrict__ depth, float* __restrict__ image,
                                                                      float* __restrict__ depth_out) {
  __shared__ float colour[256];
  {
    const double q = (double)threadIdx.x / 255.0;
    colour[threadIdx.x] = (float)fmin(fmax(q, 0.0), 1.0);
  }
  __syncthreads();
  const uintptr_t begin = reinterpret_cast<uintptr_t>(rgb), end = begin + 3u * (uintptr_t)N;
  const int64_t quads = (N + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * INGEST_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * INGEST_THREADS) {
    const int64_t i0 = 4 * q;
    const int n = (N - i0) < 4 ? (int)(N - i0) : 4;
    // ---- the 12 bytes of the lane's pixels as three words u[0..2], byte j of the lane in u[j / 4] bits 8 (j % 4) ..
    uint32_t u[3] = {0u, 0u, 0u};
    const uintptr_t a = begin + 3u * (uintptr_t)i0;
    const uint32_t sh = (uint32_t)(a & 3u);
    const uintptr_t lo = a - sh;
    const uintptr_t need = sh ? 16u : 12u;
    if (lo >= begin && lo + need <= end) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(lo);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = sh ? w[3] : 0u;
      u[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
      u[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
      u[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
    } else {
      const uint8_t* b = rgb + 3 * i0;
#pragma unroll
      for (int j = 0; j < 12; ++j)
        if (j < 3 * n) u[j >> 2] |= (uint32_t)b[j] << (8 * (j & 3));
    }
    float r[4], g[4], bl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = 3 * k;
      r[k] = colour[(u[j >> 2] >> (8 * (j & 3))) & 255u];
      g[k] = colour[(u[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255u];
      bl[k] = colour[(u[(j + 2) >> 2] >> (8 * ((j + 2) & 3))) & 255u];
    }
    ingest_store4(image + i0, r, n);
    ingest_store4(image + plane_stride + i0, g, n);
    ingest_store4(image + 2 * plane_stride + i0, bl, n);
    // ---- depth
    D d[4] = {};
    const D* dp = depth + i0;
    if (n == 4 && (reinterpret_cast<uintptr_t>(dp) & (4 * sizeof(D) - 1)) == 0) {
      struct alignas(4 * sizeof(D)) Four { D v[4]; };
      const Four f = *reinterpret_cast<const Four*>(dp);
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] = f.v[k];
    } else {
      for (int k = 0; k < n; ++k) d[k] = dp[k];
    }
    float z[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) z[k] = (float)((double)d[k] / depth_scale);
    ingest_store4(depth_out + i0, z, n);
  }
}

void launch_frame_ingest(const olsr_frame_ingest_params& p, const uint8_t* rgb, const void* depth, float* image,
                         float* depth_out, hipStream_t st) {
  const int64_t N = (int64_t)p.W * (int64_t)p.H;
  const int64_t quads = (N + 3) / 4;
  int64_t blocks = (quads + INGEST_THREADS - 1) / INGEST_THREADS;
  if (blocks > INGEST_MAX_BLOCKS) blocks = INGEST_MAX_BLOCKS;
  if (p.depth_type == OLSR_INGEST_DEPTH_U16)
    frame_ingest_kernel<uint16_t><<<(unsigned)blocks, INGEST_THREADS, 0, st>>>(N, p.plane_stride, p.depth_scale, rgb,
                                                                               (const uint16_t*)depth, image, depth_out);
  else
    frame_ingest_kernel<float><<<(unsigned)blocks, INGEST_THREADS, 0, st>>>(N, p.plane_stride, p.depth_scale, rgb,
                                                                            (const float*)depth, image, depth_out);
}

}  // namespace olsr
