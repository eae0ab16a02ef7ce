// cuda_runtime.h of oracle/ref_shim — an execution model for CUDA kernels on the host.  TEST INFRASTRUCTURE ONLY.
//
// The reference rasteriser's kernel sources include <cuda_runtime.h>, <cooperative_groups.h>, <cub/cub.cuh> and their
// kin.  This directory answers those includes with plain C++17, so that the kernel bodies compile as they stand with g++
// and run deterministically on a CPU (oracle/ref_build.py is the recipe; nothing of the reference is kept here).
//
// The model (ref_exec.cpp):
//   * a launch runs its blocks one after another in ascending linear block index (x fastest, then y, then z);
//   * the threads of a block are fibers on one OS thread; they really meet at every sync(): a thread that reaches a
//     barrier is suspended until every live thread of its block has reached it, in ascending thread rank;
//   * `__shared__` is block-wide storage (one object for all fibers; blocks never overlap in time);
//   * atomicAdd is a plain read-modify-write (nothing runs concurrently);
//   * the float overloads of the math functions that CUDA puts into the global namespace are supplied here, and
//     `exp(float)` is the project's pinned routine (../pinned_exp.h; -DREF_LIBM_EXP: the host libm instead).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <utility>

// libstdc++'s <math.h> wrapper pulls every std:: overload into the global namespace with using-declarations; a global
// `float exp(float)` of our own (below) would then collide with std::exp(float).  <cmath> above has declared everything
// the sources need; marking the wrapper as seen keeps a later `#include <math.h>` from adding the using-declarations.
#ifndef _GLIBCXX_MATH_H
#define _GLIBCXX_MATH_H 1
#endif

#include "../pinned_exp.h"

// The sources are compiled as nvcc would see them: helper_math.h then leaves min/max/fminf/rsqrtf to the toolkit (to
// this file) instead of defining host stand-ins that some translation units would see and others not, and glm takes its
// CUDA configuration (GLM_FORCE_CUDA is set by the sources).
#ifndef __CUDACC__
#define __CUDACC__ 1
#endif
#ifndef CUDA_VERSION
#define CUDA_VERSION 12000
#endif

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
// block-wide storage: one object shared by every fiber of the (single) block in flight
#define __shared__ static

// ---------------------------------------------------------------- vector types (helper_math.h supplies the operators)
#define REF_VEC(T, N)                                                                   \
  struct N##2 { T x, y; };                                                              \
  struct N##3 { T x, y, z; };                                                           \
  struct N##4 { T x, y, z, w; };                                                        \
  inline N##2 make_##N##2(T x, T y) { return N##2{x, y}; }                              \
  inline N##3 make_##N##3(T x, T y, T z) { return N##3{x, y, z}; }                      \
  inline N##4 make_##N##4(T x, T y, T z, T w) { return N##4{x, y, z, w}; }
REF_VEC(float, float)
REF_VEC(int, int)
REF_VEC(unsigned int, uint)
#undef REF_VEC

struct dim3 {
  unsigned int x, y, z;
  dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
  dim3(uint3 v) : x(v.x), y(v.y), z(v.z) {}
};

namespace ref_exec {
// the running fiber's coordinates; rewritten at every switch
extern uint3 thread_idx, block_idx;
extern dim3 block_dim, grid_dim;
void block_sync();                 // barrier over the live threads of the block
int block_sync_count(int pred);    // barrier; the number of threads whose pred was non-zero
// run `body` once per thread of every block of the grid (blocks ascending, one at a time)
void run_grid(dim3 grid, dim3 block, const std::function<void()>& body);

template <class K>
struct Launch {
  dim3 grid, block;
  K kernel;
  template <class... A>
  void operator()(A... args) const {
    const K& k = kernel;
    run_grid(grid, block, [&]() { k(args...); });
  }
};
template <class K>
Launch<K> launch(dim3 grid, dim3 block, K k) { return Launch<K>{grid, block, k}; }
}  // namespace ref_exec

#define threadIdx (::ref_exec::thread_idx)
#define blockIdx (::ref_exec::block_idx)
#define blockDim (::ref_exec::block_dim)
#define gridDim (::ref_exec::grid_dim)

// `kernel<<<grid, block>>>(args)` is rewritten by the build recipe into REF_LAUNCH((kernel), grid, block)(args)
#define REF_LAUNCH(kernel, ...) ::ref_exec::launch(__VA_ARGS__, [](auto... a) { kernel(a...); })

inline void __syncthreads() { ref_exec::block_sync(); }
inline int __syncthreads_count(int pred) { return ref_exec::block_sync_count(pred); }
[[noreturn]] inline void __trap() { std::abort(); }

template <class T>
inline T atomicAdd(T* p, T v) { T old = *p; *p = old + v; return old; }

// ---------------------------------------------------------------- global-namespace math, as CUDA declares it
inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
inline unsigned int min(unsigned int a, unsigned int b) { return a < b ? a : b; }
inline unsigned int max(unsigned int a, unsigned int b) { return a > b ? a : b; }
inline unsigned int min(unsigned int a, int b) { return min(a, (unsigned int)b); }
inline unsigned int min(int a, unsigned int b) { return min((unsigned int)a, b); }
inline unsigned int max(unsigned int a, int b) { return max(a, (unsigned int)b); }
inline unsigned int max(int a, unsigned int b) { return max((unsigned int)a, b); }
inline float min(float a, float b) { return __builtin_fminf(a, b); }
inline float max(float a, float b) { return __builtin_fmaxf(a, b); }
inline float rsqrtf(float x) { return 1.0f / std::sqrt(x); }
inline float sqrt(float x) { return std::sqrt(x); }
inline float ceil(float x) { return std::ceil(x); }
inline float floor(float x) { return std::floor(x); }
inline float sin(float x) { return std::sin(x); }
inline float cos(float x) { return std::cos(x); }
inline float exp(float x) {
#ifdef REF_LIBM_EXP
  return std::exp(x);
#else
  return pinned_expf(x);
#endif
}

// ---------------------------------------------------------------- the few runtime calls the host code makes
typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice };
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t) { return "no error"; }
inline cudaError_t cudaMemcpy(void* dst, const void* src, size_t n, cudaMemcpyKind) { std::memcpy(dst, src, n); return cudaSuccess; }
inline cudaError_t cudaMemset(void* dst, int v, size_t n) { std::memset(dst, v, n); return cudaSuccess; }
