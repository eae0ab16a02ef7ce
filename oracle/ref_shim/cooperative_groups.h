// cooperative_groups.h of oracle/ref_shim: the grid and the thread block of the execution model in cuda_runtime.h.
#pragma once
#include "cuda_runtime.h"

namespace cooperative_groups {

struct grid_group {
  unsigned long long thread_rank() const {
    const unsigned long long block = ((unsigned long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const unsigned long long in_block = ((unsigned long long)threadIdx.z * blockDim.y + threadIdx.y) * blockDim.x + threadIdx.x;
    return block * ((unsigned long long)blockDim.x * blockDim.y * blockDim.z) + in_block;
  }
};

struct thread_block {
  void sync() const { ref_exec::block_sync(); }
  unsigned int thread_rank() const { return (threadIdx.z * blockDim.y + threadIdx.y) * blockDim.x + threadIdx.x; }
  unsigned int size() const { return blockDim.x * blockDim.y * blockDim.z; }
  dim3 group_index() const { return dim3(blockIdx); }
  dim3 thread_index() const { return dim3(threadIdx); }
};

inline grid_group this_grid() { return grid_group(); }
inline thread_block this_thread_block() { return thread_block(); }

}  // namespace cooperative_groups
