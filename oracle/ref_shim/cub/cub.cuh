// cub/cub.cuh of oracle/ref_shim: the two device-wide primitives the rasteriser's host code calls, as their definitions.
// Called with a null workspace they report a workspace size and do nothing, as cub does.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../cuda_runtime.h"

namespace cub {

struct DeviceScan {
  // out[i] = in[0] + ... + in[i]; in and out may be the same array
  template <class In, class Out>
  static cudaError_t InclusiveSum(void* d_temp_storage, size_t& temp_storage_bytes, In d_in, Out d_out, int num_items) {
    if (d_temp_storage == nullptr) {
      temp_storage_bytes = 1;
      return cudaSuccess;
    }
    if (num_items > 0) {
      auto acc = d_in[0];
      d_out[0] = acc;
      for (int i = 1; i < num_items; ++i) {
        acc = acc + d_in[i];
        d_out[i] = acc;
      }
    }
    return cudaSuccess;
  }
};

struct DeviceRadixSort {
  // ascending, stable, comparing only key bits [begin_bit, end_bit): an LSD radix sort's result, whatever its digit size
  template <class Key, class Value>
  static cudaError_t SortPairs(void* d_temp_storage, size_t& temp_storage_bytes, const Key* d_keys_in, Key* d_keys_out,
                               const Value* d_values_in, Value* d_values_out, int num_items, int begin_bit = 0,
                               int end_bit = sizeof(Key) * 8) {
    if (d_temp_storage == nullptr) {
      temp_storage_bytes = 1;
      return cudaSuccess;
    }
    const int bits = end_bit - begin_bit;
    const Key mask = bits >= (int)(sizeof(Key) * 8) ? ~Key(0) : (bits <= 0 ? Key(0) : (((Key(1) << bits) - 1) << begin_bit));
    std::vector<int> order(num_items > 0 ? num_items : 0);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return (d_keys_in[a] & mask) < (d_keys_in[b] & mask); });
    for (int i = 0; i < num_items; ++i) {
      d_keys_out[i] = d_keys_in[order[i]];
      d_values_out[i] = d_values_in[order[i]];
    }
    return cudaSuccess;
  }
};

}  // namespace cub
