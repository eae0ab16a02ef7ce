// cub/device/device_radix_sort.cuh of oracle/ref_shim: see ../cub.cuh.
#pragma once
#include "../cub.cuh"
