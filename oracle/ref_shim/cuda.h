// cuda.h of oracle/ref_shim: everything is in cuda_runtime.h (see there).
#pragma once
#include "cuda_runtime.h"
