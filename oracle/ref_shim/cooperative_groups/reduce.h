// cooperative_groups/reduce.h of oracle/ref_shim: the kernels include it and use nothing of it.
#pragma once
#include "../cooperative_groups.h"
