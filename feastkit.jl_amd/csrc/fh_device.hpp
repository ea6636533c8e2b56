// fh_device.hpp -- device helpers that more than one .hip unit uses.
#pragma once
#include "fh_common.hpp"

__device__ __forceinline__ bool fh_finite(cplx a) { return isfinite(a.x) && isfinite(a.y); }
