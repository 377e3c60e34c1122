// bmv_long.hip -- the kernels of bmv_align_long (bmv_long.hip.h), instantiated in a translation unit of their own
// (declared `extern template` in bmv_long.hip.h), like bmv_variants*.hip: compile time stays bounded.
#include "bmv_long.hip.h"

namespace bmv {
template __global__ void bmv_long_prep_kernel<kLongCw>(LongJob, uint32_t);
template __global__ void bmv_long_tile_kernel<kLongCw>(LongJob);
template __global__ void bmv_long_traceback_kernel<kLongCw>(LongJob);
}  // namespace bmv
