// bmv_clip.hip -- the soft-clipping kernels of bmv_clip (bmv_clip.hip.h), in a translation unit of their own (declared
// `extern` in bmv_clip.hip.h), like bmv_annotate.hip: no other kernel's device code is recompiled beside them.
#include "bmv_clip.hip.h"

namespace bmv {
template __global__ void bmv_clip_range_kernel<kAnnotateWaves>(ClipJob);
template __global__ void bmv_clip_emit_kernel<false>(ClipJob);
template __global__ void bmv_clip_emit_kernel<true>(ClipJob);
}  // namespace bmv
