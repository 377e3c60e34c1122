// bmv_overlap.hip -- the kernels of bmv_overlap (bmv_overlap.hip.h), in a translation unit of their own (declared `extern`
// in bmv_overlap.hip.h), like bmv_clip.hip: no other kernel's device code is recompiled beside them.
#include "bmv_overlap.hip.h"

namespace bmv {
template __global__ void bmv_overlap_span_kernel<false>(OverlapJob);
template __global__ void bmv_overlap_span_kernel<true>(OverlapJob);
template __global__ void bmv_overlap_decide_kernel<kOverlapThreads>(OverlapJob);
template __global__ void bmv_overlap_restrict_kernel<kAnnotateWaves>(OverlapJob);
template __global__ void bmv_overlap_commit_kernel<kOverlapThreads>(OverlapJob);
template __global__ void bmv_overlap_score_kernel<kOverlapThreads>(OverlapJob);
}  // namespace bmv
