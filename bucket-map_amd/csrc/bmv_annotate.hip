// bmv_annotate.hip -- the annotation kernels of bmv_annotate (bmv_annotate.hip.h), instantiated in a translation unit of
// their own (declared `extern template` in bmv_annotate.hip.h), like bmv_screen.hip: the aligning kernels' device code is not
// recompiled beside them.
#include "bmv_annotate.hip.h"

namespace bmv {
template __global__ void bmv_annotate_kernel<false>(AnnotateJob);
template __global__ void bmv_annotate_kernel<true>(AnnotateJob);
}  // namespace bmv
