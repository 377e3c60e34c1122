// bmv_screen.hip -- the score-only screen kernels of bmv_align_bounded (bmv_screen.hip.h), instantiated in a translation
// unit of their own (declared `extern template` in bmv_screen.hip.h), like bmv_long.hip.
#include "bmv_screen.hip.h"

namespace bmv {
__global__ void bmv_screen_compact_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ where, uint32_t n,
                                          uint32_t *__restrict__ out) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a < n && keep[a]) out[where[a]] = a;
}

template __global__ void bmv_screen_lane_kernel<1>(ScreenJob);
template __global__ void bmv_screen_lane_kernel<2>(ScreenJob);
template __global__ void bmv_screen_lane_kernel<3>(ScreenJob);
template __global__ void bmv_screen_lane_kernel<4>(ScreenJob);
template __global__ void bmv_screen_lane_kernel<5>(ScreenJob);
template __global__ void bmv_screen_lane_kernel<6>(ScreenJob);
template __global__ void bmv_screen_lane_kernel<7>(ScreenJob);
template __global__ void bmv_screen_lane_kernel<8>(ScreenJob);
template __global__ void bmv_screen_wave_kernel<1>(ScreenJob);
template __global__ void bmv_screen_wave_kernel<2>(ScreenJob);
template __global__ void bmv_screen_wave_kernel<4>(ScreenJob);
}  // namespace bmv
