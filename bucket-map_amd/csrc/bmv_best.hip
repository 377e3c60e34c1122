// bmv_best.hip -- the distance and pick kernels of bmv_align_best (bmv_best.hip.h), instantiated in a translation unit of
// their own (declared `extern template` in bmv_best.hip.h), like bmv_screen.hip.
#include "bmv_best.hip.h"

namespace bmv {

// A wave per 64 consecutive groups.  Groups of up to 64 members: a lane each, two passes over the members.  Larger groups:
// the whole wave, one group after the other, members strided over the lanes and the minimum taken across the wave.  The key
// (d << 32 | batch index) orders by distance, then by index; kBestBeyond sorts last and never wins (a group's seed always has
// a distance).
__global__ __launch_bounds__(kWave) void bmv_best_pick_kernel(PickJob P) {
    const uint32_t lane = threadIdx.x, g = blockIdx.x * kWave + lane;
    const bool have = g < P.n_groups;
    const uint32_t a0 = have ? P.group_offset[g] : 0u, a1 = have ? P.group_offset[g + 1u] : 0u;
    const uint32_t size = a1 - a0;
    const uint64_t none = ~0ull;
    if (have && size <= (uint32_t)kWave) {
        uint64_t key = none;
        for (uint32_t a = a0; a < a1; a++) {
            const uint64_t ka = ((uint64_t)P.d[a] << 32) | a;
            key = ka < key ? ka : key;
        }
        const uint32_t w = size ? (uint32_t)key : kBestBeyond;
        const uint64_t reach = (key >> 32) + (uint64_t)P.margin[g];       // best + margin, in 64 bits
        for (uint32_t a = a0; a < a1; a++) {
            const uint32_t da = P.d[a];
            const bool in = da != kBestBeyond && (uint64_t)da <= reach;
            P.out_edits[a] = in ? da : kBestBeyond;
            P.out_end[a] = in ? P.end[a] : 0u;
        }
        P.winner[g] = w;
        P.need[g] = (size && P.full[w] == 0u) ? 1u : 0u;
    }
    uint64_t big = __ballot(have && size > (uint32_t)kWave);
    while (big) {
        const uint32_t src = (uint32_t)__builtin_ctzll(big);
        big &= big - 1ull;
        const uint32_t gg = blockIdx.x * kWave + src;
        const uint32_t b0 = (uint32_t)__shfl((int)a0, (int)src, kWave), b1 = (uint32_t)__shfl((int)a1, (int)src, kWave);
        uint64_t key = none;
        for (uint32_t a = b0 + lane; a < b1; a += (uint32_t)kWave) {
            const uint64_t ka = ((uint64_t)P.d[a] << 32) | a;
            key = ka < key ? ka : key;
        }
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint64_t other = shfl64(key, (int)(lane ^ (uint32_t)o));
            key = other < key ? other : key;
        }
        const uint32_t w = (uint32_t)key;
        const uint64_t reach = (key >> 32) + (uint64_t)P.margin[gg];
        for (uint32_t a = b0 + lane; a < b1; a += (uint32_t)kWave) {
            const uint32_t da = P.d[a];
            const bool in = da != kBestBeyond && (uint64_t)da <= reach;
            P.out_edits[a] = in ? da : kBestBeyond;
            P.out_end[a] = in ? P.end[a] : 0u;
        }
        if (lane == 0) {
            P.winner[gg] = w;
            P.need[gg] = P.full[w] == 0u ? 1u : 0u;
        }
    }
}

__global__ void bmv_best_compact_kernel(const uint32_t *__restrict__ need, const uint32_t *__restrict__ where,
                                        const uint32_t *__restrict__ winner, uint32_t n_groups, uint32_t *__restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n_groups && need[g]) out[where[g]] = winner[g];
}

template __global__ void bmv_best_lane_kernel<1>(BestJob);
template __global__ void bmv_best_lane_kernel<2>(BestJob);
template __global__ void bmv_best_lane_kernel<3>(BestJob);
template __global__ void bmv_best_lane_kernel<4>(BestJob);
template __global__ void bmv_best_lane_kernel<5>(BestJob);
template __global__ void bmv_best_lane_kernel<6>(BestJob);
template __global__ void bmv_best_lane_kernel<7>(BestJob);
template __global__ void bmv_best_lane_kernel<8>(BestJob);
template __global__ void bmv_best_wave_kernel<1>(BestJob);
template __global__ void bmv_best_wave_kernel<2>(BestJob);
template __global__ void bmv_best_wave_kernel<4>(BestJob);
}  // namespace bmv
