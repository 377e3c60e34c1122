// bmv_frag.hip -- the span and histogram kernels of bmv_frag_spans and bmv_paired_begin (bmv_frag.hip.h), in a translation unit
// of their own like bmv_pair.hip.
#include "bmv_frag.hip.h"

namespace bmv {

__global__ __launch_bounds__(kPairWaves *kWave) void bmv_frag_span_kernel(FragJob F) {
    const PairJob &P = F.P;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * kPairWaves + threadIdx.x / (uint32_t)kWave;     // the same in every lane of a wave
    if (p >= P.n_pairs) return;
    const uint32_t a0 = P.group_offset[2u * p], a1 = P.group_offset[2u * p + 1u], b1 = P.group_offset[2u * p + 2u];
    const uint32_t win_a = pair_own_winner(P, a0, a1, lane), win_b = pair_own_winner(P, a1, b1, lane);
    uint32_t span = 0u;
    if (win_a != kBestBeyond && win_b != kBestBeyond) {
        const PairCand wa = pair_load(P, win_a, true), wb = pair_load(P, win_b, true);      // the same words in every lane
        if (pair_proper(P, wa, wb) && frag_settled(P, a0, a1, wa, lane) && frag_settled(P, a1, b1, wb, lane))
            span = (uint32_t)(wa.rc ? wa.r - wb.l : wb.r - wa.l);       // R(reverse) - L(forward), in [1, cap] by pair_proper
    }
    if (lane == 0) F.span[p] = span;
}

__global__ __launch_bounds__(kFragHistThreads) void bmv_frag_hist_lds_kernel(const uint32_t *span, uint32_t n_pairs, uint32_t n_bins,
                                                                            uint32_t *hist) {
    extern __shared__ uint32_t bins[];              // n_bins
    for (uint32_t b = threadIdx.x; b < n_bins; b += kFragHistThreads) bins[b] = 0u;
    __syncthreads();
    const uint32_t stride = gridDim.x * kFragHistThreads;
    for (uint32_t p = blockIdx.x * kFragHistThreads + threadIdx.x; p < n_pairs; p += stride) {
        const uint32_t s = span[p];
        if (s < n_bins) atomicAdd(&bins[s], 1u);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < n_bins; b += kFragHistThreads) {
        const uint32_t k = bins[b];
        if (k) atomicAdd(&hist[b], k);
    }
}

__global__ __launch_bounds__(kFragHistThreads) void bmv_frag_hist_global_kernel(const uint32_t *span, uint32_t n_pairs, uint32_t n_bins,
                                                                               uint32_t *hist) {
    // A library's spans crowd into a few bins (simulated data: into one), and a global atomic add per span then queues on one
    // address: 4.4 ms for 500 000 pairs of one fragment length, measured on the form that did so (profiles/r14).  So a wave
    // adds once per DISTINCT span among its 64 -- 0.47 ms on the same batch, either figure with the span kernel's time --: the first lane still to
    // do leads, the lanes with its span are counted by a ballot, and the leader adds their number.
    const uint32_t lane = threadIdx.x & 63u, stride = gridDim.x * kFragHistThreads;
    for (uint32_t p0 = blockIdx.x * kFragHistThreads + (threadIdx.x & ~63u); p0 < n_pairs; p0 += stride) {     // (wave-uniform)
        const uint32_t p = p0 + lane;
        const uint32_t s = p < n_pairs ? span[p] : n_bins;
        uint64_t todo = __ballot(s < n_bins);
        while (todo != 0ull) {
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
            const uint32_t v = (uint32_t)__shfl((int)s, (int)leader);
            const uint64_t same = __ballot(s == v);             // (all of them still to do: a lane leaves with its span)
            if (lane == leader) atomicAdd(&hist[v], (uint32_t)__popcll(same));
            todo &= ~same;
        }
    }
}

}  // namespace bmv
