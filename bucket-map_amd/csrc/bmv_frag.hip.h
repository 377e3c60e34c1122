// bmv_frag.hip.h -- the fragment spans of bmv_frag_spans and bmv_paired_begin (include/bmv.h): per pair the span of the two own
// winners when both mates are placed without a doubt, and the histogram of those spans, from which the host learns the range a
// proper pair may span (host/frag_range.h).
//
// Span kernel: a wave per pair, kPairWaves pairs a block, nothing shared between the waves -- bmv_pair_kernel's shape, and its
// pair_load / pair_proper / pair_own_winner / pair_wave_min.  A group is SETTLED when it has an own winner and every known
// candidate lies at the winner's locus; the group's size is unbounded, so the test walks it in lane chunks of 64 and a ballot
// per chunk ends the walk at the first candidate elsewhere.  span[p] = R(reverse) - L(forward) of the two winners when both
// groups are settled and the winners are proper under [1, cap], else 0.  One plain vector store from lane 0.
//
// Histogram kernel: a resident grid of kFragHistThreads-lane blocks strides over span[].  Up to kFragLdsBins bins
// (64 KiB of LDS, the most a block may ask for without an opt-in) the bins are private to the block in LDS: zeroed, filled
// with LDS atomic adds, and after a barrier only the non-zero ones go to the global bins with one atomic add each.  Beyond that
// the adds go to the global bins directly, one per distinct span of a wave's 64 (bmv_frag.hip says why).  The host zeroes the
// global bins before every launch and sizes the grid so that a block has at least as many spans as bins to justify its zeroing
// and flushing (bmv_api.hip: run_frag).
#pragma once

#include "bmv_pair.hip.h"

namespace bmv {

constexpr uint32_t kFragHistThreads = 256;
constexpr uint32_t kFragLdsBins = 16384;            // (cap + 1) up to this: bins in LDS
constexpr uint32_t kFragMaxCap = 65535;

struct FragJob {
    PairJob P;                      // the inputs as the pair kernel takes them; min_frag = 1, max_frag = cap; no outputs
    uint32_t *span;                 // n_pairs
};

// is every known candidate of the group a0 .. a1 - 1 at the locus of `home`?  (wave-uniform result)
__device__ __forceinline__ bool frag_settled(const PairJob &P, uint32_t a0, uint32_t a1, const PairCand &home, uint32_t lane) {
    for (uint64_t ab = a0; ab < a1; ab += (uint64_t)kWave) {
        const uint64_t a = ab + lane;
        const PairCand c = pair_load(P, a, a < a1);
        if (__ballot(c.known && (c.rc != home.rc || c.at() != home.at())) != 0ull) return false;
    }
    return true;
}

// defined in bmv_frag.hip
__global__ void bmv_frag_span_kernel(FragJob F);
__global__ void bmv_frag_hist_lds_kernel(const uint32_t *span, uint32_t n_pairs, uint32_t n_bins, uint32_t *hist);
__global__ void bmv_frag_hist_global_kernel(const uint32_t *span, uint32_t n_pairs, uint32_t n_bins, uint32_t *hist);

}  // namespace bmv
