// bmv_pair.hip -- the pair kernel of bmv_pair and bmv_align_paired (bmv_pair.hip.h), in a translation unit of its own like
// bmv_best.hip.
#include "bmv_pair.hip.h"

namespace bmv {

// One pass over the combinations of the pair's two groups.  SECOND = false: the pick -- (sum, i << 32 | j), the minimum in that
// order, across the wave.  SECOND = true: the smallest sum among the proper combinations that differ from the pick (home_i,
// home_j) in the locus of either mate; `ij` is not used.
template <bool SECOND>
__device__ __forceinline__ void pair_scan(const PairJob &P, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1, uint32_t lane,
                                          const PairCand &home_i, const PairCand &home_j, uint64_t &sum, uint64_t &ij) {
    uint64_t best_s = kPairNone, best_ij = kPairNone;
    for (uint64_t jb = b0; jb < b1; jb += (uint64_t)kWave) {
        const uint64_t j = jb + lane;
        const PairCand cj = pair_load(P, j, j < b1);
        if (__ballot(cj.known) == 0ull) continue;               // (the whole wave: jb is the same in every lane)
        const bool j_home = SECOND && cj.rc == home_j.rc && cj.at() == home_j.at();
        for (uint32_t i = a0; i < a1; i++) {
            const PairCand ci = pair_load(P, i, true);          // the same words in every lane
            if (!ci.known) continue;
            if (!pair_proper(P, ci, cj)) continue;
            if (SECOND && j_home && ci.rc == home_i.rc && ci.at() == home_i.at()) continue;
            const uint64_t s = (uint64_t)ci.edits + (uint64_t)cj.edits, at = ((uint64_t)i << 32) | j;
            if (s < best_s || (!SECOND && s == best_s && at < best_ij)) {
                best_s = s;
                best_ij = at;
            }
        }
    }
    // across the wave: the smallest sum, then among the lanes that hold it the smallest (i, j)
    sum = pair_wave_min(best_s, lane);
    if (!SECOND) ij = pair_wave_min(best_s == sum ? best_ij : kPairNone, lane);
}

__global__ __launch_bounds__(kPairWaves *kWave) void bmv_pair_kernel(PairJob P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t p = blockIdx.x * kPairWaves + threadIdx.x / (uint32_t)kWave;     // the same in every lane of a wave
    if (p >= P.n_pairs) return;
    const uint32_t a0 = P.group_offset[2u * p], a1 = P.group_offset[2u * p + 1u], b1 = P.group_offset[2u * p + 2u];
    const uint32_t win_a = pair_own_winner(P, a0, a1, lane), win_b = pair_own_winner(P, a1, b1, lane);
    uint64_t s1 = kPairNone, s2 = kPairNone, ij = kPairNone;
    uint32_t pick_a = win_a, pick_b = win_b;
    if (win_a != kBestBeyond && win_b != kBestBeyond) {         // (else one mate has no known candidate: nothing is proper)
        const PairCand none{};
        pair_scan<false>(P, a0, a1, a1, b1, lane, none, none, s1, ij);
        if (s1 != kPairNone) {
            pick_a = (uint32_t)(ij >> 32);
            pick_b = (uint32_t)ij;
            const PairCand home_i = pair_load(P, pick_a, true), home_j = pair_load(P, pick_b, true);
            uint64_t unused = 0;
            pair_scan<true>(P, a0, a1, a1, b1, lane, home_i, home_j, s2, unused);
        }
    }
    if (lane == 0) {
        P.pick[2u * p] = pick_a;
        P.pick[2u * p + 1u] = pick_b;
        P.winner[2u * p] = win_a;
        P.winner[2u * p + 1u] = win_b;
        P.proper[p] = s1 != kPairNone ? 1 : 0;
        P.s1[p] = s1;
        P.s2[p] = s2;
    }
}

}  // namespace bmv
