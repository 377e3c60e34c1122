// bmv_pair.hip.h -- the pair-aware pick of bmv_pair and bmv_align_paired (include/bmv.h): of the candidate alignments of two
// mates, the combination that places them as a proper pair at the fewest edits, and the runner-up at another locus.
//
// A wave per pair; a block holds kPairWaves of them and nothing is shared between its waves (no LDS, no barrier).  The
// candidates of the SECOND mate sit in the lanes, 64 at a time; the candidates of the first mate are walked one after the other
// by the whole wave (every lane loads the same words).  Both group sizes are unbounded, so both dimensions are loops: a pair
// of 130 x 130 candidates is three lane chunks times 130 steps.  An unknown candidate (edits == kBestBeyond) of the first mate
// skips its step for the whole wave, a lane chunk without a known candidate is skipped whole.
//   pass 1   per lane the minimum of (sum, i << 32 | j) over its proper combinations, then the minimum across the wave:
//            the pick (the sum is below 2^33 and the two indices take 64 bits: two words, compared in order)
//   pass 2   only when there is a pick: the smallest sum over the proper combinations at another locus than the pick's
// The own winner of either group is bmv_best_pick_kernel's key (edits << 32 | index) minimised over the known candidates.
// Coordinates are signed 64-bit (the host checks text_start < 2^62).  Results are plain vector stores from lane 0.
#pragma once

#include "bmv_best.hip.h"

namespace bmv {

constexpr uint32_t kPairWaves = 4;                  // pairs per block
constexpr uint64_t kPairNone = ~0ull;               // BMV_PAIR_NONE

struct PairJob {
    const uint64_t *text_start;     // per alignment of the batch
    const uint32_t *text_len;
    const uint8_t *text_rc;
    const uint32_t *query_len;
    const uint32_t *edits;          // a distance or kBestBeyond
    const uint32_t *end;
    const uint32_t *contig;         // null: one contig
    const uint32_t *group_offset;   // 2 * n_pairs + 1
    uint32_t n_pairs;
    int64_t min_frag, max_frag;
    uint32_t *pick;                 // 2 * n_pairs
    uint32_t *winner;               // 2 * n_pairs
    uint8_t *proper;                // n_pairs
    uint64_t *s1, *s2;              // n_pairs
};

// what the pick needs of one alignment
struct PairCand {
    bool known, rc;
    uint32_t contig, edits;
    int64_t l, r;                   // L(a) and R(a) of bmv.h
    __device__ __forceinline__ int64_t at() const { return rc ? l : r; }    // the locus' coordinate: the exact one
};

__device__ __forceinline__ PairCand pair_load(const PairJob &P, uint64_t a, bool have) {
    PairCand c{};
    c.edits = have ? P.edits[a] : kBestBeyond;
    c.known = c.edits != kBestBeyond;
    if (c.known) {
        c.rc = P.text_rc[a] != 0;
        c.contig = P.contig ? P.contig[a] : 0u;
        const int64_t ts = (int64_t)P.text_start[a], end = (int64_t)P.end[a], m = (int64_t)P.query_len[a];
        if (c.rc) {
            c.l = ts + (int64_t)P.text_len[a] - end;
            c.r = c.l + m;
        } else {
            c.r = ts + end;
            c.l = c.r - m;
        }
    }
    return c;
}

__device__ __forceinline__ bool pair_proper(const PairJob &P, const PairCand &x, const PairCand &y) {
    if (!x.known || !y.known || x.contig != y.contig || x.rc == y.rc) return false;
    const int64_t fl = x.rc ? y.l : x.l, fr = x.rc ? y.r : x.r;       // the forward one
    const int64_t rl = x.rc ? x.l : y.l, rr = x.rc ? x.r : y.r;       // the reverse one
    const int64_t frag = rr - fl;
    return fl <= rl && fr <= rr && frag >= P.min_frag && frag <= P.max_frag;
}

__device__ __forceinline__ uint64_t pair_wave_min(uint64_t v, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint64_t other = shfl64(v, (int)(lane ^ (uint32_t)o));
        v = other < v ? other : v;
    }
    return v;
}

// the own winner of the group a0 .. a1 - 1
__device__ __forceinline__ uint32_t pair_own_winner(const PairJob &P, uint32_t a0, uint32_t a1, uint32_t lane) {
    uint64_t key = kPairNone;
    for (uint64_t a = (uint64_t)a0 + lane; a < a1; a += (uint64_t)kWave) {
        const uint32_t e = P.edits[a];
        const uint64_t ka = ((uint64_t)e << 32) | a;
        key = (e != kBestBeyond && ka < key) ? ka : key;
    }
    key = pair_wave_min(key, lane);
    return key == kPairNone ? kBestBeyond : (uint32_t)key;
}

// defined in bmv_pair.hip
__global__ void bmv_pair_kernel(PairJob P);

}  // namespace bmv
