// bmv_split.hip.h -- the two kernels of bmv_split and bmv_split_pick (include/bmv.h): per candidate alignment the stretch
// bmv_clip would keep, as a query interval in read orientation and a reference interval in genome coordinates; per read the
// non-conflicting set of those stretches, primary first, each with the score of its strongest competitor.
//
// bmv_split_range_kernel: bmv_clip_range_kernel's walk (bmv_clip.hip.h: a wave per alignment, 64 columns of an M entry per
// step, forward-strand order, a prefix minimum and a wave maximum per step, no LDS, no scratch), copied rather than shared --
// bmv_clip's device code stays what it was.  Where clip carries column indices and walks twice more to turn them into
// clip_left, clip_right, pos and ref_len, this walk carries the CURSORS: the minimum and the best (score, r, l) each keep
// the text and query cursors (ti, qi) at their border.  A border after lane j of an M step that began at (ti + c, qi + c) lies
// at (ti + c + j + 1, qi + c + j + 1); an I or D entry is one element, its end the cursors behind it.  The order of the columns
// decides every tie (the later minimum, the earlier r), so no column index is kept at all.  Sums are 64-bit as in clip; the
// cursors are bounded by text_len and query_len and take 32.  Lane 0 writes score, q_lo, q_hi, g_lo and g_hi.
//
// bmv_split_pick_kernel: a wave per group, kSplitWaves groups a block, nothing shared between the waves.  The candidates sit
// in the lanes 64 at a time; a group of any size is a loop of chunks.  The pick keeps no state per candidate: in every round a
// candidate is alive when it is eligible and conflicts with none of the chosen, which is tested anew against the at most 16
// chosen intervals.  Those live one per lane -- chosen k in lane k -- and are broadcast with a wave-uniform lane index.  The
// round's winner is the wave maximum of (S, lowest index); S can reach 2^43, so the score and the index travel as two words
// compared in order.  max_segments rounds of ceil(size / 64) chunk steps at most; the first round without a winner ends the
// list.  A last sweep gives s2 of every chosen one: per chosen k a wave maximum over the chunk's competitors, kept in lane k.
// Results are plain vector stores: lane k writes slot k of the group's row.
#pragma once

#include "bmv_annotate.hip.h"

namespace bmv {

constexpr uint32_t kSplitWaves = 4;                 // alignments (range) or groups (pick) per 256-thread block
constexpr uint32_t kSplitMaxSegments = 16;          // BMV_SPLIT_MAX_SEGMENTS
constexpr uint32_t kSplitBeyond = 0xFFFFFFFFu;      // BMV_BEYOND
constexpr int64_t kSplitNone = INT64_MIN;           // BMV_SPLIT_NONE

struct SplitRangeJob {
    AnnotateJob a;                  // the inputs only: views, begin, M/I/D entries, count
    uint32_t match, penalty;        // 1 .. 1024 each, checked on the host
    int64_t *score;                 // per alignment
    uint32_t *q_lo, *q_hi;
    int64_t *g_lo, *g_hi;
};

struct SplitPickJob {
    const int64_t *score;           // per alignment of the batch
    const uint32_t *q_lo, *q_hi;
    const int64_t *g_lo, *g_hi;
    const uint8_t *text_rc;
    const uint32_t *contig;         // null: one contig
    const uint32_t *group_offset;   // n_groups + 1
    uint32_t n_groups;
    int64_t min_score;
    uint64_t max_overlap_permille;
    uint32_t max_segments;          // 1 .. kSplitMaxSegments
    uint32_t *n_seg;                // n_groups
    uint32_t *seg;                  // n_groups * max_segments
    int64_t *s2;                    // n_groups * max_segments
};

__device__ __forceinline__ uint32_t split_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t split_uniform(uint64_t v) {
    return (uint64_t)split_uniform((uint32_t)(v >> 32)) << 32 | split_uniform((uint32_t)v);
}
// lane k's value in every lane; k is the same in every lane
__device__ __forceinline__ uint32_t split_lane(uint32_t v, uint32_t k) { return (uint32_t)__shfl((int)v, (int)k, 64); }
__device__ __forceinline__ int64_t split_lane(int64_t v, uint32_t k) { return (int64_t)__shfl((long long)v, (int)k, 64); }

// what the pick needs of one alignment
struct SplitCand {
    int64_t s, g_lo, g_hi;
    uint32_t q_lo, q_hi, contig;
    bool rc;
    __device__ __forceinline__ uint64_t qlen() const { return (uint64_t)(q_hi - q_lo); }
};

__device__ __forceinline__ SplitCand split_load(const SplitPickJob &P, uint64_t a, bool have) {
    SplitCand c{};
    if (have) {
        c.s = P.score[a];
        c.q_lo = P.q_lo[a];
        c.q_hi = P.q_hi[a];
        c.g_lo = P.g_lo[a];
        c.g_hi = P.g_hi[a];
        c.rc = P.text_rc[a] != 0;
        c.contig = P.contig ? P.contig[a] : 0u;
    }
    return c;
}

__device__ __forceinline__ SplitCand split_broadcast(const SplitCand &c, uint32_t k) {
    SplitCand o;
    o.s = split_lane(c.s, k);
    o.g_lo = split_lane(c.g_lo, k);
    o.g_hi = split_lane(c.g_hi, k);
    o.q_lo = split_lane(c.q_lo, k);
    o.q_hi = split_lane(c.q_hi, k);
    o.contig = split_lane(c.contig, k);
    o.rc = split_lane(c.rc ? 1u : 0u, k) != 0u;
    return o;
}

__device__ __forceinline__ uint64_t split_ovl_q(const SplitCand &x, const SplitCand &y) {
    const uint32_t lo = x.q_lo > y.q_lo ? x.q_lo : y.q_lo, hi = x.q_hi < y.q_hi ? x.q_hi : y.q_hi;
    return hi > lo ? (uint64_t)(hi - lo) : 0ull;
}

__device__ __forceinline__ bool split_dup(const SplitCand &x, const SplitCand &y, uint64_t ovl_q) {
    const int64_t lo = x.g_lo > y.g_lo ? x.g_lo : y.g_lo, hi = x.g_hi < y.g_hi ? x.g_hi : y.g_hi;
    return x.contig == y.contig && x.rc == y.rc && hi > lo && ovl_q > 0ull;
}

__device__ __forceinline__ bool split_conflict(const SplitPickJob &P, const SplitCand &x, const SplitCand &y) {
    const uint64_t ovl = split_ovl_q(x, y), shorter = x.qlen() < y.qlen() ? x.qlen() : y.qlen();
    return split_dup(x, y, ovl) || ovl * 1000ull > P.max_overlap_permille * shorter;
}

// the greatest v across the wave, in every lane
__device__ __forceinline__ int64_t split_wave_max(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t t = (int64_t)__shfl_xor((long long)v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// defined in bmv_split.hip
template <uint32_t WAVES>
__global__ void bmv_split_range_kernel(SplitRangeJob C);
extern template __global__ void bmv_split_range_kernel<kSplitWaves>(SplitRangeJob);
__global__ void bmv_split_pick_kernel(SplitPickJob P);

}  // namespace bmv
