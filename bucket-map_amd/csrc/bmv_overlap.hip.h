// bmv_overlap.hip.h -- the overlap pass of the verifier (bmv_overlap, include/bmv.h): the two mates of a pair are soft-clipped
// at one cut so that no reference base lies under both.  A post-pass of the bmv_annotate / bmv_clip family: the same inputs
// plus mate[] and contig[], the same forward-strand columns, bmv_clip's record layout.  No existing kernel is touched: the
// base range is bmv_clip's range kernel (or all columns), the records are written by bmv_clip's emit kernels from the
// restricted range.  Their stated assumptions hold for it: the restricted range still cuts M entries only; it may begin or
// end on an X column, which the emit's merge of adjacent runs takes like an `=` column (the walk is symmetric in the two:
// `open` carries either op across a step and an entry border, and is written when the next run's op differs).  In the mode
// without scores the range is all columns and may begin or end on a whole I or D entry, which the emit takes whole.
//
// The two mates meet BETWEEN launches, no kernel waits for another workgroup:
//   span      a wave per alignment: the base range [l, r) (written by bmv_clip's range kernel before it, or [0, C) here), and
//             G0 = g(l), G1 = g(r) from the CIGAR entries alone, 64 entries a step with a prefix sum across the wave
//   decide    a thread per alignment reads its own and its mate's (l, r, G0, G1): its role (none / first / second) and the cut m.
//             Both mates compute the same decision from the same numbers; each writes only its own slot
//   restrict  a wave per alignment with a role: r' (first) or l' (second) from the CIGAR entries alone -- every M column is `=`
//             or X, so "the last M column with g < m" needs no base --, whether it exists, and the query bases it would clip
//   commit    a thread per alignment: the restricted range when its own AND its mate's column exist, else the base range
//   (bmv_clip's count pass, two prefix sums, bmv_clip's write pass)
//   score     a thread per alignment, after the count pass: match x (= columns kept) - penalty x (X, I, D columns kept)
// All sums and coordinates are 64-bit; g is signed.
#pragma once

#include "bmv_clip.hip.h"

namespace bmv {

constexpr uint32_t kNoMate = 0xFFFFFFFFu;
constexpr uint32_t kOverlapNone = 0u, kOverlapFirst = 1u, kOverlapSecond = 2u;
constexpr uint32_t kOverlapThreads = 256;       // the per-alignment thread kernels

struct OverlapJob {
    ClipJob c;                      // c.l / c.r: the FINAL range, read by the emit kernels; c.score: the final score
    const uint32_t *mate;           // kNoMate: none
    const uint32_t *contig;         // NULL: all on one
    uint64_t *l0, *r0;              // the base range
    int64_t *g0, *g1;               // its ends in the concatenated genome
    int64_t *m;                     // the cut, where role != none
    uint32_t *role;
    uint64_t *edge;                 // restrict: r' of a first, l' of a second
    uint32_t *found;                // ... != 0 when that column exists
    uint32_t *cut_q;                // ... and the query bases between it and the base range's end
    uint32_t *cut;                  // commit: the query bases the cut added to the soft clips
    uint8_t *was_cut;               // ... and != 0 for a mate of a cut pair
};

__device__ __forceinline__ uint64_t overlap_scan(uint64_t v, uint32_t lane) {      // inclusive sum across the wave
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t o = (uint64_t)__shfl_up((long long)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ uint64_t overlap_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((long long)v, o, 64);
    return v;
}
__device__ __forceinline__ uint64_t overlap_last(uint64_t v) { return clip_uniform((uint64_t)__shfl((long long)v, 63, 64)); }

struct OverlapCols {
    uint64_t ref, qry;
};

// The reference- and the query-consuming columns before column x of the forward-strand columns, from the entries alone: 64
// entries a step, lane i the step's i-th entry in forward order; an entry that x cuts through counts its columns before x.
__device__ __forceinline__ OverlapCols overlap_before(const uint32_t *cig, uint32_t ne, bool rc, uint32_t lane, uint64_t x) {
    uint64_t col = 0, ref = 0, qry = 0;
    for (uint32_t k0 = 0; k0 < ne && col < x; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const uint32_t e = k < ne ? cig[rc ? ne - 1u - k : k] : 0u, op = e & 15u, len = e >> 4;
        const uint64_t incl = overlap_scan((uint64_t)len, lane), s = col + incl - len;
        const uint64_t take = s >= x ? 0ull : (x - s < (uint64_t)len ? x - s : (uint64_t)len);
        if (op != kOpI) ref += take;
        if (op != kOpD) qry += take;
        col += overlap_last(incl);
    }
    return {clip_uniform(overlap_sum(ref)), clip_uniform(overlap_sum(qry))};
}

// SCORED: l0 / r0 / pos0 are bmv_clip's range kernel's; else this kernel writes them: all columns, bmv_annotate's pos
template <bool SCORED>
__global__ __launch_bounds__(64 * kAnnotateWaves) void bmv_overlap_span_kernel(OverlapJob O) {
    const AnnotateJob &J = O.c.a;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kAnnotateWaves + (threadIdx.x >> 6)));
    if (a >= J.count) return;
    const uint64_t cig_at = J.cigar_offset[a];
    const uint32_t ne = (uint32_t)(J.cigar_offset[a + 1] - cig_at);
    const uint32_t *cig = J.cigar + cig_at;
    const bool rc = J.text_rc[a] != 0;
    uint64_t l, r;
    uint32_t pos0;
    if (SCORED) {
        l = O.l0[a];
        r = O.r0[a];
        pos0 = O.c.pos0[a];
    } else {
        uint64_t cols = 0, ref_all = 0;
        for (uint32_t k = lane; k < ne; k += 64u) {
            const uint32_t e = cig[k];
            cols += e >> 4;
            ref_all += (e & 15u) != kOpI ? e >> 4 : 0u;
        }
        cols = clip_uniform(overlap_sum(cols));
        ref_all = clip_uniform(overlap_sum(ref_all));
        l = 0;
        r = cols;
        pos0 = ne == 0u ? 0u : (rc ? J.text_len[a] - J.begin[a] - (uint32_t)ref_all : J.begin[a]);
    }
    const int64_t base = (int64_t)J.text_start[a] + (int64_t)pos0;
    const OverlapCols bl = overlap_before(cig, ne, rc, lane, l), br = overlap_before(cig, ne, rc, lane, r);
    if (lane == 0) {
        if (!SCORED) {
            O.l0[a] = l;
            O.r0[a] = r;
            O.c.pos0[a] = pos0;
        }
        O.g0[a] = base + (int64_t)bl.ref;
        O.g1[a] = base + (int64_t)br.ref;
    }
}

template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void bmv_overlap_decide_kernel(OverlapJob O) {
    const uint32_t a = blockIdx.x * THREADS + threadIdx.x;
    if (a >= O.c.a.count) return;
    const uint32_t b = O.mate[a];
    uint32_t role = kOverlapNone;
    int64_t m = 0;
    if (b != kNoMate && O.l0[a] < O.r0[a] && O.l0[b] < O.r0[b] && (!O.contig || O.contig[a] == O.contig[b])) {
        const int64_t a0 = O.g0[a], b0 = O.g0[b];
        const bool a_first = a0 < b0 || (a0 == b0 && a < b);
        const int64_t f1 = a_first ? O.g1[a] : O.g1[b], s1 = a_first ? O.g1[b] : O.g1[a], s0 = a_first ? b0 : a0;
        const int64_t o = f1 - s0;
        if (f1 <= s1 && o > 0) {
            m = s0 + o / 2;
            role = a_first ? kOverlapFirst : kOverlapSecond;
        }
    }
    O.role[a] = role;
    O.m[a] = m;
}

template <uint32_t WAVES>                                       // alignments per block
__global__ __launch_bounds__(64 * WAVES) void bmv_overlap_restrict_kernel(OverlapJob O) {
    const AnnotateJob &J = O.c.a;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (a >= J.count) return;
    const uint32_t role = O.role[a];
    if (role == kOverlapNone) {
        if (lane == 0) O.found[a] = 0;
        return;
    }
    const uint64_t cig_at = J.cigar_offset[a];
    const uint32_t ne = (uint32_t)(J.cigar_offset[a + 1] - cig_at);
    const uint32_t *cig = J.cigar + cig_at;
    const bool rc = J.text_rc[a] != 0;
    const int64_t l = (int64_t)O.l0[a], r = (int64_t)O.r0[a];
    const int64_t want = O.m[a] - ((int64_t)J.text_start[a] + (int64_t)O.c.pos0[a]);    // m, counted from the first column's g
    const bool first = role == kOverlapFirst;
    // per M entry with columns [s, s + len) and t reference columns before it: g(i) - g(0) = t + i - s, so g < m  <=>
    // i < s + want - t.  first: the greatest such i inside [l, r), as r' = i + 1 (0: none); second: the least i with the
    // opposite, as l' (kept as its complement for a maximum across the wave; 0: none)
    int64_t col = 0, ref = 0;
    uint64_t best = 0;
    for (uint32_t k0 = 0; k0 < ne && col < r; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const uint32_t e = k < ne ? cig[rc ? ne - 1u - k : k] : 0u, op = e & 15u, len = e >> 4;
        const uint64_t incl = overlap_scan((uint64_t)len, lane), incl_t = overlap_scan(op != kOpI ? (uint64_t)len : 0ull, lane);
        const int64_t s = col + (int64_t)(incl - len), t = ref + (int64_t)(incl_t - (op != kOpI ? len : 0u));
        if (op == 0u && len != 0u) {
            const int64_t lo = s > l ? s : l, hi = s + (int64_t)len < r ? s + (int64_t)len : r, lim = s + want - t;
            if (lo < hi) {
                if (first) {
                    const int64_t end = hi < lim ? hi : lim;    // r' for this entry
                    if (end > lo && (uint64_t)end > best) best = (uint64_t)end;
                } else {
                    const int64_t at = lo > lim ? lo : lim;     // l' for this entry
                    if (at < hi && ~(uint64_t)at > best) best = ~(uint64_t)at;
                }
            }
        }
        col += (int64_t)overlap_last(incl);
        ref += (int64_t)overlap_last(incl_t);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t t = (uint64_t)__shfl_xor((long long)best, o, 64);
        best = t > best ? t : best;
    }
    best = clip_uniform(best);
    if (best == 0ull) {
        if (lane == 0) O.found[a] = 0;
        return;
    }
    const uint64_t edge = first ? best : ~best;
    const OverlapCols at = overlap_before(cig, ne, rc, lane, edge);
    const OverlapCols end = overlap_before(cig, ne, rc, lane, first ? (uint64_t)r : (uint64_t)l);
    if (lane == 0) {
        O.found[a] = 1;
        O.edge[a] = edge;
        O.cut_q[a] = (uint32_t)(first ? end.qry - at.qry : at.qry - end.qry);
    }
}

template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void bmv_overlap_commit_kernel(OverlapJob O) {
    const uint32_t a = blockIdx.x * THREADS + threadIdx.x;
    if (a >= O.c.a.count) return;
    uint64_t l = O.l0[a], r = O.r0[a];
    uint32_t cut = 0;
    uint8_t was = 0;
    const uint32_t role = O.role[a];
    if (role != kOverlapNone && O.found[a] != 0u && O.found[O.mate[a]] != 0u) {
        if (role == kOverlapFirst) r = O.edge[a]; else l = O.edge[a];
        cut = O.cut_q[a];
        was = 1;
    }
    O.c.l[a] = l;
    O.c.r[a] = r;
    O.cut[a] = cut;
    O.was_cut[a] = was;
}

// after bmv_clip's count pass: nm[a] counts the X, I and D columns of [l, r)
template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void bmv_overlap_score_kernel(OverlapJob O) {
    const uint32_t a = blockIdx.x * THREADS + threadIdx.x;
    if (a >= O.c.a.count) return;
    const int64_t cols = (int64_t)(O.c.r[a] - O.c.l[a]), nm = (int64_t)O.c.a.nm[a];
    O.c.score[a] = (int64_t)O.c.match * (cols - nm) - (int64_t)O.c.penalty * nm;
}

// instantiated in bmv_overlap.hip
extern template __global__ void bmv_overlap_span_kernel<false>(OverlapJob);
extern template __global__ void bmv_overlap_span_kernel<true>(OverlapJob);
extern template __global__ void bmv_overlap_decide_kernel<kOverlapThreads>(OverlapJob);
extern template __global__ void bmv_overlap_restrict_kernel<kAnnotateWaves>(OverlapJob);
extern template __global__ void bmv_overlap_commit_kernel<kOverlapThreads>(OverlapJob);
extern template __global__ void bmv_overlap_score_kernel<kOverlapThreads>(OverlapJob);

}  // namespace bmv
