// bmr_kernels.hip.h -- reference-confidence blocks over the cells of the genotype caller on gfx950 (include/bmr.h states the
// rule).
//
// The state beside bmg's cells, over the references back to back: base[p] (the reference byte), st[p] and dp[p] (the two
// words of the per-position view, apart so that the passes after the first read 4 bytes where they need 4), flag[p] (1 at the
// first position of a block) and rank[p] (the exclusive prefix sum of flag, n + 1 values: rank[n] is the number of blocks).
//
//   conf     four consecutive positions per thread: their 128 bytes of cells as eight 16-byte loads, four reference bytes as
//            one word, bmg::costs with the prior 0 in u64 registers, st and dp as one 16-byte store each.  The bounds are a
//            kernel argument and indexed by an unrolled counter only.
//   exclude  one thread per EXCLUDED POSITION, not per interval: the host's prefix sum over the interval lengths says where
//            thread t lies, by bisection.  Intervals that overlap stamp the same word with the same value.
//   heads    four positions per thread: flag = IN and (st >> 8) other than the predecessor's.  ref_heads then sets the flag
//            at the first base of every reference that is IN.  bm_scan ranks the flags.
//   fill     the block records' minima at 2^32 - 1 and their sums at 0.
//   blocks   one position per lane, kPerLane trips: the head of a block writes its reference (by bisection over the
//            reference starts), start and band, its last position the end; min_gq, min_dp and sum_dp are reduced inside the
//            wave by segmented shuffles, the segment that reaches lane 63 is carried into the next trip, and what is left
//            goes to the record with no-return atomics: at most one set per (wave, block), whatever the block's length.
// No kernel waits for another workgroup.  n is 64-bit in every index.
#pragma once

#include "bmg_rule.hip.h"

namespace bmr {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kQuad = 4;                            // positions per thread in conf and heads
constexpr uint32_t kPerLane = 16;                        // trips of a wave in blocks: 1 024 positions per wave
constexpr uint32_t kMaxBands = 16, kBlockWords = 8;      // BMR_MAX_BANDS, BMR_BLOCK_WORDS
constexpr uint32_t kIn = 1u << 16, kExcluded = 1u << 17, kNoAllele = 1u << 18;
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct bounds {
    uint32_t b[kMaxBands];                               // the unused ones are 2^32 - 1: no gq reaches them
};

__device__ __forceinline__ uint32_t letter_of(uint32_t byte) {
    const uint32_t c = byte & 0xDFu;                     // either case
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

// st, dp and base hold a multiple of kQuad elements (the host sizes them so); cell holds n positions and is read below n only
__global__ __launch_bounds__(kThreads) void conf_kernel(const unsigned long long *__restrict__ cell, const uint8_t *__restrict__ base, uint64_t n,
                                                        bounds bd, uint32_t *__restrict__ st, uint32_t *__restrict__ dp) {
    const uint64_t p0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (p0 >= n) return;
    const uint32_t four = *reinterpret_cast<const uint32_t *>(base + p0);
    uint32_t s[kQuad], d[kQuad];
#pragma unroll
    for (uint32_t j = 0; j < kQuad; j++) {
        s[j] = d[j] = 0;
        if (p0 + j >= n) continue;
        const ulonglong2 *cp = reinterpret_cast<const ulonglong2 *>(cell + (p0 + j) * bmg::kCells);   // 32-byte aligned
        const ulonglong2 lo = cp[0], hi = cp[1];
        const uint64_t v[4] = {lo.x, lo.y, hi.x, hi.y};
        uint64_t cnt[4], Q[4];
#pragma unroll
        for (uint32_t a = 0; a < 4; a++) cnt[a] = v[a] >> 32, Q[a] = v[a] & bmg::kU32Max;
        d[j] = bmg::sat32(cnt[0] + cnt[1] + cnt[2] + cnt[3]);
        const uint32_t R = letter_of((four >> (8 * j)) & 0xFFu);
        if (R > 3) {
            s[j] = kNoAllele;
            continue;
        }
        uint64_t L[bmg::kGenotypes];
        bmg::costs(cnt, Q, R, 0u, L);
        uint64_t l_rr = 0, h = ~0ull;
        uint32_t k = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
#pragma unroll
            for (uint32_t a = 0; a <= b; a++, k++) {
                if (a == R && b == R) l_rr = L[k];
                else if (L[k] < h) h = L[k];
            }
        uint32_t gq = 0;
        if (l_rr <= h) {
            const uint64_t diff = h - l_rr;
            gq = diff >= 9900u ? 99u : (uint32_t)diff / 100u;
        }
        uint32_t band = 0;
#pragma unroll
        for (uint32_t i = 0; i < kMaxBands; i++) band += bd.b[i] <= gq ? 1u : 0u;
        s[j] = gq | band << 8 | kIn;
    }
    *reinterpret_cast<uint4 *>(st + p0) = make_uint4(s[0], s[1], s[2], s[3]);
    *reinterpret_cast<uint4 *>(dp + p0) = make_uint4(d[0], d[1], d[2], d[3]);
}

// thread t stamps the t-th excluded position, counted over the intervals in the order given: interval i holds
// t in [before[i], before[i + 1]) and begins at the slot first[i]
__global__ __launch_bounds__(kThreads) void exclude_kernel(const uint64_t *__restrict__ first, const uint64_t *__restrict__ before, uint64_t n_exclude,
                                                           uint64_t total, uint64_t n, uint32_t *__restrict__ st) {
    const uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= total) return;
    uint64_t lo = 0, hi = n_exclude;                     // before[lo] <= t < before[hi]
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (before[mid] <= t) lo = mid;
        else hi = mid;
    }
    const uint64_t p = first[lo] + (t - before[lo]);
    if (p < n) st[p] = kExcluded;
}

__global__ __launch_bounds__(kThreads) void heads_kernel(const uint32_t *__restrict__ st, uint64_t n, uint32_t *__restrict__ flag) {
    const uint64_t p0 = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * kQuad;
    if (p0 >= n) return;
    const uint4 q = *reinterpret_cast<const uint4 *>(st + p0);
    const uint32_t s[kQuad] = {q.x, q.y, q.z, q.w};
    uint32_t before = p0 ? st[p0 - 1] : 0u;              // 0 is no state at all: position 0 is a head if it is IN
    uint32_t f[kQuad];
#pragma unroll
    for (uint32_t j = 0; j < kQuad; j++) {
        f[j] = p0 + j < n && (s[j] & kIn) && (s[j] >> 8) != (before >> 8) ? 1u : 0u;
        before = s[j];
    }
    *reinterpret_cast<uint4 *>(flag + p0) = make_uint4(f[0], f[1], f[2], f[3]);
}

__global__ __launch_bounds__(kThreads) void ref_heads_kernel(const uint64_t *__restrict__ ref_base, uint32_t n_ref, const uint32_t *__restrict__ st,
                                                             uint32_t *__restrict__ flag) {
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_ref) return;
    const uint64_t p = ref_base[r];
    if (st[p] & kIn) flag[p] = 1u;
}

__global__ __launch_bounds__(kThreads) void fill_kernel(uint32_t *__restrict__ blk, uint64_t n_blocks) {
    const uint64_t b = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= n_blocks) return;
    uint4 *o = reinterpret_cast<uint4 *>(blk + b * kBlockWords);
    o[0] = make_uint4(0, 0, 0, 0);
    o[1] = make_uint4(kNone, kNone, 0, 0);
}

// the reference that holds slot p: ref_base[r] <= p < ref_base[r + 1]
__device__ __forceinline__ uint32_t ref_of(const uint64_t *__restrict__ ref_base, uint32_t n_ref, uint64_t p) {
    uint32_t lo = 0, hi = n_ref;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ref_base[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void flush(uint32_t *__restrict__ blk, uint32_t b, uint32_t gq, uint32_t dp, unsigned long long sum) {
    uint32_t *o = blk + (uint64_t)b * kBlockWords;
    atomicMin(o + 4, gq);                                // the results are not used: no-return atomics
    atomicMin(o + 5, dp);
    atomicAdd(reinterpret_cast<unsigned long long *>(o + 6), sum);   // 8-byte aligned: a record is 32 bytes
}

__global__ __launch_bounds__(kThreads) void blocks_kernel(const uint32_t *__restrict__ st, const uint32_t *__restrict__ dp, const uint32_t *__restrict__ flag,
                                                          const uint32_t *__restrict__ rank, uint64_t n, const uint64_t *__restrict__ ref_base,
                                                          uint32_t n_ref, uint32_t *__restrict__ blk) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    const uint64_t c0 = wave * (64ull * kPerLane);
    uint32_t cb = kNone, cgq = kNone, cdp = kNone;       // the segment carried from the trip before: the same in every lane
    unsigned long long csum = 0;
    for (uint32_t j = 0; j < kPerLane; j++) {
        if (c0 + 64ull * j >= n) break;                  // the same for the whole wave
        const uint64_t p = c0 + 64ull * j + lane;
        uint32_t b = kNone, gq = kNone, d = kNone, s = 0, f = 0;
        unsigned long long sum = 0;
        if (p < n) {
            s = st[p];
            if (s & kIn) {
                f = flag[p];
                b = rank[p] + f - 1u;                    // the heads before p, and p's own
                gq = s & 0xFFu;
                d = dp[p];
                sum = d;
            }
        }
        const uint32_t mine = b;
        // the last position of a block: the next is another block's, or none's
        uint32_t next = __shfl_down(mine, 1, 64);
        if (lane == 63) {
            next = kNone;
            if (p + 1 < n && (st[p + 1] & kIn) && !flag[p + 1]) next = mine;
        }
        if (mine != kNone && (f || next != mine)) {
            const uint32_t r = ref_of(ref_base, n_ref, p);
            uint32_t *o = blk + (uint64_t)mine * kBlockWords;
            if (f) o[0] = r, o[1] = (uint32_t)(p - ref_base[r]), o[3] = (s >> 8) & 0xFFu;
            if (next != mine) o[2] = (uint32_t)(p - ref_base[r]) + 1u;
        }
        // each lane gathers what its segment holds from its own lane upwards: equal b are side by side
#pragma unroll
        for (uint32_t o = 1; o < 64; o <<= 1) {
            const uint32_t ob = __shfl_down(mine, o, 64), og = __shfl_down(gq, o, 64), od = __shfl_down(d, o, 64);
            const unsigned long long os = __shfl_down(sum, o, 64);
            if (lane + o < 64 && ob == mine) {
                gq = og < gq ? og : gq;
                d = od < d ? od : d;
                sum += os;
            }
        }
        const uint32_t prev = __shfl_up(mine, 1, 64);
        const bool leader = lane == 0 || prev != mine;
        if (lane == 0) {
            if (cb == mine) {
                gq = cgq < gq ? cgq : gq;
                d = cdp < d ? cdp : d;
                sum += csum;
            } else if (cb != kNone) {
                flush(blk, cb, cgq, cdp, csum);
            }
        }
        const uint32_t last = __shfl(mine, 63, 64);
        if (leader && mine != kNone && mine != last) flush(blk, mine, gq, d, sum);
        // the segment that reaches lane 63 goes on into the next trip
        const uint64_t same = __ballot(mine == last);
        const int first_lane = __ffsll((unsigned long long)same) - 1;
        cb = last;
        cgq = __shfl(gq, first_lane, 64);
        cdp = __shfl(d, first_lane, 64);
        csum = __shfl(sum, first_lane, 64);
    }
    if (lane == 0 && cb != kNone) flush(blk, cb, cgq, cdp, csum);
}

}  // namespace bmr
