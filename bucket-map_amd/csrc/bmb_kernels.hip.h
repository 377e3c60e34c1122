// bmb_kernels.hip.h -- strand and mapping-quality evidence of a BAM record stream and the annotations of variant calls on
// gfx950 (include/bmb.h states the rule).
//
// The state is strand[4 * slot + a], a = A C G T, u64 each (fwd << 32 | rev), 32 bytes = one sector per position, and
// mapq[slot], u64 (n << 40 | S), over the references back to back as in bmg_kernels.hip.h.
//
//   add       bmp's add_records with a third action: the same per-record choice (a short record by its lane alone, every other
//             one by the whole wave).  on() keeps what the record adds -- 1 << 32 or 1 by its strand, (1 << 40) + mapq^2 -- and a
//             base that counts issues TWO no-return 64-bit global atomic adds.  No LDS, no scratch.
//   annotate  one call per wavefront.  The lanes load the call and its position's five cells alike (uniform addresses), and
//             stride the x of Fisher's table: a pass for the largest w (wave max), a pass for the two sums (wave sums); the
//             smallest FS is then a binary search over E, the same in every lane; lane 0 stores the sixteen words.  A single
//             thread per call would walk up to 65 535 x of four dependent table loads each.  Letters select by compares:
//             nothing is indexed by a run-time value.
// No kernel waits for another workgroup.
#pragma once

#include "bmp_walk.hip.h"

namespace bmb {

constexpr uint32_t kThreads = bmp::kThreads, kWaves = kThreads / 64;
constexpr uint32_t kStrandCells = 4, kCallWords = 24, kOutWords = 16;       // BMB_N_STRAND_CELLS, BMB_CALL_WORDS, BMB_OUT_WORDS
constexpr uint32_t kNLf = 65536, kNE = 12001, kFsCap = 6000, kFsMaxN = 65535;
constexpr uint32_t kAnnotated = 1, kNoFs = 2, kVariant = 2;
constexpr uint32_t kTie = 4;                                                // the rounding of four table entries on either side

struct params {
    uint32_t min_mapq, min_bq;
};

// the action of bmp's walkers: a base of sufficient quality and a plain letter adds to its strand cell and to the mapq cell
struct bias_action {
    static constexpr bool kIndels = false, kStats = false;
    unsigned long long *__restrict__ s, *__restrict__ m;
    uint32_t min_bq;
    unsigned long long s_add, m_add;                     // what a base of this record adds to either cell
    __device__ __forceinline__ bias_action on(uint64_t first, uint32_t flag, uint32_t mapq) const {
        return bias_action{s + first * kStrandCells, m + first, min_bq, (flag & 0x10u) ? 1ull : 1ull << 32, (1ull << 40) + (unsigned long long)(mapq * mapq)};
    }
    __device__ __forceinline__ void base(uint64_t position, uint32_t q, uint32_t code) const {
        if (q != bmp::kQualNone && q < min_bq) return;
        const uint32_t letter = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
        if (letter == 4) return;
        atomicAdd(&s[position * kStrandCells + letter], s_add);   // neither result is used: global_atomic_add_x2, no return
        atomicAdd(&m[position], m_add);
    }
    __device__ __forceinline__ void del(uint64_t) const {}
    __device__ __forceinline__ void ins(uint64_t) const {}
};

__global__ __launch_bounds__(kThreads) void add_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                       const uint8_t *__restrict__ skip, const uint32_t *__restrict__ ref_len,
                                                       const uint64_t *__restrict__ ref_base, uint32_t n_ref, params pr,
                                                       unsigned long long *__restrict__ strand, unsigned long long *__restrict__ mapq) {
    bmp::add_records(in, rec_offset, n, skip, ref_len, ref_base, n_ref, pr.min_mapq, bias_action{strand, mapq, pr.min_bq, 0, 0}, nullptr);
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

// floor(sqrt(v)), v < 2^32 (here at most 10000 x 255^2): bit by bit, integers only
__device__ __forceinline__ uint32_t isqrt64(uint64_t v) {
    uint64_t r = 0;
#pragma unroll
    for (int b = 15; b >= 0; b--) {
        const uint64_t t = r | (1ull << b);
        if (t * t <= v) r = t;
    }
    return (uint32_t)r;
}

__device__ __forceinline__ uint32_t pick4(uint32_t k, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) { return k == 0 ? v0 : k == 1 ? v1 : k == 2 ? v2 : v3; }

// out[16 i ..] = the annotation of calls[24 i ..].  The host has checked every VARIANT call's reference, position and
// letters; one that fails the check here all the same reads no cell and is written as sixteen zeros.
__global__ __launch_bounds__(kThreads) void annotate_kernel(const uint32_t *__restrict__ calls, uint64_t n_calls,
                                                            const unsigned long long *__restrict__ strand, const unsigned long long *__restrict__ mapq,
                                                            const uint32_t *__restrict__ ref_len, const uint64_t *__restrict__ ref_base, uint32_t n_ref,
                                                            const uint32_t *__restrict__ LF, const unsigned long long *__restrict__ E,
                                                            uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);   // the same in all lanes of a wave
    if (i >= n_calls) return;
    const uint4 *cp = reinterpret_cast<const uint4 *>(calls + i * kCallWords);   // 96 bytes a call: 16-byte aligned
    const uint4 c0 = cp[0], c1w = cp[1];
    const uint32_t ref = c0.x, pos = c0.y, R = c0.z, flags = c0.w, g0 = c1w.x, g1 = c1w.y;
    uint4 *o = reinterpret_cast<uint4 *>(out + i * kOutWords);                   // 64 bytes an annotation
    if (!(flags & kVariant) || ref >= n_ref || pos >= ref_len[ref] || R > 3 || g0 > 3 || g1 > 3) {
        if (lane == 0) o[0] = o[1] = o[2] = o[3] = make_uint4(0, 0, 0, 0);
        return;
    }
    const uint64_t slot = ref_base[ref] + pos;
    const ulonglong2 *sp = reinterpret_cast<const ulonglong2 *>(strand + slot * kStrandCells);   // 32-byte aligned
    const ulonglong2 lo = sp[0], hi = sp[1];
    const uint64_t mc = mapq[slot];
    const uint32_t f0 = (uint32_t)(lo.x >> 32), f1 = (uint32_t)(lo.y >> 32), f2 = (uint32_t)(hi.x >> 32), f3 = (uint32_t)(hi.y >> 32);
    const uint32_t r0 = (uint32_t)lo.x, r1_ = (uint32_t)lo.y, r2_ = (uint32_t)hi.x, r3 = (uint32_t)hi.y;
    const uint64_t n = mc >> 40, S = mc & ((1ull << 40) - 1);
    const uint32_t mq = n ? isqrt64(10000ull * S / n) : 0u;
    // the table
    const uint64_t a = pick4(R, f0, f1, f2, f3), b = pick4(R, r0, r1_, r2_, r3);
    uint64_t c = 0, d = 0;
    if (g0 != R) c += pick4(g0, f0, f1, f2, f3), d += pick4(g0, r0, r1_, r2_, r3);
    if (g1 != R && g1 != g0) c += pick4(g1, f0, f1, f2, f3), d += pick4(g1, r0, r1_, r2_, r3);
    const uint64_t row1 = a + b, row2 = c + d, col1 = a + c, col2 = b + d;
    uint32_t fs = 0, note = kAnnotated;
    if (row1 + row2 > kFsMaxN || row1 == 0 || row2 == 0 || col1 == 0 || col2 == 0) {
        note |= kNoFs;
    } else {
        // every index below is at most row1 + row2 <= 65 535: inside LF
        const uint32_t R1 = (uint32_t)row1, R2 = (uint32_t)row2, C1 = (uint32_t)col1;
        const uint32_t x_lo = C1 > R2 ? C1 - R2 : 0u, x_hi = R1 < C1 ? R1 : C1;
        auto cost = [&](uint32_t x) { return LF[x] + LF[R1 - x] + LF[C1 - x] + LF[R2 - C1 + x]; };   // -w(x), at most 4 LF[65535] < 2^32
        uint32_t least = 0xFFFFFFFFu;                    // -m: the smallest cost
        for (uint32_t x = x_lo + lane; x <= x_hi; x += 64) {
            const uint32_t v = cost(x);
            least = v < least ? v : least;
        }
        least = wave_min32(least);
        const uint32_t mine = cost((uint32_t)a);         // -w(a); w(x) <= w(a) + 4 is cost(x) + 4 >= cost(a)
        uint64_t s_all = 0, s_ext = 0;
        for (uint32_t x = x_lo + lane; x <= x_hi; x += 64) {
            const uint32_t v = cost(x), k = v - least;
            const uint64_t e = k < kNE ? E[k] : 0ull;
            s_all += e;
            if ((uint64_t)v + kTie >= mine) s_ext += e;
        }
        s_all = wave_sum64(s_all), s_ext = wave_sum64(s_ext);
        // the smallest k in 0 .. 6000 with s_all E[k] <= s_ext 2^40 (E does not grow with k), or 6000
        const uint64_t rhs_hi = s_ext >> 24, rhs_lo = s_ext << 40;
        uint32_t below = 0, top = kFsCap;                // the answer lies in [below, top]
        while (below < top) {
            const uint32_t mid = (below + top) / 2;
            const uint64_t e = E[mid], p_hi = __umul64hi(s_all, e), p_lo = s_all * e;
            if (p_hi < rhs_hi || (p_hi == rhs_hi && p_lo <= rhs_lo)) top = mid;
            else below = mid + 1;
        }
        fs = below;
    }
    if (lane == 0) {
        o[0] = make_uint4(f0, f1, f2, f3);
        o[1] = make_uint4(r0, r1_, r2_, r3);
        o[2] = make_uint4(mq, fs, note, (uint32_t)n);
        o[3] = make_uint4((uint32_t)a, (uint32_t)b, (uint32_t)c, (uint32_t)d);
    }
}

}  // namespace bmb
