// bmg_kernels.hip.h -- quality-weighted allele evidence and diploid genotype calls of a BAM record stream on gfx950
// (include/bmg.h states the rule).
//
// The state is cell[4 * slot + a], a = A C G T, u64 each, over the references back to back as in bmp_kernels.hip.h: 32 bytes =
// one sector per position.  A cell is n << 32 | Q.
//
//   add   bmp's add_records with another action: the same per-record choice (a short record by its lane alone, every other
//         one by the whole wave with aligned quality and sequence words), and at a base that counts ONE no-return 64-bit
//         global atomic add of (1 << 32) + q_eff, which carries the count and the quality sum together.  Deletions,
//         insertions and the per-reference sums are not its business: the walkers leave those loops out.
//   call  one thread per site: three 16-byte loads of the site, one position's 32 bytes of cells as two 16-byte loads, the
//         ten costs in u64 registers, six 16-byte stores.  No atomics.
// No kernel waits for another workgroup.
#pragma once

#include "bmg_rule.hip.h"
#include "bmp_walk.hip.h"

namespace bmg {

constexpr uint32_t kThreads = bmp::kThreads;
constexpr uint32_t kSiteWords = 12, kCallWords = 24;     // BMG_SITE_WORDS, BMG_CALL_WORDS
constexpr uint32_t kGenotyped = 1, kVariant = 2, kKindSnv = 1;

// the action of bmp's walkers: a base of sufficient quality and a plain letter adds its count and its quality in one atomic
struct cell_action {
    static constexpr bool kIndels = false, kStats = false;
    unsigned long long *__restrict__ c;
    uint32_t min_bq, q_absent, q_cap;
    __device__ __forceinline__ cell_action on(uint64_t first, uint32_t, uint32_t) const { return cell_action{c + first * kCells, min_bq, q_absent, q_cap}; }
    __device__ __forceinline__ void base(uint64_t position, uint32_t q, uint32_t code) const {
        if (q != bmp::kQualNone && q < min_bq) return;
        const uint32_t letter = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
        if (letter == 4) return;
        const uint32_t q_eff = q == bmp::kQualNone ? q_absent : (q < q_cap ? q : q_cap);
        atomicAdd(&c[position * kCells + letter], (1ull << 32) + q_eff);   // the result is not used: global_atomic_add_x2, no return
    }
    __device__ __forceinline__ void del(uint64_t) const {}
    __device__ __forceinline__ void ins(uint64_t) const {}
};

__global__ __launch_bounds__(kThreads) void add_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                       const uint8_t *__restrict__ skip, const uint32_t *__restrict__ ref_len,
                                                       const uint64_t *__restrict__ ref_base, uint32_t n_ref, params pr,
                                                       unsigned long long *__restrict__ cell) {
    bmp::add_records(in, rec_offset, n, skip, ref_len, ref_base, n_ref, pr.min_mapq, cell_action{cell, pr.min_bq, pr.q_absent, pr.q_cap}, nullptr);
}

// out[24 i ..] = the call of sites[12 i ..] from the cells.  The host has checked every site's reference and position; a
// site that fails the check here all the same reads no cell and is written as not genotyped with n = 0.
__global__ __launch_bounds__(kThreads) void call_kernel(const uint32_t *__restrict__ sites, uint64_t n_sites, const unsigned long long *__restrict__ cell,
                                                        const uint32_t *__restrict__ ref_len, const uint64_t *__restrict__ ref_base, uint32_t n_ref,
                                                        uint32_t prior, uint32_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_sites) return;
    const uint4 *sp = reinterpret_cast<const uint4 *>(sites + i * kSiteWords);   // 48 bytes a site: 16-byte aligned
    const uint4 s0 = sp[0], s2 = sp[2];
    const uint32_t ref = s0.x, pos = s0.y, R = s0.z, kind = s2.w;
    uint64_t n[4] = {0, 0, 0, 0}, Q[4] = {0, 0, 0, 0};
    if (ref < n_ref && pos < ref_len[ref]) {
        const ulonglong2 *cp = reinterpret_cast<const ulonglong2 *>(cell + (ref_base[ref] + pos) * kCells);   // 32-byte aligned
        const ulonglong2 lo = cp[0], hi = cp[1];
        const uint64_t v[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
        for (uint32_t a = 0; a < 4; a++) n[a] = v[a] >> 32, Q[a] = v[a] & kU32Max;
    }
    const uint64_t depth = n[0] + n[1] + n[2] + n[3];
    uint4 *o = reinterpret_cast<uint4 *>(out + i * kCallWords);                  // 96 bytes a call: 16-byte aligned
    if (!(kind & kKindSnv) || R > 3 || depth == 0) {
        o[0] = make_uint4(ref, pos, R, 0);
        o[1] = make_uint4(0, 0, 0, 0);
        o[2] = make_uint4((uint32_t)n[0], (uint32_t)n[1], (uint32_t)n[2], (uint32_t)n[3]);
        o[3] = o[4] = o[5] = make_uint4(0, 0, 0, 0);
        return;
    }
    uint64_t L[kGenotypes];
    costs(n, Q, R, prior, L);
    uint64_t least = 0, l_rr = 0;                        // tracked in registers: L is only ever indexed by unrolled counters
    uint32_t k = 0, best = 0, best_a = 0, best_b = 0, k_rr = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; b++)
#pragma unroll
        for (uint32_t a = 0; a <= b; a++, k++) {
            if (a == R && b == R) k_rr = k, l_rr = L[k];
            if (k == 0 || L[k] < least) least = L[k], best = k, best_a = a, best_b = b;   // the smallest k among equals
        }
    if (l_rr == least) best = k_rr, best_a = best_b = R;  // a tie goes to RR
    uint64_t second = ~0ull;
#pragma unroll
    for (uint32_t g = 0; g < kGenotypes; g++)
        if (g != best && L[g] < second) second = L[g];
    const uint64_t gq = (second - least) / 100u;
    uint32_t pl[kGenotypes];
#pragma unroll
    for (uint32_t g = 0; g < kGenotypes; g++) pl[g] = sat32(L[g] - least);
    o[0] = make_uint4(ref, pos, R, kGenotyped | (best != k_rr ? kVariant : 0u));
    o[1] = make_uint4(best_a, best_b, gq > 99 ? 99u : (uint32_t)gq, sat32(l_rr - least));
    o[2] = make_uint4((uint32_t)n[0], (uint32_t)n[1], (uint32_t)n[2], (uint32_t)n[3]);
    o[3] = make_uint4(pl[0], pl[1], pl[2], pl[3]);
    o[4] = make_uint4(pl[4], pl[5], pl[6], pl[7]);
    o[5] = make_uint4(pl[8], pl[9], sat32(depth), 0);
}

}  // namespace bmg
