// bmc_kernels.hip.h -- per-base depth of a BAM record stream on gfx950 (include/bmc.h states the rule).
//
// The state is one u32 difference array `diff` over the references back to back, reference r at ref_base[r] with
// ref_len[r] + 1 slots: a clipped block [s, e) adds +1 at s and -1 at e, and e <= ref_len[r] falls into r's own extra slot,
// so every reference's differences sum to zero and one scan runs straight across the borders.
//
//   blocks      one LANE per record, chosen per record: a counted record of at most kShortOps ops and kShortSeq bases is
//               walked by its lane alone (a million 1-op short reads cost a 64th of a wave each); every other counted record
//               of the wave is then walked by the whole wave, one after the other: the lanes stride over the ops, the two
//               cursors are a carried wave scan, each lane adds its own block, and a block of 64 bases or more has its quality
//               bytes summed by all lanes in aligned 4-byte words.  Adjacent blocks (= next to X) share a border whose -1 and
//               +1 cancel: neither is issued.  32-bit global atomic adds: integer sums, so their order does not matter.
//               n_reads, sum_mapq, sum_qual, n_qual and n_long are summed over the wave's lanes of equal reference first: one
//               atomic per (wave, reference, value), not per record.
//   runs_count  after bmscan::exclusive_sum (depth[i + 1] is the depth of slot i; arithmetic mod 2^32 is exact, depth <=
//               records < 2^32): per tile of kTile slots the run starts (depth > 0 and other than the slot before), and per
//               reference cov_bases and sum_depth -- one pair of atomics per tile, the reference found by bisection of
//               ref_base; a tile that holds a border falls back to per-thread sums.
//   runs_emit   the same tiles with the scanned tile counts: the k-th run start in place order writes (reference, start,
//               depth) of run k, the run end that follows it -- the slot where a depth > 0 changes -- writes run k's end;
//               ranks, not atomics, place every value.
// No kernel waits for another workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm_scan.hip.h"

namespace bmc {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kShortOps = 8, kShortSeq = 512;       // blocks: what one lane walks alone
constexpr uint32_t kWideSpan = 64;                       // blocks: quality bytes of a block from which the wave shares them
constexpr uint32_t kItems = bmscan::kItems, kTile = bmscan::kTile;
constexpr uint32_t kStats = 7;                           // BMC_N_STATS; n_reads cov_bases sum_depth sum_mapq sum_qual n_qual n_long
constexpr uint32_t kSkipFlags = 0x4u | 0x100u | 0x200u | 0x400u, kQualNone = 0xFF;
static_assert(kThreads == (uint32_t)bmscan::kThreads, "the run passes use the scan's block reduction");

__device__ __forceinline__ uint32_t load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint32_t load16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ bool is_block(uint32_t op) { return op == 0 || op == 7 || op == 8; }
__device__ __forceinline__ bool takes_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
__device__ __forceinline__ bool takes_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

// quality bytes p[0, len) that are not 0xFF, by all lanes in aligned words.  A word may reach up to 3 bytes before p (the
// same record) and behind p + len (the stream's buffer has 16 bytes of room behind its end); those bytes are masked out.
__device__ __forceinline__ void span_sum(const uint8_t *p, uint64_t len, uint32_t lane, uint64_t &sum, uint64_t &count) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = a + len;
    for (uintptr_t w = (a & ~uintptr_t{3}) + 4u * lane; w < b; w += 4u * 64u) {
        const uint32_t x = *reinterpret_cast<const uint32_t *>(w);
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t q = (x >> (8 * j)) & 255u;
            const bool ok = w + j >= a && w + j < b && q != kQualNone;
            sum += ok ? q : 0u;
            count += ok ? 1u : 0u;
        }
    }
}

// one counted record by its lane alone: at most kShortOps ops, at most kShortSeq bases
__device__ __forceinline__ void walk_alone(const uint8_t *cigar, uint32_t n_cigar, const uint8_t *qual, uint32_t l_seq, uint32_t pos, uint32_t rlen,
                                           uint32_t *__restrict__ d, uint64_t &sum_q, uint64_t &n_q) {
    constexpr uint64_t kNone = ~uint64_t{0};
    uint64_t rc = pos, qc = 0, pending = kNone;          // pending: the -1 of the block before, not yet added
    uint32_t sum = 0, count = 0;
    for (uint32_t k = 0; k < n_cigar; k++) {
        const uint32_t c = load32(cigar + 4ull * k), op = c & 15u, len = c >> 4;
        if (is_block(op) && len && rc < rlen) {
            const uint64_t e = rc + len < rlen ? rc + len : rlen;
            if (pending == rc) {
                // the block before ends where this one starts: -1 and +1 cancel
            } else {
                if (pending != kNone) atomicAdd(&d[pending], 0xFFFFFFFFu);
                atomicAdd(&d[rc], 1u);
            }
            pending = e;
            if (l_seq)
                for (uint64_t j = 0; j < e - rc; j++) {  // qc + (e - rc) <= l_seq: the host has checked the query length
                    const uint32_t q = qual[qc + j];
                    sum += q != kQualNone ? q : 0u;
                    count += q != kQualNone ? 1u : 0u;
                }
        }
        if (takes_ref(op)) rc += len;
        if (takes_query(op)) qc += len;
    }
    if (pending != kNone) atomicAdd(&d[pending], 0xFFFFFFFFu);
    sum_q = sum, n_q = count;
}

// one counted record by the whole wave (every argument is the same in all lanes); the sums come back in every lane
__device__ __forceinline__ void walk_wave(const uint8_t *cigar, uint32_t n_cigar, const uint8_t *qual, uint32_t l_seq, uint32_t pos, uint32_t rlen,
                                          uint32_t *__restrict__ d, uint32_t lane, uint64_t &sum_q, uint64_t &n_q) {
    uint64_t rc = pos, qc = 0, sum = 0, count = 0;
    for (uint32_t c0 = 0; c0 < n_cigar; c0 += 64) {      // the same trips in every lane: shuffles below
        const uint32_t k = c0 + lane;
        uint32_t op = 15, len = 0;
        if (k < n_cigar) {
            const uint32_t c = load32(cigar + 4ull * k);
            op = c & 15u, len = c >> 4;
        }
        const uint64_t r_adv = takes_ref(op) ? len : 0u, q_adv = takes_query(op) ? len : 0u;
        const uint64_t r_incl = bmscan::wave_inclusive<uint64_t>(r_adv, lane), q_incl = bmscan::wave_inclusive<uint64_t>(q_adv, lane);
        const uint64_t s = rc + r_incl - r_adv, q0 = qc + q_incl - q_adv;
        const bool has = is_block(op) && len && s < rlen;
        const uint64_t e = has ? (s + len < rlen ? s + len : rlen) : s;
        // op k + 1 starts at s + len: where that is a block too and lies on the reference, this -1 and its +1 cancel
        const bool next_has = __shfl_down((int)has, 1, 64) && lane < 63;
        const bool no_minus = has && next_has && s + len < rlen;
        const bool no_plus = __shfl_up((int)no_minus, 1, 64) && lane > 0;
        if (has && !no_plus) atomicAdd(&d[s], 1u);
        if (has && !no_minus) atomicAdd(&d[e], 0xFFFFFFFFu);
        if (l_seq) {                                     // uniform
            const uint64_t span = e - s;                 // q0 + span <= l_seq: the host has checked the query length
            if (span && span < kWideSpan)
                for (uint64_t j = 0; j < span; j++) {
                    const uint32_t q = qual[q0 + j];
                    sum += q != kQualNone ? q : 0u;
                    count += q != kQualNone ? 1u : 0u;
                }
            uint64_t wide = __ballot(span >= kWideSpan);
            while (wide) {
                const int src = __ffsll((unsigned long long)wide) - 1;
                wide &= wide - 1;
                const uint64_t at = __shfl(q0, src, 64), n = __shfl(span, src, 64);
                span_sum(qual + at, n, lane, sum, count);
            }
        }
        rc += __shfl(r_incl, 63, 64);
        qc += __shfl(q_incl, 63, 64);
    }
    sum_q = wave_sum64(sum);
    n_q = wave_sum64(count);
}

// diff += the blocks of the counted records, stats += n_reads, sum_mapq, sum_qual, n_qual, n_long.  `in` has 16 bytes of
// room behind n_bytes; the fields of a record fit its extent, ops are 0 .. 8, the query length is l_seq (host checks).
__global__ __launch_bounds__(kThreads) void blocks_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                          const uint8_t *__restrict__ skip, const uint32_t *__restrict__ ref_len,
                                                          const uint64_t *__restrict__ ref_base, uint32_t n_ref, uint32_t *__restrict__ diff,
                                                          unsigned long long *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x, wave_first = i - lane;
    bool placed = false, counted = false, wide = false;
    uint32_t ref = 0, mapq = 0;
    uint64_t sum_q = 0, n_q = 0;
    if (i < n) {
        const uint8_t *r = in + rec_offset[i];
        const int32_t ref_i = (int32_t)load32(r + 4), pos_i = (int32_t)load32(r + 8);
        const uint32_t l_name = r[12], n_cigar = load16(r + 16), flag = load16(r + 18), l_seq = load32(r + 20);
        placed = !(flag & kSkipFlags) && !(skip && skip[i]) && ref_i >= 0 && (uint32_t)ref_i < n_ref && pos_i >= 0 && n_cigar > 0;
        uint32_t rlen = 0;
        if (placed) {
            ref = (uint32_t)ref_i;
            rlen = ref_len[ref];
            placed = (uint32_t)pos_i < rlen;
        }
        if (placed) {
            const uint8_t *cigar = r + 36 + l_name;
            counted = !(n_cigar == 2 && load32(cigar) == (l_seq << 4 | 4u) && (load32(cigar + 4) & 15u) == 3u);   // the long-CIGAR placeholder
            mapq = r[13];
            wide = counted && (n_cigar > kShortOps || l_seq > kShortSeq);
            if (counted && !wide)
                walk_alone(cigar, n_cigar, cigar + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2, l_seq, (uint32_t)pos_i, rlen, diff + ref_base[ref], sum_q,
                           n_q);
        }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {                                       // the wave's other counted records, by all lanes
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint8_t *r = in + rec_offset[wave_first + src];
        const uint32_t w_ref = load32(r + 4), w_pos = load32(r + 8), l_name = r[12], n_cigar = load16(r + 16), l_seq = load32(r + 20);
        const uint8_t *cigar = r + 36 + l_name;
        uint64_t s = 0, c = 0;
        walk_wave(cigar, n_cigar, cigar + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2, l_seq, w_pos, ref_len[w_ref], diff + ref_base[w_ref], lane, s, c);
        if ((int)lane == src) sum_q = s, n_q = c;
    }
    uint64_t left = __ballot(placed);
    while (left) {                                       // per reference among the wave's lanes: one atomic per value
        const int src = __ffsll((unsigned long long)left) - 1;
        const uint32_t r0 = __shfl(ref, src, 64);
        const bool mine = placed && ref == r0;
        left &= ~__ballot(mine);
        const uint32_t reads = wave_sum32(mine && counted ? 1u : 0u), mq = wave_sum32(mine && counted ? mapq : 0u);
        const uint32_t n_long = wave_sum32(mine && !counted ? 1u : 0u);
        const uint64_t sq = wave_sum64(mine ? sum_q : 0u), nq = wave_sum64(mine ? n_q : 0u);
        if ((int)lane == src) {
            unsigned long long *st = stats + (uint64_t)r0 * kStats;
            if (reads) atomicAdd(&st[0], (unsigned long long)reads);
            if (mq) atomicAdd(&st[3], (unsigned long long)mq);
            if (sq) atomicAdd(&st[4], (unsigned long long)sq);
            if (nq) atomicAdd(&st[5], (unsigned long long)nq);
            if (n_long) atomicAdd(&st[6], (unsigned long long)n_long);
        }
    }
}

// the reference that holds slot: ref_base[r] <= slot < ref_base[r + 1] (slot < ref_base[n_ref])
__device__ __forceinline__ uint32_t ref_of(const uint64_t *__restrict__ ref_base, uint32_t n_ref, uint64_t slot) {
    uint32_t a = 0, b = n_ref;
    while (b - a > 1) {
        const uint32_t m = a + (b - a) / 2;
        if (ref_base[m] <= slot) a = m; else b = m;
    }
    return a;
}

// d[j] = depth of slot base + j - 1 (d[0]: the slot before; depth[0] = 0 stands before slot 0), 0 beyond the last slot
__device__ __forceinline__ void load_depths(const uint32_t *__restrict__ depth, uint64_t n_slots, uint64_t base, uint32_t (&d)[kItems + 1]) {
#pragma unroll
    for (uint32_t j = 0; j <= kItems; j++) d[j] = base + j <= n_slots ? depth[base + j] : 0u;
}

__global__ __launch_bounds__(kThreads) void runs_count_kernel(const uint32_t *__restrict__ depth, uint64_t n_slots,
                                                              const uint64_t *__restrict__ ref_base, uint32_t n_ref,
                                                              uint32_t *__restrict__ tile_count, unsigned long long *__restrict__ stats) {
    __shared__ uint32_t ws32[kThreads / 64 + 1];
    __shared__ uint64_t ws64[kThreads / 64 + 1];
    __shared__ uint32_t s_ref[2];
    const uint64_t tile0 = (uint64_t)blockIdx.x * kTile, base = tile0 + (uint64_t)threadIdx.x * kItems;
    if (threadIdx.x == 0) {
        const uint64_t last = tile0 + kTile < n_slots ? tile0 + kTile - 1 : n_slots - 1;
        s_ref[0] = ref_of(ref_base, n_ref, tile0);
        s_ref[1] = ref_of(ref_base, n_ref, last);
    }
    uint32_t d[kItems + 1];
    load_depths(depth, n_slots, base, d);
    uint32_t starts = 0, cov = 0;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kItems; j++) {
        const bool in = base + j < n_slots;
        starts += in && d[j + 1] > 0 && d[j + 1] != d[j];
        cov += in && d[j + 1] > 0;
        sum += in ? d[j + 1] : 0u;
    }
    uint32_t all_starts, all_cov;
    uint64_t all_sum;
    (void)bmscan::block_inclusive<uint32_t>(starts, ws32, &all_starts);   // its barriers also publish s_ref
    (void)bmscan::block_inclusive<uint32_t>(cov, ws32, &all_cov);
    (void)bmscan::block_inclusive<uint64_t>(sum, ws64, &all_sum);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = all_starts;
    const uint32_t r_first = s_ref[0], r_last = s_ref[1];
    if (r_first == r_last) {                             // the whole tile on one reference
        if (threadIdx.x == 0 && all_cov) {
            atomicAdd(&stats[(uint64_t)r_first * kStats + 1], (unsigned long long)all_cov);
            atomicAdd(&stats[(uint64_t)r_first * kStats + 2], (unsigned long long)all_sum);
        }
        return;
    }
    if (cov == 0 || base >= n_slots) return;             // a border in the tile: every thread for itself
    uint32_t r = ref_of(ref_base, n_ref, base);
    uint64_t next = ref_base[r + 1], c = 0, s = 0;
    for (uint32_t j = 0; j < kItems && base + j < n_slots; j++) {
        while (base + j >= next) {                       // r + 1 < n_ref here: the slot lies below ref_base[n_ref]
            if (c) {
                atomicAdd(&stats[(uint64_t)r * kStats + 1], (unsigned long long)c);
                atomicAdd(&stats[(uint64_t)r * kStats + 2], (unsigned long long)s);
            }
            c = s = 0;
            r++;
            next = ref_base[r + 1];
        }
        c += d[j + 1] > 0;
        s += d[j + 1];
    }
    if (c) {
        atomicAdd(&stats[(uint64_t)r * kStats + 1], (unsigned long long)c);
        atomicAdd(&stats[(uint64_t)r * kStats + 2], (unsigned long long)s);
    }
}

// runs[4 k ..] = (reference, start, end, depth) of the k-th run in place order; tile_rank = the exclusive sums of tile_count
__global__ __launch_bounds__(kThreads) void runs_emit_kernel(const uint32_t *__restrict__ depth, uint64_t n_slots, const uint64_t *__restrict__ ref_base,
                                                             uint32_t n_ref, const uint32_t *__restrict__ tile_rank, uint32_t n_runs,
                                                             uint32_t *__restrict__ runs) {
    __shared__ uint32_t ws32[kThreads / 64 + 1];
    const uint64_t base = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    uint32_t d[kItems + 1];
    load_depths(depth, n_slots, base, d);
    uint32_t starts = 0;
#pragma unroll
    for (uint32_t j = 0; j < kItems; j++) starts += base + j < n_slots && d[j + 1] > 0 && d[j + 1] != d[j];
    uint32_t all;
    uint32_t rank = bmscan::block_inclusive<uint32_t>(starts, ws32, &all) - starts + tile_rank[blockIdx.x];   // run starts before this thread's slots
    uint32_t r = 0;
    bool have_r = false;
    for (uint32_t j = 0; j < kItems && base + j < n_slots; j++) {
        const uint32_t before = d[j], now = d[j + 1];
        if (now == before) continue;
        const uint64_t slot = base + j;
        if (!have_r) r = ref_of(ref_base, n_ref, slot), have_r = true;
        while (slot >= ref_base[r + 1]) r++;
        const uint32_t at = (uint32_t)(slot - ref_base[r]);
        // a run that is open before this slot is the last one started: it lies on this reference, whose extra slot has depth 0
        if (before > 0 && rank > 0 && rank - 1 < n_runs) runs[4ull * (rank - 1) + 2] = at;
        if (now > 0) {
            if (rank < n_runs) {                         // always; keeps a wrong scan from becoming a wild store
                runs[4ull * rank] = r;
                runs[4ull * rank + 1] = at;
                runs[4ull * rank + 3] = now;
            }
            rank++;
        }
    }
}

}  // namespace bmc
