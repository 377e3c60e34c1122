// bmp_kernels.hip.h -- per-base allele counts and variant sites of a BAM record stream on gfx950 (include/bmp.h states the
// rule).
//
// The state is counter-major: cnt[8 * slot + k], k = A C G T N DEL INS LOWQ, over the references back to back (reference r at
// ref_base[r], ref_len[r] slots: no extra slot, nothing is added beyond a reference's end), 32 bytes = one sector per
// position, and ref[slot], the reference's byte.
//
//   add         one LANE per record, chosen per record as in bmc_kernels.hip.h: a counted record of at most kShortOps ops,
//               kShortSeq bases and kShortSeq deleted positions is walked by its lane alone (a million 1-op short reads
//               cost a 64th of a wave each; the 64 lanes' byte loads run side by side); every other counted record of the
//               wave is then walked by the whole wave, one after the other: the lanes stride over the ops, the two cursors
//               and "an M, =, X or D came before" are a wave scan and a ballot carried from trip to trip, a lane adds its
//               own op where that spans fewer than kWideSpan positions, and every longer block or deletion is shared by
//               the wave: a lane takes the four bases of one ALIGNED 4-byte word of qualities, and their nibbles from the
//               two aligned words of packed sequence that hold them (shifted by the byte and the odd or even query index,
//               so an odd query offset after 3S or an odd I reads the right nibble).  Every count is a no-return 32-bit
//               global atomic add: integer sums, so their order does not matter.  n_reads, n_low_mapq and n_left_out
//               are summed over the wave's lanes of equal reference first: one atomic per (wave, reference, value).
//   sites_count per tile of kTile positions (a thread has kItems consecutive ones: two 16-byte loads per position, one
//               8-byte load of reference bytes): the sites, and per reference n_bases, n_lowq and n_sites -- a block
//               reduction and one set of atomics per tile, the reference found by bisection of ref_base; a tile that holds
//               a border falls back to per-thread sums, as bmc's runs_count does.
//   sites_emit  the same tiles with the scanned tile counts: the k-th site in place order writes its twelve words at 12 k;
//               ranks, not atomics, place every value.
// The walk itself -- which records count, the two classes, the word-wise reads -- is bmp_walk.hip.h, templates over the action
// at a base, a deleted position and an insertion; bmg_kernels.hip.h instantiates them with another action.
// No kernel waits for another workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm_scan.hip.h"
#include "bmp_walk.hip.h"

namespace bmp {

constexpr uint32_t kItems = bmscan::kItems, kTile = bmscan::kTile;
constexpr uint32_t kCounters = 8, kDel = 5, kIns = 6, kLowq = 7;   // BMP_N_COUNTERS and the places in it
constexpr uint32_t kSiteWords = 12;                      // BMP_SITE_WORDS
constexpr uint32_t kRefPad = 8;                          // bytes of room behind ref: sites_* read whole 8-byte words
static_assert(kThreads == (uint32_t)bmscan::kThreads && kItems == 8, "the site passes use the scan's tiles and 8-byte reference words");

struct thresholds {
    uint32_t min_mapq, min_bq, min_alt, min_frac_ppm;
};

// the counter of a base with the quality q and the 4-bit code
__device__ __forceinline__ uint32_t counter_of(uint32_t q, uint32_t code, uint32_t min_bq) {
    if (q != kQualNone && q < min_bq) return kLowq;
    return code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
}

// the action of bmp_walk.hip.h's walkers: every count is a no-return add -- the result is not used, so the compiler issues
// global_atomic_add_u32 without a returned value
struct count_action {
    static constexpr bool kIndels = true, kStats = true;
    uint32_t *__restrict__ c;
    uint32_t min_bq;
    __device__ __forceinline__ count_action on(uint64_t first, uint32_t, uint32_t) const { return count_action{c + first * kCounters, min_bq}; }
    __device__ __forceinline__ void count(uint64_t position, uint32_t which) const { atomicAdd(&c[position * kCounters + which], 1u); }
    __device__ __forceinline__ void base(uint64_t position, uint32_t q, uint32_t code) const { count(position, counter_of(q, code, min_bq)); }
    __device__ __forceinline__ void del(uint64_t position) const { count(position, kDel); }
    __device__ __forceinline__ void ins(uint64_t position) const { count(position, kIns); }
};

// cnt += the bases, deletions and insertions of the counted records, stats += n_reads, n_low_mapq, n_left_out
__global__ __launch_bounds__(kThreads) void add_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                       const uint8_t *__restrict__ skip, const uint32_t *__restrict__ ref_len,
                                                       const uint64_t *__restrict__ ref_base, uint32_t n_ref, thresholds th,
                                                       uint32_t *__restrict__ cnt, unsigned long long *__restrict__ stats) {
    add_records(in, rec_offset, n, skip, ref_len, ref_base, n_ref, th.min_mapq, count_action{cnt, th.min_bq}, stats);
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

// 0 .. 3 for A C G T in either case, 4 for every other byte
__device__ __forceinline__ uint32_t allele_of(uint32_t byte) {
    const uint32_t u = byte & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// the kind bits of a position with the counters v and the reference allele
__device__ __forceinline__ uint32_t kind_of(const uint32_t (&v)[kCounters], uint32_t allele, const thresholds &th) {
    const uint64_t span = (uint64_t)v[0] + v[1] + v[2] + v[3] + v[4] + v[kDel];
    const uint64_t bar = (uint64_t)th.min_frac_ppm * span;               // < 2^20 * 2^35
    uint32_t alt = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) alt = k != allele && v[k] > alt ? v[k] : alt;
    const bool snv = allele < 4 && alt >= th.min_alt && (uint64_t)alt * 1000000u >= bar;
    const bool del = v[kDel] >= th.min_alt && (uint64_t)v[kDel] * 1000000u >= bar;
    const bool ins = v[kIns] >= th.min_alt && (uint64_t)v[kIns] * 1000000u >= bar;
    return (snv ? 1u : 0u) | (del ? 2u : 0u) | (ins ? 4u : 0u);
}

__device__ __forceinline__ void load_counters(const uint32_t *__restrict__ cnt, uint64_t slot, uint32_t (&v)[kCounters]) {
    const uint4 *p = reinterpret_cast<const uint4 *>(cnt + slot * kCounters);   // 32-byte aligned: cnt is, and a position has 32 bytes
    const uint4 lo = p[0], hi = p[1];
    v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
}

// the thread's kItems reference bytes as one word (ref has kRefPad bytes of room; base is a multiple of 8)
__device__ __forceinline__ uint64_t load_ref_bytes(const uint8_t *__restrict__ ref, uint64_t base) {
    return *reinterpret_cast<const uint64_t *>(ref + base);
}

__global__ __launch_bounds__(kThreads) void sites_count_kernel(const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ ref, uint64_t n_slots,
                                                               const uint64_t *__restrict__ ref_base, uint32_t n_ref, thresholds th,
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
    uint32_t sites = 0, is_site = 0;                     // is_site: bit j for the thread's j-th position
    uint64_t bases = 0, lowq = 0;
    const uint64_t letters = base < n_slots ? load_ref_bytes(ref, base) : 0u;
#pragma unroll
    for (uint32_t j = 0; j < kItems; j++) {
        if (base + j >= n_slots) continue;
        uint32_t v[kCounters];
        load_counters(cnt, base + j, v);
        const uint32_t kind = kind_of(v, allele_of((uint32_t)(letters >> (8 * j)) & 255u), th);
        sites += kind != 0;
        is_site |= (kind != 0 ? 1u : 0u) << j;
        bases += (uint64_t)v[0] + v[1] + v[2] + v[3] + v[4];
        lowq += v[kLowq];
    }
    uint32_t all_sites;
    uint64_t all_bases, all_lowq;
    (void)bmscan::block_inclusive<uint32_t>(sites, ws32, &all_sites);   // its barriers also publish s_ref
    (void)bmscan::block_inclusive<uint64_t>(bases, ws64, &all_bases);
    (void)bmscan::block_inclusive<uint64_t>(lowq, ws64, &all_lowq);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = all_sites;
    const uint32_t r_first = s_ref[0], r_last = s_ref[1];
    if (r_first == r_last) {                             // the whole tile on one reference
        if (threadIdx.x == 0) {
            unsigned long long *st = stats + (uint64_t)r_first * kStats;
            if (all_bases) atomicAdd(&st[3], (unsigned long long)all_bases);
            if (all_lowq) atomicAdd(&st[4], (unsigned long long)all_lowq);
            if (all_sites) atomicAdd(&st[5], (unsigned long long)all_sites);
        }
        return;
    }
    if ((bases == 0 && lowq == 0 && sites == 0) || base >= n_slots) return;   // a border in the tile: every thread for itself
    uint32_t r = ref_of(ref_base, n_ref, base);
    uint64_t next = ref_base[r + 1], b = 0, l = 0, s = 0;
    auto flush = [&]() {
        unsigned long long *st = stats + (uint64_t)r * kStats;
        if (b) atomicAdd(&st[3], (unsigned long long)b);
        if (l) atomicAdd(&st[4], (unsigned long long)l);
        if (s) atomicAdd(&st[5], (unsigned long long)s);
        b = l = s = 0;
    };
    for (uint32_t j = 0; j < kItems && base + j < n_slots; j++) {
        while (base + j >= next) {                       // r + 1 < n_ref here: the slot lies below ref_base[n_ref]
            flush();
            r++;
            next = ref_base[r + 1];
        }
        uint32_t v[kCounters];
        load_counters(cnt, base + j, v);                 // once more: only the few tiles with a border come here
        b += (uint64_t)v[0] + v[1] + v[2] + v[3] + v[4];
        l += v[kLowq];
        s += (is_site >> j) & 1u;
    }
    flush();
}

// sites[12 k ..] = (reference, position, allele, the eight counters, kind) of the k-th site in place order; tile_rank = the
// exclusive sums of tile_count
__global__ __launch_bounds__(kThreads) void sites_emit_kernel(const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ ref, uint64_t n_slots,
                                                              const uint64_t *__restrict__ ref_base, uint32_t n_ref, thresholds th,
                                                              const uint32_t *__restrict__ tile_rank, uint32_t n_sites, uint32_t *__restrict__ out) {
    __shared__ uint32_t ws32[kThreads / 64 + 1];
    const uint64_t base = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kItems;
    const uint64_t letters = base < n_slots ? load_ref_bytes(ref, base) : 0u;
    uint32_t kinds = 0, sites = 0;                       // kinds: 3 bits per position
#pragma unroll
    for (uint32_t j = 0; j < kItems; j++) {
        if (base + j >= n_slots) continue;
        uint32_t v[kCounters];
        load_counters(cnt, base + j, v);
        const uint32_t kind = kind_of(v, allele_of((uint32_t)(letters >> (8 * j)) & 255u), th);
        kinds |= kind << (3 * j);
        sites += kind != 0;
    }
    uint32_t all;
    uint32_t rank = bmscan::block_inclusive<uint32_t>(sites, ws32, &all) - sites + tile_rank[blockIdx.x];   // sites before this thread's positions
    if (sites == 0) return;
    uint32_t r = ref_of(ref_base, n_ref, base);
    for (uint32_t j = 0; j < kItems; j++) {
        const uint32_t kind = (kinds >> (3 * j)) & 7u;
        if (kind == 0) continue;
        const uint64_t slot = base + j;
        while (slot >= ref_base[r + 1]) r++;
        if (rank < n_sites) {                            // always; keeps a wrong scan from becoming a wild store
            uint32_t v[kCounters];
            load_counters(cnt, slot, v);
            uint4 *o = reinterpret_cast<uint4 *>(out + (uint64_t)rank * kSiteWords);   // 48 bytes a site: 16-byte aligned
            o[0] = make_uint4(r, (uint32_t)(slot - ref_base[r]), allele_of((uint32_t)(letters >> (8 * j)) & 255u), v[0]);
            o[1] = make_uint4(v[1], v[2], v[3], v[4]);
            o[2] = make_uint4(v[5], v[6], v[7], kind);
        }
        rank++;
    }
}

}  // namespace bmp
