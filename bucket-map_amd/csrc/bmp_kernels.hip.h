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
// No kernel waits for another workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm_scan.hip.h"

namespace bmp {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kShortOps = 8, kShortSeq = 512;       // add: what one lane walks alone
constexpr uint32_t kWideSpan = 16;                       // add: positions of an op from which the wave shares them
constexpr uint32_t kItems = bmscan::kItems, kTile = bmscan::kTile;
constexpr uint32_t kCounters = 8, kDel = 5, kIns = 6, kLowq = 7;   // BMP_N_COUNTERS and the places in it
constexpr uint32_t kStats = 6;                           // BMP_N_STATS; n_reads n_low_mapq n_left_out n_bases n_lowq n_sites
constexpr uint32_t kSiteWords = 12;                      // BMP_SITE_WORDS
constexpr uint32_t kSkipFlags = 0x4u | 0x100u | 0x200u | 0x400u, kQualNone = 0xFF;
constexpr uint32_t kRefPad = 8;                          // bytes of room behind ref: sites_* read whole 8-byte words
static_assert(kThreads == (uint32_t)bmscan::kThreads && kItems == 8, "the site passes use the scan's tiles and 8-byte reference words");

struct thresholds {
    uint32_t min_mapq, min_bq, min_alt, min_frac_ppm;
};

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

__device__ __forceinline__ bool is_block(uint32_t op) { return op == 0 || op == 7 || op == 8; }
__device__ __forceinline__ bool takes_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
__device__ __forceinline__ bool takes_query(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }

// the counter of a base with the quality q and the 4-bit code
__device__ __forceinline__ uint32_t counter_of(uint32_t q, uint32_t code, uint32_t min_bq) {
    if (q != kQualNone && q < min_bq) return kLowq;
    return code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
}

// the no-return add: the result is not used, so the compiler issues global_atomic_add_u32 without a returned value
__device__ __forceinline__ void count(uint32_t *__restrict__ c, uint64_t position, uint32_t which) {
    atomicAdd(&c[position * kCounters + which], 1u);
}

// bases [q0, q0 + n) of the query at positions [s, s + n), one base at a time (byte loads): a lane's own short stretch
__device__ __forceinline__ void bases_alone(const uint8_t *seq, const uint8_t *qual, uint64_t q0, uint64_t n, uint64_t s, uint32_t *__restrict__ c,
                                            uint32_t min_bq) {
    for (uint64_t j = 0; j < n; j++) {
        const uint64_t at = q0 + j;
        const uint32_t code = (seq[at >> 1] >> ((at & 1u) ? 0 : 4)) & 15u;
        count(c, s + j, counter_of(qual[at], code, min_bq));
    }
}

// the same by all lanes (every argument is the same in all of them).  A lane takes the aligned word of four quality bytes
// at w; a word may reach up to 3 bytes before qual + q0 (the same record) and behind the last byte (the stream's buffer has
// 16 bytes of room behind its end); those bytes are masked out.  The bases' nibbles lie in at most 3 consecutive bytes of
// seq, read as the two aligned words from the first one's on (the second at most 4 bytes behind a byte of seq: inside the
// qualities or the room).
__device__ __forceinline__ void bases_shared(const uint8_t *seq, const uint8_t *qual, uint64_t q0, uint64_t n, uint64_t s, uint32_t *__restrict__ c,
                                             uint32_t lane, uint32_t min_bq) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(qual + q0), b = a + n;
    for (uintptr_t w = (a & ~uintptr_t{3}) + 4u * lane; w < b; w += 4u * 64u) {
        const uint32_t x = *reinterpret_cast<const uint32_t *>(w);
        const uintptr_t first = w < a ? a : w;           // the first byte of the word that counts
        const uint64_t at0 = q0 + (first - a);           // its query index
        const uintptr_t sb = reinterpret_cast<uintptr_t>(seq + (at0 >> 1));
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(sb & ~uintptr_t{3});
        const uint64_t packed = ((uint64_t)sw[0] | (uint64_t)sw[1] << 32) >> (8u * (uint32_t)(sb & 3u));   // byte i: seq[(at0 >> 1) + i]
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uintptr_t addr = w + j;
            if (addr < first || addr >= b) continue;
            const uint64_t at = q0 + (addr - a);
            const uint32_t byte = (uint32_t)(packed >> (8u * (uint32_t)((at >> 1) - (at0 >> 1)))) & 255u;
            const uint32_t code = (byte >> ((at & 1u) ? 0 : 4)) & 15u;
            count(c, s + (addr - a), counter_of((x >> (8 * j)) & 255u, code, min_bq));
        }
    }
}

// one counted record by its lane alone: at most kShortOps ops, kShortSeq bases and kShortSeq deleted positions
__device__ __forceinline__ void walk_alone(const uint8_t *cigar, uint32_t n_cigar, const uint8_t *seq, const uint8_t *qual, uint32_t pos, uint32_t rlen,
                                           uint32_t *__restrict__ c, uint32_t min_bq) {
    uint64_t rc = pos, qc = 0;
    bool anchored = false;                               // an M, =, X or D of a length > 0 came before
    for (uint32_t k = 0; k < n_cigar; k++) {
        const uint32_t w = load32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
        if ((is_block(op) || op == 2) && len && rc < rlen) {
            const uint64_t e = rc + len < rlen ? rc + len : rlen;
            if (op == 2)
                for (uint64_t p = rc; p < e; p++) count(c, p, kDel);
            else
                bases_alone(seq, qual, qc, e - rc, rc, c, min_bq);   // qc + (e - rc) <= l_seq: the host has checked the query length
        }
        if (op == 1 && len && anchored && rc >= 1 && rc - 1 < rlen) count(c, rc - 1, kIns);
        if ((is_block(op) || op == 2) && len) anchored = true;
        if (takes_ref(op)) rc += len;
        if (takes_query(op)) qc += len;
    }
}

// one counted record by the whole wave (every argument is the same in all lanes)
__device__ __forceinline__ void walk_wave(const uint8_t *cigar, uint32_t n_cigar, const uint8_t *seq, const uint8_t *qual, uint32_t pos, uint32_t rlen,
                                          uint32_t *__restrict__ c, uint32_t lane, uint32_t min_bq) {
    uint64_t rc = pos, qc = 0;
    bool anchored = false;
    for (uint32_t c0 = 0; c0 < n_cigar; c0 += 64) {      // the same trips in every lane: shuffles and ballots below
        const uint32_t k = c0 + lane;
        uint32_t op = 15, len = 0;
        if (k < n_cigar) {
            const uint32_t w = load32(cigar + 4ull * k);
            op = w & 15u, len = w >> 4;
        }
        const uint64_t r_adv = takes_ref(op) ? len : 0u, q_adv = takes_query(op) ? len : 0u;
        const uint64_t r_incl = bmscan::wave_inclusive<uint64_t>(r_adv, lane), q_incl = bmscan::wave_inclusive<uint64_t>(q_adv, lane);
        const uint64_t s = rc + r_incl - r_adv, q0 = qc + q_incl - q_adv;
        const uint64_t anchors = __ballot((is_block(op) || op == 2) && len);
        const bool before = anchored || (anchors & ((uint64_t{1} << lane) - 1)) != 0;
        if (op == 1 && len && before && s >= 1 && s - 1 < rlen) count(c, s - 1, kIns);
        const bool del = op == 2;
        const bool has = (is_block(op) || del) && len && s < rlen;
        const uint64_t span = has ? (s + len < rlen ? s + len : rlen) - s : 0u;   // q0 + span <= l_seq for a block (host check)
        if (span && span < kWideSpan) {
            if (del)
                for (uint64_t p = 0; p < span; p++) count(c, s + p, kDel);
            else
                bases_alone(seq, qual, q0, span, s, c, min_bq);
        }
        uint64_t wide = __ballot(span >= kWideSpan);
        while (wide) {
            const int src = __ffsll((unsigned long long)wide) - 1;
            wide &= wide - 1;
            const uint64_t at = __shfl(q0, src, 64), n = __shfl(span, src, 64), from = __shfl(s, src, 64);
            if (__shfl((int)del, src, 64))
                for (uint64_t p = lane; p < n; p += 64) count(c, from + p, kDel);
            else
                bases_shared(seq, qual, at, n, from, c, lane, min_bq);
        }
        anchored = anchored || anchors != 0;
        rc += __shfl(r_incl, 63, 64);
        qc += __shfl(q_incl, 63, 64);
    }
}

// cnt += the bases, deletions and insertions of the counted records, stats += n_reads, n_low_mapq, n_left_out.  `in` has 16
// bytes of room behind n_bytes; the fields of a record fit its extent, ops are 0 .. 8, the query length is l_seq (host checks).
__global__ __launch_bounds__(kThreads) void add_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                       const uint8_t *__restrict__ skip, const uint32_t *__restrict__ ref_len,
                                                       const uint64_t *__restrict__ ref_base, uint32_t n_ref, thresholds th,
                                                       uint32_t *__restrict__ cnt, unsigned long long *__restrict__ stats) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x, wave_first = i - lane;
    bool placed = false, counted = false, left_out = false, wide = false;
    uint32_t ref = 0;
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
            left_out = l_seq == 0 || (n_cigar == 2 && load32(cigar) == (l_seq << 4 | 4u) && (load32(cigar + 4) & 15u) == 3u);   // the long-CIGAR placeholder
            counted = !left_out && r[13] >= th.min_mapq;
            if (counted) {
                wide = n_cigar > kShortOps || l_seq > kShortSeq;
                uint64_t deleted = 0;
                for (uint32_t k = 0; !wide && k < n_cigar; k++) {
                    const uint32_t w = load32(cigar + 4ull * k);
                    if ((w & 15u) == 2) deleted += w >> 4;
                }
                wide = wide || deleted > kShortSeq;
                if (!wide) {
                    const uint8_t *seq = cigar + 4ull * n_cigar;
                    walk_alone(cigar, n_cigar, seq, seq + ((uint64_t)l_seq + 1) / 2, (uint32_t)pos_i, rlen, cnt + ref_base[ref] * kCounters, th.min_bq);
                }
            }
        }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {                                       // the wave's other counted records, by all lanes
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint8_t *r = in + rec_offset[wave_first + src];
        const uint32_t w_ref = load32(r + 4), w_pos = load32(r + 8), l_name = r[12], n_cigar = load16(r + 16), l_seq = load32(r + 20);
        const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar;
        walk_wave(cigar, n_cigar, seq, seq + ((uint64_t)l_seq + 1) / 2, w_pos, ref_len[w_ref], cnt + ref_base[w_ref] * kCounters, lane, th.min_bq);
    }
    uint64_t left = __ballot(placed);
    while (left) {                                       // per reference among the wave's lanes: one atomic per value
        const int src = __ffsll((unsigned long long)left) - 1;
        const uint32_t r0 = __shfl(ref, src, 64);
        const bool mine = placed && ref == r0;
        left &= ~__ballot(mine);
        const uint32_t reads = wave_sum32(mine && counted ? 1u : 0u), low = wave_sum32(mine && !counted && !left_out ? 1u : 0u);
        const uint32_t out = wave_sum32(mine && left_out ? 1u : 0u);
        if ((int)lane == src) {
            unsigned long long *st = stats + (uint64_t)r0 * kStats;
            if (reads) atomicAdd(&st[0], (unsigned long long)reads);
            if (low) atomicAdd(&st[1], (unsigned long long)low);
            if (out) atomicAdd(&st[2], (unsigned long long)out);
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
