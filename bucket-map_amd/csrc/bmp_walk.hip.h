// bmp_walk.hip.h -- the walk of a BAM record stream that the pileup counter (bmp_kernels.hip.h), the genotype caller
// (bmg_kernels.hip.h) and the bias annotator (bmb_kernels.hip.h) share: which records are counted (include/bmp.h: PLACED,
// COUNTED RECORD), the two-class walk of their CIGARs with the clipping to the reference, and the word-wise reads of qualities and packed sequence.  What happens at a
// base, a deleted position and an insertion's anchor is the ACTION the walkers are templates over; each module has its own.
// Templates and inline functions only: no kernel is defined here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm_scan.hip.h"

namespace bmp {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kShortOps = 8, kShortSeq = 512;       // add: what one lane walks alone
constexpr uint32_t kWideSpan = 16;                       // add: positions of an op from which the wave shares them
constexpr uint32_t kStats = 6;                           // BMP_N_STATS; n_reads n_low_mapq n_left_out n_bases n_lowq n_sites
constexpr uint32_t kSkipFlags = 0x4u | 0x100u | 0x200u | 0x400u, kQualNone = 0xFF;

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

// WHAT THE WALK DOES AT A BASE, A DELETED POSITION AND AN INSERTION'S ANCHOR is its action, a small struct:
//   Act on(first, flag, mapq) const  the action on the reference whose first slot is `first`, for a record with that flag
//                                and that mapq byte (bmb's action keeps them, the others ignore them); positions count from first
//   void base(p, q, code) const  a base of an M, = or X op at position p with the quality byte q and the 4-bit code
//   void del(p) const            a deleted position;  void ins(p) const  an insertion anchored at p
//   kIndels                      false: del and ins do nothing, and the walkers leave their loops out
//   kStats                       true: add_records sums n_reads, n_low_mapq and n_left_out per reference

// bases [q0, q0 + n) of the query at positions [s, s + n), one base at a time (byte loads): a lane's own short stretch
template <class Act>
__device__ __forceinline__ void bases_alone(const uint8_t *seq, const uint8_t *qual, uint64_t q0, uint64_t n, uint64_t s, const Act &act) {
    for (uint64_t j = 0; j < n; j++) {
        const uint64_t at = q0 + j;
        const uint32_t code = (seq[at >> 1] >> ((at & 1u) ? 0 : 4)) & 15u;
        act.base(s + j, qual[at], code);
    }
}

// the same by all lanes (every argument is the same in all of them).  A lane takes the aligned word of four quality bytes
// at w; a word may reach up to 3 bytes before qual + q0 (the same record) and behind the last byte (the stream's buffer has
// 16 bytes of room behind its end); those bytes are masked out.  The bases' nibbles lie in at most 3 consecutive bytes of
// seq, read as the two aligned words from the first one's on (the second at most 4 bytes behind a byte of seq: inside the
// qualities or the room).
template <class Act>
__device__ __forceinline__ void bases_shared(const uint8_t *seq, const uint8_t *qual, uint64_t q0, uint64_t n, uint64_t s, const Act &act,
                                             uint32_t lane) {
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
            act.base(s + (addr - a), (x >> (8 * j)) & 255u, code);
        }
    }
}

// one counted record by its lane alone: at most kShortOps ops, kShortSeq bases and kShortSeq deleted positions
template <class Act>
__device__ __forceinline__ void walk_alone(const uint8_t *cigar, uint32_t n_cigar, const uint8_t *seq, const uint8_t *qual, uint32_t pos, uint32_t rlen,
                                           const Act &act) {
    uint64_t rc = pos, qc = 0;
    bool anchored = false;                               // an M, =, X or D of a length > 0 came before
    (void)anchored;
    for (uint32_t k = 0; k < n_cigar; k++) {
        const uint32_t w = load32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
        if ((is_block(op) || op == 2) && len && rc < rlen) {
            const uint64_t e = rc + len < rlen ? rc + len : rlen;
            if (op == 2) {
                if constexpr (Act::kIndels)
                    for (uint64_t p = rc; p < e; p++) act.del(p);
            } else
                bases_alone(seq, qual, qc, e - rc, rc, act);   // qc + (e - rc) <= l_seq: the host has checked the query length
        }
        if constexpr (Act::kIndels) {
            if (op == 1 && len && anchored && rc >= 1 && rc - 1 < rlen) act.ins(rc - 1);
            if ((is_block(op) || op == 2) && len) anchored = true;
        }
        if (takes_ref(op)) rc += len;
        if (takes_query(op)) qc += len;
    }
}

// one counted record by the whole wave (every argument is the same in all lanes)
template <class Act>
__device__ __forceinline__ void walk_wave(const uint8_t *cigar, uint32_t n_cigar, const uint8_t *seq, const uint8_t *qual, uint32_t pos, uint32_t rlen,
                                          const Act &act, uint32_t lane) {
    uint64_t rc = pos, qc = 0;
    bool anchored = false;
    (void)anchored;
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
        if constexpr (Act::kIndels) {
            const uint64_t anchors = __ballot((is_block(op) || op == 2) && len);
            const bool before = anchored || (anchors & ((uint64_t{1} << lane) - 1)) != 0;
            if (op == 1 && len && before && s >= 1 && s - 1 < rlen) act.ins(s - 1);
            anchored = anchored || anchors != 0;
        }
        const bool del = Act::kIndels && op == 2;
        const bool has = (is_block(op) || del) && len && s < rlen;
        const uint64_t span = has ? (s + len < rlen ? s + len : rlen) - s : 0u;   // q0 + span <= l_seq for a block (host check)
        if (span && span < kWideSpan) {
            if (del) {
                if constexpr (Act::kIndels)
                    for (uint64_t p = 0; p < span; p++) act.del(s + p);
            } else
                bases_alone(seq, qual, q0, span, s, act);
        }
        uint64_t wide = __ballot(span >= kWideSpan);
        while (wide) {
            const int src = __ffsll((unsigned long long)wide) - 1;
            wide &= wide - 1;
            const uint64_t at = __shfl(q0, src, 64), n = __shfl(span, src, 64), from = __shfl(s, src, 64);
            if (__shfl((int)del, src, 64)) {
                if constexpr (Act::kIndels)
                    for (uint64_t p = lane; p < n; p += 64) act.del(from + p);
            } else
                bases_shared(seq, qual, at, n, from, act, lane);
        }
        rc += __shfl(r_incl, 63, 64);
        qc += __shfl(q_incl, 63, 64);
    }
}

// The records' pass of an add kernel: the action of the bases, deletions and insertions of the counted records and, with
// kStats, stats += n_reads, n_low_mapq, n_left_out.  `in` has 16 bytes of room behind n_bytes; the fields of a record fit its
// extent, ops are 0 .. 8, the query length is l_seq (host checks).
template <class Act>
__device__ __forceinline__ void add_records(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                            const uint8_t *__restrict__ skip, const uint32_t *__restrict__ ref_len,
                                            const uint64_t *__restrict__ ref_base, uint32_t n_ref, uint32_t min_mapq, const Act &act,
                                            unsigned long long *__restrict__ stats) {
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
            counted = !left_out && r[13] >= min_mapq;
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
                    walk_alone(cigar, n_cigar, seq, seq + ((uint64_t)l_seq + 1) / 2, (uint32_t)pos_i, rlen, act.on(ref_base[ref], flag, r[13]));
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
        const uint32_t w_flag = load16(r + 18), w_mapq = r[13];   // dead code where the action ignores them
        const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar;
        walk_wave(cigar, n_cigar, seq, seq + ((uint64_t)l_seq + 1) / 2, w_pos, ref_len[w_ref], act.on(ref_base[w_ref], w_flag, w_mapq), lane);
    }
    if constexpr (Act::kStats) {
        uint64_t left = __ballot(placed);
        while (left) {                                   // per reference among the wave's lanes: one atomic per value
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
}

}  // namespace bmp
