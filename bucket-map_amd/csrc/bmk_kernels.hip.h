// bmk_kernels.hip.h -- links between the het SNV sites that a BAM record stream observes, and the phase of the sites from
// them, on gfx950 (include/bmk.h states the rule).
//
// The state is slot[H] (u32, ascending: the site's position among the references back to back), meta[H] (uint4: reference,
// position, index of the call, allele letters a0 | a1 << 4) and link[(i * reach + d - 1) * 4 + 2 a_i + a_j] (u32).  Nothing is
// kept per reference position, and the add is SITE-DRIVEN: it reads one quality byte and one nibble per site under a record.
//
//   add      one record per lane, the project's two classes (bmp_walk.hip.h's counted-record test, restated here because the
//            walk below is another one).  A SHORT record (at most kShortOps ops and kShortSeq bases) is walked by its lane
//            alone: one binary search for its first site (and one over the sites under each D or N, however long it is), then
//            a reference cursor, a query cursor and a site cursor over its ops; the last eight observations live in registers (eight site numbers shifted by constant indices and a byte of
//            allele bits), so a new observation is paired with at most `reach` earlier ones on the spot.  Every OTHER record is
//            shared by its wave: 64 ops per trip, op starts from bmscan::wave_inclusive, and the sites under the trip's ops are
//            taken 64 at a time, lane l the site cursor + l.  A lane finds the op over its site by a 6-step search of the
//            inclusive ends through shuffles.  The observations of a trip are then a DENSE SLOT ARRAY indexed by site - first
//            site of the trip, one bit per slot, held as two ballots (observed, allele) -- order-free by construction; the eight
//            slots before the trip are a byte pair carried from trip to trip.  Lane l pairs its slot with the slots l - 1 ..
//            l - reach.  A link is one no-return 32-bit global atomic add.  No LDS, no scratch.
//   pick     one thread per site: parent, flip, d, cis, trans from its <= reach cells (one uint4 load each).
//   jump     pointer jumping with parity, parent | hap << 31 in one word, ping-pong: a round reads only the other array.
//   mark     a non-root sets its root's mark (atomic or, no return).
//   out      the eight words of a site and the two sums (wave sums, then one 64-bit atomic per wave and value).
// No kernel waits for another workgroup.
#pragma once

#include "bmp_walk.hip.h"

namespace bmk {

constexpr uint32_t kThreads = bmp::kThreads;
constexpr uint32_t kCallWords = 24, kOutWords = 8, kStats = 4, kMaxReach = 8;   // BMK_CALL_WORDS, BMK_OUT_WORDS, BMK_N_STATS, BMK_MAX_REACH
constexpr uint32_t kPhased = 1, kRoot = 2, kVariant = 2;
constexpr uint32_t kNoSite = 0xFFFFFFFFu;

struct params {
    uint32_t min_mapq, min_bq, min_links, min_frac_ppm, reach;
};

// the first site in [lo, H) whose slot is >= key (slot ascends)
__device__ __forceinline__ uint32_t first_site_from(const uint32_t *__restrict__ slot, uint32_t lo, uint32_t H, uint64_t key) {
    uint32_t hi = H;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (slot[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// 0 or 1: which allele of the site the base at query index `at` is; 2: no observation
__device__ __forceinline__ uint32_t observe(const uint8_t *seq, const uint8_t *qual, uint64_t at, uint32_t alleles, uint32_t min_bq) {
    const uint32_t q = qual[at];
    if (q != bmp::kQualNone && q < min_bq) return 2u;
    const uint32_t code = (seq[at >> 1] >> ((at & 1u) ? 0 : 4)) & 15u;
    const uint32_t letter = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
    return letter == (alleles & 15u) ? 0u : letter == (alleles >> 4) ? 1u : 2u;   // a letter of 4 equals neither: alleles are 0 .. 3
}

// a short record by its lane alone; returns its observations
__device__ __forceinline__ uint32_t links_alone(const uint8_t *cigar, uint32_t n_cigar, const uint8_t *seq, const uint8_t *qual, uint32_t pos, uint32_t rlen,
                                                uint64_t base, const uint32_t *__restrict__ slot, const uint4 *__restrict__ meta, uint32_t H,
                                                const params &pr, uint32_t *__restrict__ link) {
    uint32_t sc = first_site_from(slot, 0, H, base + pos);
    uint64_t rc = pos, qc = 0;
    uint32_t prev[kMaxReach];                            // the sites of the last observations, the latest first; constant indices only
#pragma unroll
    for (uint32_t k = 0; k < kMaxReach; k++) prev[k] = kNoSite;
    uint32_t prev_a = 0, n_obs = 0;                      // bit k: the allele seen at prev[k]
    for (uint32_t k = 0; k < n_cigar && rc < rlen && sc < H; k++) {
        const uint32_t w = bmp::load32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
        if (bmp::takes_ref(op) && len) {
            const uint64_t e = rc + len < rlen ? rc + len : rlen, limit = base + e;
            if (!bmp::is_block(op)) sc = first_site_from(slot, sc, H, limit);   // a D or an N observes nothing: over its sites in one search, however long it is
            while (sc < H && slot[sc] < limit) {
                if (bmp::is_block(op)) {
                    const uint64_t p = slot[sc] - base;
                    const uint32_t a = observe(seq, qual, qc + (p - rc), meta[sc].w, pr.min_bq);   // qc + (p - rc) < l_seq: the host has checked the query length
                    if (a < 2) {
#pragma unroll
                        for (uint32_t b = 0; b < kMaxReach; b++)
                            if (prev[b] != kNoSite && sc - prev[b] <= pr.reach)
                                atomicAdd(&link[((uint64_t)prev[b] * pr.reach + (sc - prev[b] - 1)) * 4 + 2 * ((prev_a >> b) & 1u) + a], 1u);   // no result used: no return
#pragma unroll
                        for (uint32_t b = kMaxReach - 1; b > 0; b--) prev[b] = prev[b - 1];
                        prev[0] = sc;
                        prev_a = prev_a << 1 | a;
                        n_obs++;
                    }
                }
                sc++;
            }
        }
        if (bmp::takes_ref(op)) rc += len;
        if (bmp::takes_query(op)) qc += len;
    }
    return n_obs;
}

// one record by the whole wave (every argument is the same in all lanes); returns this lane's observations
__device__ __forceinline__ uint32_t links_wave(const uint8_t *cigar, uint32_t n_cigar, const uint8_t *seq, const uint8_t *qual, uint32_t pos, uint32_t rlen,
                                               uint64_t base, const uint32_t *__restrict__ slot, const uint4 *__restrict__ meta, uint32_t H,
                                               const params &pr, uint32_t *__restrict__ link, uint32_t lane) {
    uint32_t sc = first_site_from(slot, 0, H, base + pos);  // the same in every lane
    uint64_t rc = pos, qc = 0;
    uint32_t before_has = 0, before_a = 0, n_obs = 0;    // bit k: the slot of site sc - 8 + k
    for (uint32_t c0 = 0; c0 < n_cigar && rc < rlen && sc < H; c0 += 64) {   // the same trips in every lane
        const uint32_t k = c0 + lane;
        uint32_t op = 15, len = 0;
        if (k < n_cigar) {
            const uint32_t w = bmp::load32(cigar + 4ull * k);
            op = w & 15u, len = w >> 4;
        }
        const uint64_t r_adv = bmp::takes_ref(op) ? len : 0u, q_adv = bmp::takes_query(op) ? len : 0u;
        const uint64_t r_incl = bmscan::wave_inclusive<uint64_t>(r_adv, lane), q_incl = bmscan::wave_inclusive<uint64_t>(q_adv, lane);
        const uint64_t r_end = rc + r_incl, q0 = qc + q_incl - q_adv;   // r_end ascends over the lanes
        const uint64_t trip_end = __shfl(r_end, 63, 64);
        const uint64_t limit = base + (trip_end < rlen ? trip_end : rlen);
        for (;;) {                                       // the sites under this trip's ops, 64 at a time
            const uint32_t j = sc + lane;                // sc < H <= 2^31: no wrap
            const uint32_t at_slot = j < H ? slot[j] : 0u;
            const bool mine = j < H && at_slot < limit;
            const uint64_t taken = __ballot(mine);       // slot ascends: the lanes 0 .. count - 1
            const uint32_t count = (uint32_t)__popcll((unsigned long long)taken);
            if (count == 0) break;
            const uint64_t p = mine ? at_slot - base : rc;   // rc <= p < trip_end
            uint32_t src = 0;                            // the lanes whose ops end at or before p: the op over p is the next one
#pragma unroll
            for (uint32_t step = 32; step > 0; step >>= 1) {
                const uint64_t v = __shfl(r_end, (int)(src + step - 1), 64);
                if (v <= p) src += step;
            }
            src &= 63u;                                  // p < trip_end = r_end of lane 63, so src <= 63 already
            const uint32_t s_op = __shfl(op, (int)src, 64);
            const uint64_t s_end = __shfl(r_end, (int)src, 64), s_adv = __shfl(r_adv, (int)src, 64), s_q0 = __shfl(q0, (int)src, 64);
            uint32_t a = 2;
            if (mine && bmp::is_block(s_op)) a = observe(seq, qual, s_q0 + (p - (s_end - s_adv)), meta[j].w, pr.min_bq);
            const uint64_t has = __ballot(a < 2), ones = __ballot(a == 1);   // the dense slots of this batch: bit l is site sc + l
            if (a < 2) {
                n_obs++;
#pragma unroll
                for (uint32_t d = 1; d <= kMaxReach; d++) {
                    if (d > pr.reach || d > j) continue;
                    const bool seen = d <= lane ? (has >> (lane - d)) & 1u : (before_has >> (8u + lane - d)) & 1u;
                    if (!seen) continue;
                    const uint32_t a_i = d <= lane ? (uint32_t)(ones >> (lane - d)) & 1u : (before_a >> (8u + lane - d)) & 1u;
                    atomicAdd(&link[((uint64_t)(j - d) * pr.reach + (d - 1)) * 4 + 2 * a_i + a], 1u);
                }
            }
            if (count >= 8) {
                before_has = (uint32_t)(has >> (count - 8)) & 255u, before_a = (uint32_t)(ones >> (count - 8)) & 255u;
            } else {
                before_has = (before_has >> count | (uint32_t)has << (8 - count)) & 255u;
                before_a = (before_a >> count | (uint32_t)ones << (8 - count)) & 255u;
            }
            sc += count;
            if (count < 64) break;
        }
        rc = trip_end;
        qc += __shfl(q_incl, 63, 64);
    }
    return n_obs;
}

__global__ __launch_bounds__(kThreads) void add_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                       const uint8_t *__restrict__ skip, const uint32_t *__restrict__ ref_len,
                                                       const uint64_t *__restrict__ ref_base, uint32_t n_ref, params pr,
                                                       const uint32_t *__restrict__ slot, const uint4 *__restrict__ meta, uint32_t H,
                                                       uint32_t *__restrict__ link, unsigned long long *__restrict__ n_observations) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x, wave_first = i - lane;
    bool wide = false;
    uint32_t n_obs = 0;
    if (i < n) {
        const uint8_t *r = in + rec_offset[i];
        const int32_t ref_i = (int32_t)bmp::load32(r + 4), pos_i = (int32_t)bmp::load32(r + 8);
        const uint32_t l_name = r[12], n_cigar = bmp::load16(r + 16), flag = bmp::load16(r + 18), l_seq = bmp::load32(r + 20);
        bool placed = !(flag & bmp::kSkipFlags) && !(skip && skip[i]) && ref_i >= 0 && (uint32_t)ref_i < n_ref && pos_i >= 0 && n_cigar > 0;
        uint32_t rlen = 0;
        if (placed) {
            rlen = ref_len[ref_i];
            placed = (uint32_t)pos_i < rlen;
        }
        if (placed) {
            const uint8_t *cigar = r + 36 + l_name;
            const bool left_out = l_seq == 0 || (n_cigar == 2 && bmp::load32(cigar) == (l_seq << 4 | 4u) && (bmp::load32(cigar + 4) & 15u) == 3u);
            if (!left_out && r[13] >= pr.min_mapq) {
                wide = n_cigar > bmp::kShortOps || l_seq > bmp::kShortSeq;
                if (!wide) {
                    const uint8_t *seq = cigar + 4ull * n_cigar;
                    n_obs = links_alone(cigar, n_cigar, seq, seq + ((uint64_t)l_seq + 1) / 2, (uint32_t)pos_i, rlen, ref_base[ref_i], slot, meta, H, pr, link);
                }
            }
        }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {                                       // the wave's other counted records, by all lanes
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint8_t *r = in + rec_offset[wave_first + src];
        const uint32_t w_ref = bmp::load32(r + 4), w_pos = bmp::load32(r + 8), l_name = r[12], n_cigar = bmp::load16(r + 16), l_seq = bmp::load32(r + 20);
        const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar;
        n_obs += links_wave(cigar, n_cigar, seq, seq + ((uint64_t)l_seq + 1) / 2, w_pos, ref_len[w_ref], ref_base[w_ref], slot, meta, H, pr, link, lane);
    }
    const uint32_t sum = bmp::wave_sum32(n_obs);
    if (lane == 0 && sum) atomicAdd(n_observations, (unsigned long long)sum);
}

// parent | flip << 31 of site j (itself and 0 for a root) and (d, cis, trans) of its parent link
__global__ __launch_bounds__(kThreads) void pick_kernel(const uint4 *__restrict__ meta, const uint32_t *__restrict__ link, uint32_t H, params pr,
                                                        uint32_t *__restrict__ up, uint4 *__restrict__ chosen) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= H) return;
    const uint32_t ref = meta[j].x;
    uint32_t word = j;
    uint4 how = make_uint4(0, 0, 0, 0);
    for (uint32_t d = 1; d <= pr.reach && d <= j; d++) {
        const uint32_t i = j - d;
        if (meta[i].x != ref) break;                     // sites ascend: every earlier one is on another reference too
        const uint4 c = reinterpret_cast<const uint4 *>(link)[(uint64_t)i * pr.reach + (d - 1)];
        const uint64_t cis = (uint64_t)c.x + c.w, trans = (uint64_t)c.y + c.z, big = cis > trans ? cis : trans;
        if (big >= pr.min_links && big * 1000000ull >= (uint64_t)pr.min_frac_ppm * (cis + trans)) {
            word = i | (trans > cis ? 0x80000000u : 0u);
            how = make_uint4(d, (uint32_t)cis, (uint32_t)trans, 0);
            break;
        }
    }
    up[j] = word;
    chosen[j] = how;
}

// one round of pointer jumping with parity: to[j] from `from` alone
__global__ __launch_bounds__(kThreads) void jump_kernel(const uint32_t *__restrict__ from, uint32_t *__restrict__ to, uint32_t H) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= H) return;
    const uint32_t mine = from[j], above = from[mine & 0x7FFFFFFFu];
    to[j] = (above & 0x7FFFFFFFu) | ((mine ^ above) & 0x80000000u);
}

__global__ __launch_bounds__(kThreads) void mark_kernel(const uint32_t *__restrict__ up, uint32_t H, uint32_t *__restrict__ has_child) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= H) return;
    const uint32_t root = up[j] & 0x7FFFFFFFu;
    if (root != j) atomicOr(&has_child[root], 1u);       // no result used: no return
}

__global__ __launch_bounds__(kThreads) void out_kernel(const uint4 *__restrict__ meta, const uint32_t *__restrict__ up, const uint4 *__restrict__ chosen,
                                                       const uint32_t *__restrict__ has_child, uint32_t H, uint32_t *__restrict__ out,
                                                       unsigned long long *__restrict__ stats) {
    const uint32_t j = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t phased = 0, block = 0;
    if (j < H) {
        const uint32_t word = up[j], root = word & 0x7FFFFFFFu;
        const bool is_root = root == j;
        phased = has_child[root] & 1u;
        block = is_root ? phased : 0u;
        const uint4 how = chosen[j];
        uint4 *o = reinterpret_cast<uint4 *>(out + (uint64_t)j * kOutWords);
        o[0] = make_uint4(meta[j].z, root, meta[root].y, word >> 31);
        o[1] = make_uint4((phased ? kPhased : 0u) | (is_root ? kRoot : 0u), how.x, how.y, how.z);
    }
    const uint32_t n_phased = bmp::wave_sum32(phased), n_blocks = bmp::wave_sum32(block);
    if (lane == 0) {
        if (n_phased) atomicAdd(&stats[1], (unsigned long long)n_phased);
        if (n_blocks) atomicAdd(&stats[2], (unsigned long long)n_blocks);
    }
}

}  // namespace bmk
