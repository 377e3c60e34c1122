// bmn_kernels.hip.h -- the kernels of the indel caller (include/bmn.h states the rule), hand-written for gfx950.
//   add:    count_kernel  -- which records are counted (bmp.h's test), their extent into `cover` (two adds that return nothing
//                            per record), the number of events per record; the per-reference sums
//           emit_kernel   -- the same walk again with the scanned offsets: each event is one 16-byte store
//           Both keep bmp_walk.hip.h's two classes: a lane walks a record of at most kShortOps ops alone, the wave takes a
//           longer one 64 ops a trip with the cursors, the anchored flag and the event offset carried from trip to trip.
//           Only headers and CIGARs are read, and the packed sequence under an insertion of at most 32 bases.
//   finish: seq_keys / slot_keys (the two stable radix sorts of bms_radix_sort: seq first, then slot << 32 | w1), run_heads
//           and starts (the runs of equal events), alleles_kernel, cover_scan_kernel (with bm_scan's block sums),
//           anchor_heads, calls_kernel (one thread per anchor loops over its alleles; first the site flag, then, rank-placed,
//           the call).  No kernel waits for another workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bm_scan.hip.h"
#include "bmp_walk.hip.h"

namespace bmn {

using bmp::is_block;
using bmp::load16;
using bmp::load32;
using bmp::takes_query;
using bmp::takes_ref;
using bmp::wave_sum32;

constexpr uint32_t kThreads = 256;
constexpr uint32_t kShortOps = bmp::kShortOps;           // what one lane walks alone
constexpr uint32_t kStats = 3, kEventWords = 4, kAlleleWords = 8, kCallWords = 16, kMaxIns = 32;
constexpr uint32_t kGenotyped = 1, kVariant = 2;
constexpr uint32_t kIns = 1u << 31, kOther = 1u << 30;

struct params {
    uint32_t min_mapq, min_alt, min_frac_ppm, q_indel, prior;
};

__device__ __forceinline__ bool anchors(uint32_t op, uint32_t len) { return (is_block(op) || op == 2) && len; }

// the op at the reference cursor s gives an event (include/bmn.h: EVENTS); before: an anchoring op came before it
__device__ __forceinline__ bool is_event(uint32_t op, uint32_t len, bool before, uint64_t s, uint32_t rlen, uint32_t endc) {
    if (!len || !before || s < 1) return false;
    if (op == 2) return s + len <= rlen;
    return op == 1 && s < endc;
}

// the four words of the event of an I or D op at the cursors (s, q0) on the reference whose first slot is `first`
__device__ __forceinline__ uint4 make_event(uint64_t first, uint64_t s, uint32_t op, uint32_t len, const uint8_t *seq, uint64_t q0) {
    uint4 e;
    e.x = (uint32_t)(first + s - 1);
    e.y = len, e.z = 0, e.w = 0;
    if (op != 1) return e;
    e.y |= kIns;
    bool other = len > kMaxIns;
    uint64_t bits = 0;
    if (!other) {
        // The bases lie in at most 17 packed bytes from seq + (q0 >> 1) on, read as the at most five aligned words that hold
        // them.  A word may reach up to 3 bytes before that byte (the record's CIGAR or sequence) and behind the last one (its
        // qualities, or the stream's 16 bytes of room).  nib counts nibbles from the first word on, a byte's high nibble first.
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(seq + (q0 >> 1));
        const uint32_t *w = reinterpret_cast<const uint32_t *>(b0 & ~uintptr_t{3});
        const uint32_t nib0 = 2u * (uint32_t)(b0 & 3u) + (uint32_t)(q0 & 1u);
        uint32_t word = 0;
        for (uint32_t j = 0; j < len; j++) {
            const uint32_t nib = nib0 + j;
            if (j == 0 || !(nib & 7u)) word = w[nib >> 3];
            const uint32_t byte = (word >> (8u * ((nib >> 1) & 3u))) & 255u;
            const uint32_t code = (byte >> ((nib & 1u) ? 0 : 4)) & 15u;
            if (code == 0 || (code & (code - 1))) other = true;
            bits |= (uint64_t)((uint32_t)__ffs((int)code) - 1u & 3u) << (2 * j);
        }
    }
    if (other)
        e.y |= kOther;
    else
        e.z = (uint32_t)bits, e.w = (uint32_t)(bits >> 32);
    return e;
}

__device__ __forceinline__ void cover_add(uint32_t *cover, uint32_t pos, uint32_t endc) {
    if (endc >= pos + 2u) {                              // endc <= ref_len < 2^32 - 2: no wrap
        atomicAdd(&cover[pos], 1u);
        atomicAdd(&cover[endc - 1], 0xFFFFFFFFu);
    }
}

// The first pass of an add.  `in` has 16 bytes of room behind n_bytes; the fields of a record fit its extent, ops are 0 .. 8
// (host checks).  rec_events[i] = the events of record i, rec_end[i] = its end'.
__global__ __launch_bounds__(kThreads) void count_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                         const uint8_t *__restrict__ skip, const uint32_t *__restrict__ ref_len,
                                                         const uint64_t *__restrict__ ref_base, uint32_t n_ref, uint32_t min_mapq,
                                                         uint32_t *__restrict__ cover, unsigned long long *__restrict__ stats,
                                                         uint32_t *__restrict__ rec_events, uint32_t *__restrict__ rec_end) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x, wave_first = i - lane;
    bool placed = false, counted = false, left_out = false, wide = false;
    uint32_t ref = 0, events = 0, endc = 0;
    if (i < n) {
        const uint8_t *r = in + rec_offset[i];
        const int32_t ref_i = (int32_t)load32(r + 4), pos_i = (int32_t)load32(r + 8);
        const uint32_t l_name = r[12], n_cigar = load16(r + 16), flag = load16(r + 18), l_seq = load32(r + 20);
        placed = !(flag & bmp::kSkipFlags) && !(skip && skip[i]) && ref_i >= 0 && (uint32_t)ref_i < n_ref && pos_i >= 0 && n_cigar > 0;
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
            wide = counted && n_cigar > kShortOps;
            if (counted && !wide) {
                uint64_t end = (uint32_t)pos_i;
                for (uint32_t k = 0; k < n_cigar; k++) {
                    const uint32_t w = load32(cigar + 4ull * k);
                    if (takes_ref(w & 15u)) end += w >> 4;
                }
                endc = end < rlen ? (uint32_t)end : rlen;
                uint64_t rc = (uint32_t)pos_i;
                bool anchored = false;
                for (uint32_t k = 0; k < n_cigar; k++) {
                    const uint32_t w = load32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
                    events += is_event(op, len, anchored, rc, rlen, endc) ? 1u : 0u;
                    anchored = anchored || anchors(op, len);
                    if (takes_ref(op)) rc += len;
                }
                cover_add(cover + ref_base[ref], (uint32_t)pos_i, endc);
            }
        }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {                                       // the wave's records of many ops, by all lanes
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint8_t *r = in + rec_offset[wave_first + src];
        const uint32_t w_ref = load32(r + 4), w_pos = load32(r + 8), l_name = r[12], n_cigar = load16(r + 16);
        const uint8_t *cigar = r + 36 + l_name;
        const uint32_t rlen = ref_len[w_ref];
        uint64_t end = w_pos;
        for (uint32_t c0 = 0; c0 < n_cigar; c0 += 64) {  // the extent first: an insertion asks whether reference follows it
            const uint32_t k = c0 + lane;
            uint64_t adv = 0;
            if (k < n_cigar) {
                const uint32_t w = load32(cigar + 4ull * k);
                adv = takes_ref(w & 15u) ? w >> 4 : 0u;
            }
            end += __shfl(bmscan::wave_inclusive<uint64_t>(adv, lane), 63, 64);
        }
        const uint32_t w_endc = end < rlen ? (uint32_t)end : rlen;
        uint64_t rc = w_pos;
        bool anchored = false;
        uint32_t found = 0;
        for (uint32_t c0 = 0; c0 < n_cigar; c0 += 64) {
            const uint32_t k = c0 + lane;
            uint32_t op = 15, len = 0;
            if (k < n_cigar) {
                const uint32_t w = load32(cigar + 4ull * k);
                op = w & 15u, len = w >> 4;
            }
            const uint64_t r_adv = takes_ref(op) ? len : 0u;
            const uint64_t r_incl = bmscan::wave_inclusive<uint64_t>(r_adv, lane);
            const uint64_t a = __ballot(anchors(op, len));
            const bool before = anchored || (a & ((uint64_t{1} << lane) - 1)) != 0;
            found += (uint32_t)__popcll(__ballot(is_event(op, len, before, rc + r_incl - r_adv, rlen, w_endc)));
            anchored = anchored || a != 0;
            rc += __shfl(r_incl, 63, 64);
        }
        if ((int)lane == src) {
            events = found, endc = w_endc;
            cover_add(cover + ref_base[w_ref], w_pos, w_endc);
        }
    }
    if (i < n) rec_events[i] = events, rec_end[i] = endc;
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

// The second pass of an add: the events of record i go to events[first_event + rec_first[i] ...], in the order of its ops.
// Only records with events are walked (rec_events[i] > 0: counted, on a reference, with a CIGAR).
__global__ __launch_bounds__(kThreads) void emit_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                        const uint32_t *__restrict__ ref_len, const uint64_t *__restrict__ ref_base,
                                                        const uint32_t *__restrict__ rec_events, const uint32_t *__restrict__ rec_end,
                                                        const uint64_t *__restrict__ rec_first, uint64_t first_event, uint4 *__restrict__ events) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x, wave_first = i - lane;
    bool wide = false;
    if (i < n && rec_events[i]) {
        const uint8_t *r = in + rec_offset[i];
        const uint32_t ref = load32(r + 4), pos = load32(r + 8), l_name = r[12], n_cigar = load16(r + 16);
        wide = n_cigar > kShortOps;
        if (!wide) {
            const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar;
            const uint32_t rlen = ref_len[ref], endc = rec_end[i];
            const uint64_t first = ref_base[ref];
            uint64_t rc = pos, qc = 0, at = first_event + rec_first[i];
            bool anchored = false;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t w = load32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
                if (is_event(op, len, anchored, rc, rlen, endc)) events[at++] = make_event(first, rc, op, len, seq, qc);
                anchored = anchored || anchors(op, len);
                if (takes_ref(op)) rc += len;
                if (takes_query(op)) qc += len;
            }
        }
    }
    uint64_t todo = __ballot(wide);
    while (todo) {
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t rec = wave_first + src;
        const uint8_t *r = in + rec_offset[rec];
        const uint32_t w_ref = load32(r + 4), w_pos = load32(r + 8), l_name = r[12], n_cigar = load16(r + 16);
        const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar;
        const uint32_t rlen = ref_len[w_ref], endc = rec_end[rec];
        const uint64_t first = ref_base[w_ref];
        uint64_t rc = w_pos, qc = 0, at = first_event + rec_first[rec];
        bool anchored = false;
        for (uint32_t c0 = 0; c0 < n_cigar; c0 += 64) {  // the same trips in every lane: shuffles and ballots below
            const uint32_t k = c0 + lane;
            uint32_t op = 15, len = 0;
            if (k < n_cigar) {
                const uint32_t w = load32(cigar + 4ull * k);
                op = w & 15u, len = w >> 4;
            }
            const uint64_t r_adv = takes_ref(op) ? len : 0u, q_adv = takes_query(op) ? len : 0u;
            const uint64_t r_incl = bmscan::wave_inclusive<uint64_t>(r_adv, lane), q_incl = bmscan::wave_inclusive<uint64_t>(q_adv, lane);
            const uint64_t s = rc + r_incl - r_adv, q0 = qc + q_incl - q_adv;
            const uint64_t a = __ballot(anchors(op, len)), below = (uint64_t{1} << lane) - 1;
            const bool before = anchored || (a & below) != 0;
            const bool mine = is_event(op, len, before, s, rlen, endc);
            const uint64_t found = __ballot(mine);
            if (mine) events[at + (uint32_t)__popcll(found & below)] = make_event(first, s, op, len, seq, q0);
            at += (uint32_t)__popcll(found);
            anchored = anchored || a != 0;
            rc += __shfl(r_incl, 63, 64);
            qc += __shfl(q_incl, 63, 64);
        }
    }
}

// ---- finish ----
__global__ __launch_bounds__(kThreads) void seq_keys_kernel(const uint4 *__restrict__ events, uint32_t n, uint64_t *__restrict__ key,
                                                            uint32_t *__restrict__ index) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const uint4 e = events[j];
    key[j] = (uint64_t)e.z | (uint64_t)e.w << 32;
    index[j] = (uint32_t)j;
}

__global__ __launch_bounds__(kThreads) void slot_keys_kernel(const uint4 *__restrict__ events, const uint32_t *__restrict__ index, uint32_t n,
                                                             uint64_t *__restrict__ key) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const uint4 e = events[index[j]];
    key[j] = (uint64_t)e.x << 32 | e.y;
}

// head[j] = the event at place j differs from the one before it
__global__ __launch_bounds__(kThreads) void run_heads_kernel(const uint4 *__restrict__ events, const uint32_t *__restrict__ index, uint32_t n,
                                                             uint32_t *__restrict__ head) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    uint32_t h = 1;
    if (j) {
        const uint4 e = events[index[j]], p = events[index[j - 1]];
        h = e.x != p.x || e.y != p.y || e.z != p.z || e.w != p.w;
    }
    head[j] = h;
}

// start[k] = the place of the k-th head, start[the number of heads] = n;  rank is the exclusive scan of head (n + 1 values)
__global__ __launch_bounds__(kThreads) void starts_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ rank, uint32_t n,
                                                          uint32_t *__restrict__ start) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    if (head[j]) start[rank[j]] = (uint32_t)j;
    if (j == 0) start[rank[n]] = n;
}

__device__ __forceinline__ uint32_t ref_of_slot(const uint64_t *__restrict__ ref_base, uint32_t n_ref, uint64_t slot) {
    uint32_t lo = 0, hi = n_ref;                         // the last r with ref_base[r] <= slot
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ref_base[mid] <= slot) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void alleles_kernel(const uint4 *__restrict__ events, const uint32_t *__restrict__ index,
                                                           const uint32_t *__restrict__ start, uint32_t n_alleles,
                                                           const uint64_t *__restrict__ ref_base, uint32_t n_ref, uint4 *__restrict__ out) {
    const uint64_t a = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (a >= n_alleles) return;
    const uint32_t j = start[a];
    const uint4 e = events[index[j]];
    const uint32_t ref = ref_of_slot(ref_base, n_ref, e.x);
    out[2 * a] = make_uint4(ref, (uint32_t)(e.x - ref_base[ref]), e.y, e.z);
    out[2 * a + 1] = make_uint4(e.w, start[a + 1] - j, 0u, 0u);
}

// head[a] = allele a lies on another anchor than the one before it
__global__ __launch_bounds__(kThreads) void anchor_heads_kernel(const uint32_t *__restrict__ alleles, uint32_t n_alleles, uint32_t *__restrict__ head) {
    const uint64_t a = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (a >= n_alleles) return;
    uint32_t h = 1;
    if (a) {
        const uint32_t *x = alleles + a * kAlleleWords, *p = x - kAlleleWords;
        h = x[0] != p[0] || x[1] != p[1];
    }
    head[a] = h;
}

// the inclusive scan of cover in place, wrapping: sums holds the exclusive scan of bm_scan's block sums
__global__ __launch_bounds__(bmscan::kThreads) void cover_scan_kernel(uint32_t *cover, uint64_t n, const uint32_t *__restrict__ sums) {
    __shared__ uint32_t ws[bmscan::kThreads / 64 + 1];
    const uint64_t base = (uint64_t)blockIdx.x * bmscan::kTile + (uint64_t)threadIdx.x * bmscan::kItems;
    uint32_t item[bmscan::kItems], v = 0;
#pragma unroll
    for (int i = 0; i < bmscan::kItems; i++) {
        item[i] = base + i < n ? cover[base + i] : 0u;
        v += item[i];
    }
    uint32_t total;
    uint32_t run = bmscan::block_inclusive<uint32_t>(v, ws, &total) - v + sums[blockIdx.x];
#pragma unroll
    for (int i = 0; i < bmscan::kItems; i++) {
        run += item[i];
        if (base + i < n) cover[base + i] = run;
    }
}

__device__ __forceinline__ uint32_t sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// One thread per anchor, a loop over its alleles (an anchor may have any number).  kEmit false: flag[k] = the anchor is a
// site.  kEmit true: flag is read, rank (its exclusive scan) places the call.
template <bool kEmit>
__global__ __launch_bounds__(kThreads) void calls_kernel(const uint32_t *__restrict__ alleles, const uint32_t *__restrict__ start, uint32_t n_anchors,
                                                         const uint32_t *__restrict__ cover, const uint64_t *__restrict__ ref_base, params pr,
                                                         uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank, uint4 *__restrict__ out) {
    const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n_anchors) return;
    if (kEmit && !flag[k]) return;
    const uint32_t a0 = start[k], a1 = start[k + 1];
    uint64_t E = 0;
    uint32_t n_alt = 0, alt = a0;
    for (uint32_t a = a0; a < a1; a++) {
        const uint32_t *x = alleles + (uint64_t)a * kAlleleWords;
        E += x[5];
        if (!(x[2] & kOther) && x[5] > n_alt) n_alt = x[5], alt = a;   // n >= 1; a tie keeps the first
    }
    const uint32_t *x = alleles + (uint64_t)alt * kAlleleWords;
    const uint32_t D = cover[ref_base[x[0]] + x[1]];
    if (!kEmit) {
        flag[k] = n_alt && D > 0 && n_alt >= pr.min_alt && (uint64_t)n_alt * 1000000ull >= (uint64_t)pr.min_frac_ppm * D;
        return;
    }
    const uint64_t n_ref = D > E ? D - E : 0u;
    const uint64_t L[3] = {100ull * pr.q_indel * n_alt, 301ull * (n_ref + n_alt) + pr.prior, 100ull * pr.q_indel * n_ref + pr.prior};
    uint32_t g = 0;
    if (L[1] < L[g]) g = 1;
    if (L[2] < L[g]) g = 2;
    const uint64_t o1 = L[(g + 1) % 3], o2 = L[(g + 2) % 3], second = o1 < o2 ? o1 : o2;
    const uint64_t gq = (second - L[g]) / 100;
    uint4 *o = out + 4ull * rank[k];
    o[0] = make_uint4(x[0], x[1], x[2], x[3]);
    o[1] = make_uint4(x[4], kGenotyped | (g ? kVariant : 0u), g, gq > 99 ? 99u : (uint32_t)gq);
    o[2] = make_uint4(sat32(L[0] - L[g]), (uint32_t)n_ref, n_alt, sat32(E - n_alt));
    o[3] = make_uint4(D, sat32(L[0] - L[g]), sat32(L[1] - L[g]), sat32(L[2] - L[g]));
}

}  // namespace bmn
