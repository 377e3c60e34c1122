// bmv_clip.hip.h -- the soft-clipping pass of the verifier (bmv_clip, include/bmv.h): of an alignment's columns in
// forward-strand order it keeps the contiguous range [l, r) of greatest score (+match for an `=` column, -penalty for an
// X, I or D column; smallest r, then largest l among equals) and reports the rest of the query as S entries.  A post-pass
// like bmv_annotate, with the same inputs and the same walk (bmv_annotate.hip.h: a wave per alignment, 64 columns of an M
// entry per step, forward-strand order from the start, no LDS, no scratch); no aligning or annotating kernel is touched.
//
// Three walks:
//   range   P[i] = score of columns [0, i).  Per step one ballot of "ranks differ" gives lane i P[col + i + 1] - P[col]
//           from a population count (at most 64 * 1024 in size: 32 bits, packed with the lane as  rel * 64 + 63 - lane);
//           an inclusive prefix-minimum of that key across lanes (the later lane wins ties by its smaller low bits), set
//           against the minimum carried from before the step (the step wins ties: its indices are later); the lane's
//           candidate P[r] - min; a wave maximum of  candidate * 64 + 63 - lane  (the smaller r wins ties), taken only in
//           steps where some lane beats the best so far.  An I or D entry is one element of weight -penalty * length: no
//           border can fall inside it, and its end can only become the new minimum.  Carried in uniform registers: P, the
//           column index, the minimum with its index, the best (score, r, l).  Sums and indices are 64-bit.
//   count   bmv_annotate's walk over the columns of [l, r) only, WRITE = false: nm, pos, ref_len, the clips, the sizes
//   write   the same with WRITE = true, after two exclusive sums (bm_scan.hip.h), S entries first and last
// A non-empty range begins and ends on an `=` column, so it cuts M entries only and the first and last kept runs are `=`.
#pragma once

#include "bmv_annotate.hip.h"

namespace bmv {

constexpr uint32_t kOpS = 4u;

struct ClipJob {
    AnnotateJob a;                  // the inputs, and nm / pos / ref_len / sizes / offsets / xcigar / ref_bases of the kept part
    uint32_t match, penalty;        // 1 .. 1024 each, checked on the host
    int64_t *score;                 // written by the range pass, per alignment ...
    uint64_t *l, *r;
    uint32_t *pos0;                 // ... with the forward-strand start of the whole alignment (bmv_annotate's pos)
    uint32_t *clip_left, *clip_right;   // written by the count pass
};

__device__ __forceinline__ uint32_t clip_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t clip_uniform(uint64_t v) {
    return (uint64_t)clip_uniform((uint32_t)(v >> 32)) << 32 | clip_uniform((uint32_t)v);
}

template <uint32_t WAVES>                                       // alignments per block
__global__ __launch_bounds__(64 * WAVES) void bmv_clip_range_kernel(ClipJob C) {
    const AnnotateJob &J = C.a;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVES + (threadIdx.x >> 6)));
    if (a >= J.count) return;
    const uint64_t cig_at = J.cigar_offset[a];
    const uint32_t ne = (uint32_t)(J.cigar_offset[a + 1] - cig_at);
    const uint32_t *cig = J.cigar + cig_at;
    const bool rc = J.text_rc[a] != 0;
    const uint32_t m = J.query_len[a];
    uint32_t ref_all = 0;                                       // reference bases consumed: M and D lengths
    for (uint32_t k = lane; k < ne; k += 64u) {
        const uint32_t e = cig[k];
        ref_all += (e & 15u) != kOpI ? e >> 4 : 0u;
    }
    ref_all = annotate_wave_sum(ref_all);
    const uint32_t pos0 = ne == 0u ? 0u : (rc ? J.text_len[a] - J.begin[a] - ref_all : J.begin[a]);
    const uint8_t *T = J.genome + J.text_start[a];
    const uint8_t *Q = J.reads + J.query_start[a];
    const int32_t match = (int32_t)C.match, penalty = (int32_t)C.penalty;

    uint32_t ti = pos0, qi = 0;
    uint64_t col = 0;                                           // columns walked so far
    int64_t P = 0;                                              // P[col]
    int64_t min_p = 0;                                          // the least P[0 .. col], at its latest index
    uint64_t min_at = 0;
    int64_t best = 0;                                           // the empty range [0, 0) until a greater score is met
    uint64_t best_l = 0, best_r = 0;
    const uint64_t upto = (2ull << lane) - 1ull;                // lanes 0 .. lane (all of them for lane 63)
    for (uint32_t k = 0; k < ne; k++) {
        const uint32_t e = cig[rc ? ne - 1u - k : k], op = e & 15u, len = e >> 4;
        if (op != 0u) {                                         // I or D: one element, its end may be the new minimum
            P -= (int64_t)penalty * (int64_t)len;
            col += len;
            if (P <= min_p) {
                min_p = P;
                min_at = col;
            }
            if (op == kOpI) qi += len; else ti += len;
            continue;
        }
        auto fetch = [&](uint32_t c) -> uint32_t {              // ranks differ
            if (c + lane >= len) return 0u;
            const uint32_t tr = bmdna::dna4_code(T[ti + c + lane]);
            const uint32_t qx = qi + c + lane;
            const uint32_t qr = rc ? bmdna::dna4_code(Q[m - 1u - qx]) ^ 3u : bmdna::dna4_code(Q[qx]);
            return tr != qr ? 1u : 0u;
        };
        uint32_t cur = fetch(0u);
        for (uint32_t c = 0; c < len; c += 64u) {
            const uint32_t nxt = c + 64u < len ? fetch(c + 64u) : 0u;
            const uint32_t cnt = len - c < 64u ? len - c : 64u;
            const uint64_t x = __ballot(cur != 0u);             // (lanes beyond cnt hold 0: they look like matches and,
                                                                //  being later lanes, change no valid lane's prefix)
            const int32_t nx = (int32_t)__popcll(x & upto);
            const int32_t rel = match * ((int32_t)lane + 1 - nx) - penalty * nx;    // P[col + lane + 1] - P[col]
            int32_t key = rel * 64 + (int32_t)(63u - lane);
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const int32_t o = __shfl_up(key, d, 64);
                if (lane >= d && o < key) key = o;
            }
            const int64_t carried = min_p - P;                  // <= 0: P[col] itself is among the carried
            const int64_t here = (int64_t)(key >> 6);
            const bool in_step = here <= carried;
            const int64_t low = in_step ? here : carried;
            const uint64_t low_at = in_step ? col + (uint64_t)(64u - ((uint32_t)key & 63u)) : min_at;
            const int64_t cand = lane < cnt ? (int64_t)rel - low : -1;
            if (__ballot(cand > best) != 0ull) {
                long long top = (long long)cand * 64 + (long long)(63u - lane);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const long long t = __shfl_xor(top, o, 64);
                    top = t > top ? t : top;
                }
                const uint32_t w = clip_uniform(63u - ((uint32_t)top & 63u));
                best = (int64_t)clip_uniform((uint64_t)(top >> 6));
                best_r = col + w + 1u;
                best_l = clip_uniform((uint64_t)__shfl((long long)low_at, (int)w, 64));
            }
            const int32_t end_key = (int32_t)clip_uniform((uint32_t)__shfl(key, (int)(cnt - 1u), 64));
            const int32_t all_x = (int32_t)__popcll(x);
            if ((int64_t)(end_key >> 6) <= carried) {
                min_p = P + (int64_t)(end_key >> 6);
                min_at = col + (uint64_t)(64u - ((uint32_t)end_key & 63u));
            }
            P += (int64_t)(match * ((int32_t)cnt - all_x) - penalty * all_x);
            col += cnt;
            cur = nxt;
        }
        ti += len;
        qi += len;
    }
    if (lane == 0) {
        C.score[a] = best;
        C.l[a] = best_l;
        C.r[a] = best_r;
        C.pos0[a] = pos0;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(64 * kAnnotateWaves) void bmv_clip_emit_kernel(ClipJob C) {
    const AnnotateJob &J = C.a;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kAnnotateWaves + (threadIdx.x >> 6)));
    if (a >= J.count) return;
    const uint64_t cig_at = J.cigar_offset[a];
    const uint32_t ne = (uint32_t)(J.cigar_offset[a + 1] - cig_at);
    const uint32_t *cig = J.cigar + cig_at;
    const bool rc = J.text_rc[a] != 0;
    const uint32_t m = J.query_len[a];
    const uint64_t l = C.l[a], r = C.r[a];
    uint32_t *out = WRITE ? J.xcigar + J.xcigar_offset[a] : nullptr;
    uint8_t *ref = WRITE ? J.ref_bases + J.ref_offset[a] : nullptr;
    if (ne == 0u || l == r) {                                   // nothing kept: zeros, and the whole query as one S entry
        const uint32_t all = ne == 0u ? 0u : m;
        if (lane == 0) {
            if (!WRITE) {
                J.nm[a] = 0;
                J.pos[a] = 0;
                J.ref_len[a] = 0;
                J.n_xcigar[a] = all ? 1u : 0u;
                J.n_ref[a] = 0;
                C.clip_left[a] = 0;
                C.clip_right[a] = all;
            } else if (all) {
                out[0] = (all << 4) | kOpS;
            }
        }
        return;
    }
    const uint8_t *T = J.genome + J.text_start[a];
    const uint8_t *Q = J.reads + J.query_start[a];
    constexpr uint32_t kLetters = 0x54474341u;                  // "ACGT", rank r in byte r

    uint32_t ti = C.pos0[a], qi = 0;                            // the next text / query base, forward strand
    uint64_t col = 0;
    uint32_t open = 0;                                          // the run not yet written, packed; 0 = none (lengths are > 0)
    uint32_t n_out = 0, n_ref = 0, nm = 0;
    uint32_t clip_left = 0, pos = 0, kept_q = 0, kept_t = 0;
    bool started = false;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t k = 0; k < ne && col < r; k++) {
        const uint32_t e = cig[rc ? ne - 1u - k : k], op = e & 15u, len = e >> 4;
        if (col + len <= l) {                                   // wholly before the range
            if (op != kOpD) qi += len;
            if (op != kOpI) ti += len;
            col += len;
            continue;
        }
        uint32_t from = 0, to = len;                            // the entry's columns inside [l, r)
        if (!started) {                                         // column l: an `=` column of an M entry
            from = (uint32_t)(l - col);
            clip_left = qi + from;
            pos = ti + from;
            started = true;
            if (clip_left) {
                if (WRITE && lane == 0) out[0] = (clip_left << 4) | kOpS;
                n_out = 1;
            }
        }
        if (r - col < (uint64_t)len) to = (uint32_t)(r - col);
        col += len;
        if (op != 0u) {                                         // I or D, whole: closes the open run and is the open run now
            if (open) {
                if (WRITE && lane == 0) out[n_out] = open;
                n_out++;
            }
            open = e;
            nm += len;
            if (op == kOpI) {
                qi += len;
                kept_q += len;
            } else {
                if (WRITE)
                    for (uint32_t x = lane; x < len; x += 64u)
                        ref[n_ref + x] = (uint8_t)(kLetters >> (8u * bmdna::dna4_code(T[ti + x])));
                n_ref += len;
                ti += len;
                kept_t += len;
            }
            continue;
        }
        // an M entry, columns [from, to), 64 a step; packed per lane: bit 0 ranks differ, bits 1-2 the text's rank
        auto fetch = [&](uint32_t c) -> uint32_t {
            if (c + lane >= to) return 0u;
            const uint32_t tr = bmdna::dna4_code(T[ti + c + lane]);
            const uint32_t qx = qi + c + lane;
            const uint32_t qr = rc ? bmdna::dna4_code(Q[m - 1u - qx]) ^ 3u : bmdna::dna4_code(Q[qx]);
            return (tr != qr ? 1u : 0u) | (tr << 1);
        };
        uint32_t cur = fetch(from);
        for (uint32_t c = from; c < to; c += 64u) {
            const uint32_t nxt = c + 64u < to ? fetch(c + 64u) : 0u;
            const uint32_t cnt = to - c < 64u ? to - c : 64u;
            const uint64_t valid = cnt == 64u ? ~0ull : (1ull << cnt) - 1ull;
            const uint64_t x = __ballot((cur & 1u) != 0u);      // (lanes beyond cnt hold 0)
            const uint64_t starts = ((x ^ (x << 1)) | 1ull) & valid;
            const uint32_t runs = (uint32_t)__popcll(starts);
            const uint32_t op0 = (x & 1ull) ? kOpX : kOpEq;
            uint32_t base = n_out, carry = 0;
            if (open) {
                if ((open & 15u) == op0) {
                    carry = open >> 4;                          // the first run continues the open one
                } else {
                    if (WRITE && lane == 0) out[base] = open;
                    base++;
                }
            }
            if (WRITE) {
                const uint32_t rank = (uint32_t)__popcll(starts & below);
                if (((starts >> lane) & 1ull) && rank + 1u < runs) {        // every run but the step's last is complete
                    const uint64_t next = starts & ~((2ull << lane) - 1ull);
                    const uint32_t run_len = (uint32_t)__builtin_ctzll(next) - lane + (rank == 0u ? carry : 0u);
                    out[base + rank] = (run_len << 4) | ((cur & 1u) ? kOpX : kOpEq);
                }
                if (cur & 1u) ref[n_ref + (uint32_t)__popcll(x & below)] = (uint8_t)(kLetters >> (8u * (cur >> 1)));
            }
            const uint32_t last = 63u - (uint32_t)__builtin_clzll(starts);
            open = ((cnt - last + (runs == 1u ? carry : 0u)) << 4) | (((x >> last) & 1ull) ? kOpX : kOpEq);
            n_out = base + runs - 1u;
            const uint32_t nx = (uint32_t)__popcll(x);
            n_ref += nx;
            nm += nx;
            cur = nxt;
        }
        ti += len;
        qi += len;
        kept_q += to - from;
        kept_t += to - from;
    }
    if (open) {
        if (WRITE && lane == 0) out[n_out] = open;
        n_out++;
    }
    const uint32_t clip_right = m - clip_left - kept_q;
    if (clip_right) {
        if (WRITE && lane == 0) out[n_out] = (clip_right << 4) | kOpS;
        n_out++;
    }
    if (!WRITE && lane == 0) {
        J.nm[a] = nm;
        J.pos[a] = pos;
        J.ref_len[a] = kept_t;
        J.n_xcigar[a] = n_out;
        J.n_ref[a] = n_ref;
        C.clip_left[a] = clip_left;
        C.clip_right[a] = clip_right;
    }
}

// instantiated in bmv_clip.hip
extern template __global__ void bmv_clip_range_kernel<kAnnotateWaves>(ClipJob);
extern template __global__ void bmv_clip_emit_kernel<false>(ClipJob);
extern template __global__ void bmv_clip_emit_kernel<true>(ClipJob);

}  // namespace bmv
