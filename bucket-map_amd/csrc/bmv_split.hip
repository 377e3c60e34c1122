// bmv_split.hip -- the range and the pick kernel of bmv_split and bmv_split_pick (bmv_split.hip.h), in a translation unit of
// their own like bmv_clip.hip and bmv_pair.hip: no other kernel's device code is recompiled beside them.
#include "bmv_split.hip.h"

namespace bmv {

template <uint32_t WAVES>                                       // alignments per block
__global__ __launch_bounds__(64 * WAVES) void bmv_split_range_kernel(SplitRangeJob C) {
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

    uint32_t ti = pos0, qi = 0;                                 // the next text / query base, forward strand
    int64_t P = 0;                                              // the score of the columns walked so far
    int64_t min_p = 0;                                          // the least P so far, at its latest border ...
    uint32_t min_ti = pos0, min_qi = 0;                         // ... whose cursors these are
    int64_t best = 0;                                           // the empty range until a greater score is met
    uint32_t l_ti = pos0, l_qi = 0, r_ti = pos0, r_qi = 0;      // the cursors at the best range's two borders
    const uint64_t upto = (2ull << lane) - 1ull;                // lanes 0 .. lane (all of them for lane 63)
    for (uint32_t k = 0; k < ne; k++) {
        const uint32_t e = cig[rc ? ne - 1u - k : k], op = e & 15u, len = e >> 4;
        if (op != 0u) {                                         // I or D: one element, its end may be the new minimum
            P -= (int64_t)penalty * (int64_t)len;
            if (op == kOpI) qi += len; else ti += len;
            if (P <= min_p) {
                min_p = P;
                min_ti = ti;
                min_qi = qi;
            }
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
            const int32_t rel = match * ((int32_t)lane + 1 - nx) - penalty * nx;    // the score from the step's start to behind this lane
            int32_t key = rel * 64 + (int32_t)(63u - lane);     // the prefix minimum of (rel, later lane first)
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const int32_t o = __shfl_up(key, d, 64);
                if (lane >= d && o < key) key = o;
            }
            const int64_t carried = min_p - P;                  // <= 0: the step's own start is among the carried
            const int64_t here = (int64_t)(key >> 6);
            const bool in_step = here <= carried;               // (the step wins ties: its borders are later)
            const int64_t low = in_step ? here : carried;
            const uint32_t low_off = in_step ? 64u - ((uint32_t)key & 63u) : 0u;    // columns from the step's start; 0: carried
            const int64_t cand = lane < cnt ? (int64_t)rel - low : -1;
            if (__ballot(cand > best) != 0ull) {
                long long top = (long long)cand * 64 + (long long)(63u - lane);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const long long t = __shfl_xor(top, o, 64);
                    top = t > top ? t : top;
                }
                const uint32_t w = split_uniform(63u - ((uint32_t)top & 63u));
                best = (int64_t)split_uniform((uint64_t)(top >> 6));
                r_ti = ti + c + w + 1u;
                r_qi = qi + c + w + 1u;
                const uint32_t off = split_uniform(split_lane(low_off, w));
                l_ti = off ? ti + c + off : min_ti;
                l_qi = off ? qi + c + off : min_qi;
            }
            const int32_t end_key = (int32_t)split_uniform(split_lane((uint32_t)key, cnt - 1u));
            const int32_t all_x = (int32_t)__popcll(x);
            if ((int64_t)(end_key >> 6) <= carried) {
                const uint32_t off = 64u - ((uint32_t)end_key & 63u);
                min_p = P + (int64_t)(end_key >> 6);
                min_ti = ti + c + off;
                min_qi = qi + c + off;
            }
            P += (int64_t)(match * ((int32_t)cnt - all_x) - penalty * all_x);
            cur = nxt;
        }
        ti += len;
        qi += len;
    }
    if (lane == 0) {
        const bool kept = best > 0;                             // a non-empty range: it begins and ends on an = column
        const uint32_t cl = kept ? l_qi : 0u, cr = ne == 0u ? 0u : (kept ? m - r_qi : m);
        const uint32_t pos = kept ? l_ti : 0u, ref_len = kept ? r_ti - l_ti : 0u;
        const int64_t g_lo = (int64_t)J.text_start[a] + (int64_t)pos;
        C.score[a] = best;
        C.q_lo[a] = rc ? cr : cl;
        C.q_hi[a] = m - (rc ? cl : cr);
        C.g_lo[a] = g_lo;
        C.g_hi[a] = g_lo + (int64_t)ref_len;
    }
}

template __global__ void bmv_split_range_kernel<kSplitWaves>(SplitRangeJob);

__global__ __launch_bounds__(kSplitWaves * 64) void bmv_split_pick_kernel(SplitPickJob P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t g = split_uniform(blockIdx.x * kSplitWaves + (threadIdx.x >> 6));
    if (g >= P.n_groups) return;
    const uint32_t a0 = split_uniform(P.group_offset[g]), a1 = split_uniform(P.group_offset[g + 1u]);
    const uint32_t ms = P.max_segments;
    SplitCand mine{};                                           // lane k: the k-th chosen alignment ...
    uint32_t mine_at = kSplitBeyond;                            // ... and its batch index
    uint32_t nc = 0;
    for (uint32_t round = 0; round < ms; round++) {
        int64_t bs = kSplitNone;                                // this lane's best alive candidate: its score and index
        uint32_t ba = kSplitBeyond;
        for (uint64_t base = a0; base < a1; base += 64u) {
            const uint64_t a = base + lane;
            const SplitCand c = split_load(P, a, a < a1);
            bool alive = a < a1 && c.s >= P.min_score;
            if (__ballot(alive) == 0ull) continue;              // (the whole wave: base is the same in every lane)
            for (uint32_t k = 0; k < nc; k++) {
                const SplitCand ch = split_broadcast(mine, k);   // (every lane takes part in a broadcast: nothing of it
                const uint32_t ch_at = split_lane(mine_at, k);  //  behind a lane's own condition)
                alive = alive && ch_at != (uint32_t)a && !split_conflict(P, c, ch);
            }
            if (alive && c.s > bs) {                            // (within a lane the indices ascend: the first of equals stays)
                bs = c.s;
                ba = (uint32_t)a;
            }
        }
        // across the wave: the greatest score, then among the lanes that hold it the lowest index
        const int64_t top = (int64_t)split_uniform((uint64_t)split_wave_max(bs));
        if (top == kSplitNone) break;
        uint32_t at = bs == top ? ba : kSplitBeyond;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t t = (uint32_t)__shfl_xor((int)at, o, 64);
            at = t < at ? t : at;
        }
        const uint32_t w = split_uniform(at);
        const SplitCand won = split_load(P, w, true);           // the same words in every lane
        if (lane == nc) {
            mine = won;
            mine_at = w;
        }
        nc++;
    }
    // s2 of every chosen one: the best competitor that is not chosen, is no dup of it and covers half of it
    int64_t s2 = kSplitNone;
    for (uint64_t base = a0; nc != 0u && base < a1; base += 64u) {
        const uint64_t a = base + lane;
        const SplitCand c = split_load(P, a, a < a1);
        bool rival = a < a1 && c.s > 0;
        for (uint32_t k = 0; k < nc; k++) {
            const uint32_t ch_at = split_lane(mine_at, k);      // (read by every lane, also one that is no rival any more:
            rival = rival && ch_at != (uint32_t)a;              //  lane k itself may be one of those)
        }
        if (__ballot(rival) == 0ull) continue;
        for (uint32_t k = 0; k < nc; k++) {
            const SplitCand ch = split_broadcast(mine, k);
            const uint64_t ovl = split_ovl_q(c, ch);
            const bool counts = rival && !split_dup(c, ch, ovl) && 2ull * ovl >= ch.qlen();
            const int64_t v = split_wave_max(counts ? c.s : kSplitNone);
            if (lane == k && v > s2) s2 = v;
        }
    }
    if (lane < ms) {
        const uint64_t slot = (uint64_t)g * ms + lane;
        P.seg[slot] = mine_at;                                  // (kSplitBeyond and kSplitNone in the lanes from nc on)
        P.s2[slot] = s2;
    }
    if (lane == 0) P.n_seg[g] = nc;
}

}  // namespace bmv
