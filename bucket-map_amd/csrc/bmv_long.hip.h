// bmv_long.hip.h -- gfx950 kernels of bmv_align_long (include/bmv.h): alignments beyond the context's limits, of any
// length that fits uint32 and whose trace fits the scratch.
//
// The recurrence, the checkpoints and the tie rules are bmv_align_kernel's (bmv_kernels.hip.h); what changes is who runs
// which part of the matrix.  The query's words are laid over as many lanes as it needs, CW words per lane, and the lanes are
// skewed along the text exactly as in one group of bmv_align_kernel: lane G works on column T - G at time step T.  Those
// lanes are cut into STRIPS of 64 (one wave) and the time axis into CHUNKS of `chunk` steps (a multiple of 16): TILE (s, k)
// is strip s over the steps k * chunk + 1 .. (k + 1) * chunk, one wave.  What a tile needs from outside comes through HBM:
//   - the vertical state (Pv, Mv) of every word at its first step: the checkpoint tile (s, k - 1) stored at its last step;
//   - what left the lane before its first lane at the step before its first (the horizontal delta of that lane's last word,
//     from tile (s, k - 1)'s last delta record);
//   - what leaves the last word of the strip above, one step before this strip's first lane needs it: the delta records of
//     tile (s - 1, k) and, for the first step, (s - 1, k - 1).
// So tile (s, k) depends on tiles with s + k smaller by one or two, and launch d runs every tile with s + k = d of every
// alignment in the piece: no workgroup ever waits for another.  Blocks of 16 time steps never straddle a tile, so the
// checkpoints are exactly what one wave of bmv_align_kernel would store: per alignment, entry (block b, word w) at
// b * W + w -- (Pv, Mv) at the start of block b, and the 16 horizontal deltas leaving word w during block b.
//
// The text is packed once per alignment (2 bits a base, reverse-complemented when asked) and each tile stages the
// chunk + 64 columns it reads into LDS.  The traceback is one LANE per alignment (64 per wave): bmv_align_lane_kernel's
// walk -- 16 columns of one (word, block) recomputed from the checkpoint and kept rotated, diagonal runs read off with one
// bit extraction per column -- over the skewed blocks of bmv_align_kernel.  Run-length CIGAR entries are left in reverse;
// bmv_gather_kernel packs them.
#pragma once

#include "bmv_kernels.hip.h"

namespace bmv {

constexpr int kLongCw = 8;                      // 64-row words per lane: a strip is 512 words, 32 768 query rows

struct LongSlot {
    uint64_t at;                                // byte offset of the alignment's region in the scratch
    uint32_t a;                                 // index of the alignment in the batch
    uint32_t m, n, W;                           // query bases, text bases, 64-row words of the query
    uint32_t n_strips, n_chunks, chunk;         // tiles: strips of 64 lanes, chunks of `chunk` time steps
    uint32_t n_blocks;                          // blocks of 16 time steps with a checkpoint (n_chunks * chunk / 16 + 1)
};

struct LongJob {
    const uint8_t *genome;                      // ASCII
    const uint8_t *reads;                       // ASCII
    const uint8_t *lut;                         // dna4 rank of a char (256 entries)
    const uint64_t *text_start;                 // per alignment of the batch
    const uint8_t *text_rc;
    const uint64_t *query_start;
    const LongSlot *slots;                      // the alignments of this piece
    uint32_t count;
    uint8_t *scratch;                           // one region per slot (long_region_bytes)
    const uint32_t *tiles;                      // this launch's tiles: (slot, strip) pairs
    uint32_t d;                                 // ... with strip + chunk = d
    uint32_t *ops_rev;                          // count x ops_stride reversed CIGAR entries
    uint32_t ops_stride;
    int32_t *out_score;                         // per alignment of the batch
    uint32_t *out_begin;
    uint32_t *out_nops;                         // per slot
};

// A slot's region: checkpoints (Pv, Mv) [block][word], horizontal deltas [block][word], the query's bit planes [word],
// the text as a 2-bit stream (16 columns per 32-bit word, column 16 i + x in bits 2x.. of word i, two words of slack), and
// the bottom row's running minimum (score, best, best column) that the last strip hands from chunk to chunk.
struct LongRegion {
    uint64_t *ckpt;
    uint32_t *hbuf;
    uint64_t *planes;
    uint32_t *text;
    int32_t *state;
};

__host__ __device__ inline uint64_t long_round16(uint64_t b) { return (b + 15u) & ~(uint64_t)15u; }
__host__ __device__ inline uint32_t long_text_words(uint32_t n) { return (uint32_t)(((uint64_t)n + 15u) / 16u) + 2u; }

__host__ __device__ inline uint64_t long_region_bytes(uint32_t W, uint32_t n, uint32_t n_blocks, uint64_t off[5] = nullptr) {
    const uint64_t entries = (uint64_t)n_blocks * W;
    uint64_t o[5];
    o[0] = 0;
    o[1] = o[0] + entries * 16u;
    o[2] = o[1] + long_round16(entries * 4u);
    o[3] = o[2] + (uint64_t)W * 16u;
    o[4] = o[3] + long_round16((uint64_t)long_text_words(n) * 4u);
    if (off)
        for (int k = 0; k < 5; k++) off[k] = o[k];
    return o[4] + 16u;
}

__device__ __forceinline__ LongRegion long_region(uint8_t *scratch, const LongSlot &S) {
    uint64_t o[5];
    long_region_bytes(S.W, S.n, S.n_blocks, o);
    uint8_t *base = scratch + S.at;
    return LongRegion{reinterpret_cast<uint64_t *>(base + o[0]), reinterpret_cast<uint32_t *>(base + o[1]),
                      reinterpret_cast<uint64_t *>(base + o[2]), reinterpret_cast<uint32_t *>(base + o[3]),
                      reinterpret_cast<int32_t *>(base + o[4])};
}

// Set-up of a piece: the query's bit planes and the packed text of every slot, and the bottom row's start (score m at
// column 0).  `per_slot` blocks of 256 threads per slot, each thread a word of the query and a word of the text at a time.
template <int CW>
__global__ __launch_bounds__(256) void bmv_long_prep_kernel(LongJob J, uint32_t per_slot) {
    const uint32_t slot = blockIdx.x / per_slot, part = blockIdx.x % per_slot;
    if (slot >= J.count) return;
    const LongSlot S = J.slots[slot];
    const LongRegion R = long_region(J.scratch, S);
    const uint32_t n = S.n, m = S.m, n_tw = long_text_words(n);
    const uint8_t *q = J.reads + J.query_start[S.a];
    const uint8_t *src = J.genome + J.text_start[S.a];
    const bool rc = J.text_rc[S.a] != 0;
    const uint32_t items = S.W > n_tw ? S.W : n_tw;
    for (uint32_t i = part * 256u + threadIdx.x; i < items; i += per_slot * 256u) {
        if (i < S.W) {
            // rows past the query's end: rank 0 (they compare like any other row; nothing below the last row flows up)
            const uint64_t row0 = (uint64_t)i * 64u;
            const uint32_t rows = m - row0 < 64u ? (uint32_t)(m - row0) : 64u;
            uint64_t p0 = 0, p1 = 0;
            for (uint32_t k = 0; k < rows; k++) {
                const uint64_t r = J.lut[q[row0 + k]];
                p0 |= (r & 1u) << k;
                p1 |= (r >> 1) << k;
            }
            R.planes[2u * (size_t)i] = p0;
            R.planes[2u * (size_t)i + 1u] = p1;
        }
        if (i < n_tw) {
            // text window, reverse-complemented if asked (bucket_locator.h:562-567)
            uint32_t v = 0;
            for (uint32_t x = 0; x < kBlock; x++) {
                const uint64_t j = (uint64_t)i * kBlock + x;
                if (j < n) {
                    const uint32_t r = J.lut[rc ? src[n - 1u - j] : src[j]];
                    v |= (rc ? 3u - r : r) << (2u * x);
                }
            }
            R.text[i] = v;
        }
    }
    if (part == 0 && threadIdx.x == 0) {
        R.state[0] = (int32_t)m;                                // score of column 0: H[m][0] = m
        R.state[1] = (int32_t)m;                                // the minimum so far
        R.state[2] = 0;                                         // ... and its column
    }
}

// One tile (strip s, chunk k) per wave; see the head of this file.  Dynamic LDS: chunk / 16 + 5 words of packed text.
template <int CW>
__global__ __launch_bounds__(kWave) void bmv_long_tile_kernel(LongJob J) {
    extern __shared__ uint32_t lds_words[];
    const uint32_t lane = threadIdx.x;
    const uint32_t slot = J.tiles[2u * blockIdx.x], s = J.tiles[2u * blockIdx.x + 1u], k = J.d - s;
    const LongSlot S = J.slots[slot];
    const LongRegion R = long_region(J.scratch, S);
    const uint32_t n = S.n, m = S.m, W = S.W, C = S.chunk;
    const uint32_t G = s * kWave + lane;                        // the lane among all lanes of the alignment
    const uint32_t wfirst = G * CW;
    const bool holds = wfirst < W;
    const uint32_t T0 = k * C;                                  // steps T0 + 1 .. T0 + C (the host keeps them below 2^32)
    const uint32_t b0 = T0 / kBlock;                            // the tile's first block of 16 steps

    // the text columns this tile reads: 0-based T0 - 64 (s + 1) .. (a multiple of 16), chunk + 64 of them
    const int64_t col0 = (int64_t)T0 - 64 * ((int64_t)s + 1);
    const int64_t qw0 = col0 / (int64_t)kBlock;
    const uint32_t n_lds = C / kBlock + 5u, n_tw = long_text_words(n);
    for (uint32_t x = lane; x < n_lds; x += kWave) {
        const int64_t qw = qw0 + x;
        lds_words[x] = qw >= 0 && qw < (int64_t)n_tw ? R.text[qw] : 0u;
    }
    __syncthreads();

    uint64_t q0[CW], q1[CW], pv[CW], mv[CW];
    uint32_t hacc_p[CW], hacc_m[CW];                            // deltas leaving each word in this block, the latest in bit 0
#pragma unroll
    for (int c = 0; c < CW; c++) {
        const uint32_t w = wfirst + c;
        q0[c] = q1[c] = 0;
        pv[c] = ~0ull;                                          // column 0: H[i][0] = i
        mv[c] = 0;
        hacc_p[c] = hacc_m[c] = 0;
        if (holds && w < W) {
            q0[c] = R.planes[2u * (size_t)w];
            q1[c] = R.planes[2u * (size_t)w + 1u];
            if (k) {                                            // where tile (s, k - 1) left the word
                const uint64_t *ck = R.ckpt + ((size_t)b0 * W + w) * 2u;
                pv[c] = ck[0];
                mv[c] = ck[1];
            }
        }
    }
    // the delta that left this lane's last word at step T0 (in tile (s, k - 1)), for the lane after it
    uint32_t hp_prev = 0, hm_prev = 0;
    if (k && holds && wfirst + CW - 1u < W) {
        const uint32_t rec = R.hbuf[(size_t)(b0 - 1u) * W + wfirst + CW - 1u];   // step 15 of the block: bits 0 and 16
        hp_prev = (rec & 1u) << 31;
        hm_prev = ((rec >> 16) & 1u) << 31;
    }
    // the bottom row: kept by the lane that holds the query's last word, handed from chunk to chunk through the region
    const uint32_t last_word = W - 1u, last_bit = (m - 1u) & 63u, last_c = last_word % CW;
    const bool bottom = holds && last_word / CW == G;
    int32_t score = 0, best = 0;
    uint32_t best_j = 0;
    if (bottom) {
        score = R.state[0];
        best = R.state[1];
        best_j = (uint32_t)R.state[2];
    }
    // above the strip's first word: the last word of the strip above (full, on the lane before), one step earlier
    const uint32_t w_above = wfirst - 1u;
    uint32_t habove = 0, habove_b = 0xFFFFFFFFu;

    for (uint32_t t = 1; t <= C; t++) {
        // what left lane G - 1's last row a step ago: DPP moves down the whole wave by one lane (wave_shr:1)
        uint32_t hpw = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hp_prev, 0x138, 0xF, 0xF, false);
        uint32_t hmw = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hm_prev, 0x138, 0xF, 0xF, false);
        const uint32_t T = T0 + t;
        const uint32_t j = T - G;                               // 1-based text column of this lane (when T > G)
        if (holds && T > G && j <= n) {
            const uint32_t li = t + 63u - lane;                 // j - 1 - col0
            const uint32_t ch = (lds_words[li / kBlock] >> (2u * (li % kBlock))) & 3u;
            const uint64_t nt0 = not_plane((ch & 1u) != 0), nt1 = not_plane((ch & 2u) != 0);
            if (lane == 0) {
                if (s) {
                    // the strip above's last word passed column j at step T - 1 (0-based T - 2): +1 in bit 15 - x, -1 in 31 - x
                    const uint32_t ta = T - 2u, bq = ta / kBlock, x = ta % kBlock;
                    if (bq != habove_b) {
                        habove = R.hbuf[(size_t)bq * W + w_above];
                        habove_b = bq;
                    }
                    hpw = habove << (kBlock + x);
                    hmw = habove << x;
                } else {
                    hpw = hmw = 0;                              // row 0 is all zeros: free leading text gaps
                }
            }
#pragma unroll
            for (int c = 0; c < CW; c++) {
                const uint64_t eq0 = match_rows(q0[c], q1[c], nt0, nt1);
                uint64_t ph, mh, d0;
                myers_step_carry(eq0, hpw, hmw, pv[c], mv[c], ph, mh, d0);
                if ((uint32_t)c == last_c && bottom) {
                    if (CW > 1) asm volatile("" ::: "memory");   // keeps this a branch: not to be if-converted
                    score += (int32_t)((ph >> last_bit) & 1ull) - (int32_t)((mh >> last_bit) & 1ull);
                    if (score <= best) {                        // the LAST minimum of the bottom row
                        best = score;
                        best_j = j;
                    }
                }
                hacc_p[c] = __builtin_amdgcn_alignbit(hacc_p[c], hpw, 31);     // (hacc << 1) | bit 31 of the delta word
                hacc_m[c] = __builtin_amdgcn_alignbit(hacc_m[c], hmw, 31);
            }
            hp_prev = hpw;
            hm_prev = hmw;
        } else if (holds) {
            // a step this lane sits out (before its first column or past the text): its place in the record stays empty
#pragma unroll
            for (int c = 0; c < CW; c++) {
                hacc_p[c] <<= 1;
                hacc_m[c] <<= 1;
            }
        }
        // end of a block of 16 steps, for the whole wave at once (chunks are multiples of 16)
        if (t % kBlock == 0u) {
            const uint32_t bt = b0 + (t - 1u) / kBlock;
#pragma unroll
            for (int c = 0; c < CW; c++) {
                const uint32_t w = wfirst + c;
                if (holds && w < W) {
                    const size_t e = (size_t)bt * W + w;
                    R.hbuf[e] = (hacc_p[c] & 0xFFFFu) | (hacc_m[c] << 16);   // step x at bit 15 - x (+1), 31 - x (-1)
                    uint64_t *ck = R.ckpt + (e + W) * 2u;                   // the state block bt + 1 starts from
                    ck[0] = pv[c];
                    ck[1] = mv[c];
                }
                hacc_p[c] = hacc_m[c] = 0;
            }
        }
    }
    if (bottom) {
        R.state[0] = score;
        R.state[1] = best;
        R.state[2] = (int32_t)best_j;
    }
}

// Traceback, one alignment per lane: from the LAST minimum of the bottom row, diagonal first, then up, then left
// (include/bmv.h, rules 1-2), in rounds of one (word, block) cell recomputed from its checkpoint.
template <int CW>
__global__ __launch_bounds__(kWave) void bmv_long_traceback_kernel(LongJob J) {
    const uint32_t slot = blockIdx.x * kWave + threadIdx.x;
    if (slot >= J.count) return;
    const LongSlot S = J.slots[slot];
    const LongRegion R = long_region(J.scratch, S);
    const uint32_t n = S.n, m = S.m, W = S.W;
    const int32_t best = R.state[1];
    uint64_t D[kBlock], U[kBlock];                              // rotated: bit (r - x) & 63 of [x] is row r of column x
    uint32_t *ops = J.ops_rev + (size_t)slot * J.ops_stride;
    uint32_t i = m, j = (uint32_t)R.state[2], n_rev = 0, cur_op = 3, cur_len = 0;
    auto emit = [&](uint32_t op, uint32_t len) {
        if (op == cur_op) {
            cur_len += len;
        } else {
            if (cur_len) ops[n_rev++] = (cur_len << 4) | cur_op;
            cur_op = op;
            cur_len = len;
        }
    };
    while (i > 0) {
        uint32_t wc = 0, bc = 0;
        if (j > 0) {
            // the cell (word, block of 16 time steps) the walk stands in: word wc sits on lane wc / CW and passes column j at
            // step j + wc / CW
            wc = (i - 1u) >> 6;
            const uint32_t lw = wc / CW;
            bc = (j + lw - 1u) / kBlock;
            uint64_t kpv = ~0ull, kmv = 0ull;                   // block 0 starts from column 0: H[i][0] = i
            if (bc) {
                const uint64_t *ck = R.ckpt + ((size_t)bc * W + wc) * 2u;
                kpv = ck[0];
                kmv = ck[1];
            }
            // the deltas entering the word at the block's 16 steps = those that left the word above at the same COLUMNS: the
            // same steps if it sits on the same lane, one step earlier if on the lane before (row 0 above word 0: zeros)
            uint32_t hw = 0;
            if (wc) {
                const uint32_t cur = R.hbuf[(size_t)bc * W + wc - 1u];
                if ((wc - 1u) / CW == lw) {
                    hw = cur;
                } else {
                    const uint32_t before = bc ? R.hbuf[(size_t)(bc - 1u) * W + wc - 1u] : 0u;
                    hw = ((cur >> 1) & 0x7FFF7FFFu) | ((before & 0x00010001u) << 15);
                }
            }
            const uint64_t p0 = R.planes[2u * (size_t)wc], p1 = R.planes[2u * (size_t)wc + 1u];
            // the block's 16 text bases: columns 16 bc + 1 - lw + x, out of two words of the 2-bit stream
            const int64_t c0 = (int64_t)bc * kBlock - (int64_t)lw;  // 0-based column of x = 0 (may be negative)
            const int64_t tq = c0 >> 4;                         // floor
            const uint32_t tsh = (uint32_t)(c0 & 15);
            const uint32_t tlo = tq >= 0 ? R.text[tq] : 0u, thi = tq + 1 >= 0 ? R.text[tq + 1] : 0u;
            const uint32_t tw = tsh ? (tlo >> (2u * tsh)) | (thi << (32u - 2u * tsh)) : tlo;
#pragma unroll
            for (int x = 0; x < (int)kBlock; x++) {
                const int64_t col = c0 + 1 + x;                 // 1-based
                D[x] = U[x] = 0;
                if (col >= 1 && col <= (int64_t)n) {
                    const uint64_t eq0 = match_rows(p0, p1, not_plane(((tw >> (2 * x)) & 1u) != 0), not_plane(((tw >> (2 * x + 1)) & 1u) != 0));
                    uint32_t hpw = hw << (x + (int)kBlock), hmw = hw << x;    // the step's bits to bit 31
                    uint64_t ph, mh, d0;
                    myers_step_carry(eq0, hpw, hmw, kpv, kmv, ph, mh, d0);
                    D[x] = rotr64(~(eq0 ^ d0), (uint32_t)x);    // diagonal predecessor valid
                    U[x] = rotr64(kpv, (uint32_t)x);            // upper predecessor valid
                }
            }
        }
        while (i > 0) {
            if (j == 0) {                                       // column 0: only upper predecessors, all the way
                emit(1u, i);
                i = 0;
                break;
            }
            const uint32_t w = (i - 1u) >> 6, tcol = j + w / CW - 1u;
            if (w != wc || tcol / kBlock != bc) break;          // left the cell: next round
            // diagonal first, as far as it goes: the cells (i - r, j - r) sit at bit `at` of columns x - r
            const uint32_t x = tcol % kBlock, bit = (i - 1u) & 63u, at = (bit - x) & 63u;
            uint32_t room = x < bit ? x : bit;                  // cells of this diagonal inside the word, the block and the text
            room = (room < j - 1u ? room : j - 1u) + 1u;
            const uint32_t gaps = ~gather_bit(D, at) & ((2u << x) - 1u);
            uint32_t run = gaps ? x - (31u - (uint32_t)__builtin_clz(gaps)) : x + 1u;
            run = run < room ? run : room;
            if (run) {
                emit(0u, run);
                i -= run;
                j -= run;
            }
            if (run < room) {                                   // stopped by a cell whose diagonal predecessor is not valid
                if ((gather_bit(U, at) >> (x - run)) & 1u) {
                    emit(1u, 1u);
                    i--;
                } else {
                    emit(2u, 1u);
                    j--;
                }
            }
        }
    }
    if (cur_len) ops[n_rev++] = (cur_len << 4) | cur_op;
    J.out_score[S.a] = -best;
    J.out_begin[S.a] = j;
    J.out_nops[slot] = n_rev;
}

// instantiated in bmv_long.hip
extern template __global__ void bmv_long_prep_kernel<kLongCw>(LongJob, uint32_t);
extern template __global__ void bmv_long_tile_kernel<kLongCw>(LongJob);
extern template __global__ void bmv_long_traceback_kernel<kLongCw>(LongJob);

}  // namespace bmv
