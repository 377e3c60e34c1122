// bmv_screen.hip.h -- score-only screen of bmv_align_bounded (include/bmv.h): which alignments of a batch can NOT have a
// semi-global edit distance within their bound k.  Same recurrence (myers_step_carry), same dna4 folding table and the same
// reverse complement of the text as the aligning kernels in bmv_kernels.hip.h; no checkpoints, no deltas, no CIGAR scratch.
//
// Ukkonen's cut-off at the lower end of the column.  The band of a column is the query's words 0 .. nw - 1; the invariant is
// that every cell below the band has D > k, and by induction every cell IN the band with D <= k is exact and every other one
// is not below its true value (its best predecessor is then itself <= k, so in the band and exact; what comes from outside
// is an upper bound).  B is the computed score of the band's bottom row.
//   * A word is brought in for column j when B <= k in column j - 1 (only then can its first row be <= k in column j: the
//     upper neighbour is >= k, the diagonal one is B, the left one is outside).  It starts from upper bounds: vertical
//     deltas all +1 below B.  B moves by at most one per column, so one word per column is enough.
//   * A word is left out when its bottom row is >= k + 64: vertical deltas are at most 1, so all its 64 cells are > k.
//   * With B > k the last row la with D <= k is at most 64 nw - (B - k).  When m - la > n - j the alignment is REJECTED: a
//     path within k through column j passes it at a row i with D = d <= k, the rows below it rise by at most one each, so
//     la >= i + (k - d), and the path still needs (m - i) - (n - j) <= k - d insertions.  That speaks of paths THROUGH column
//     j only: an alignment may have ended in an earlier column.  So the bottom row is watched as well: once the band holds
//     the query's last word and B <= k + (64 W - m) -- row m may be within k; the rows past the query's end add at most one
//     each -- the alignment is let through at once and never rejected.
// The screen only ever rejects; what it lets through is aligned in full and the bound is applied to that score, so an
// alignment the screen gives up on (the band outgrows what the kernel holds) costs time, never correctness.
//
// Two mappings.  Queries of up to 512 bases: one alignment per lane as in bmv_align_lane_kernel, the text fetched by the
// whole wave 64 columns at a time while any lane still needs it.  Longer queries: ONE alignment per wave, CW words per lane,
// lanes skewed along the text (lane l is at column t - l), the band growing downwards lane by lane; the wave leaves at the
// step its alignment is decided, so the alignments of a batch never wait for each other -- the skewed groups of
// bmv_align_kernel would keep a wave until its slowest alignment is done, and at 4 of 5 wrong loci that is nearly always a
// true one.  The band of a wrong locus is about 2 k rows; the host picks CW so that 64 CW words hold it.
#pragma once

#include "bmv_kernels.hip.h"

namespace bmv {

struct ScreenJob {
    const uint8_t *genome;
    const uint8_t *reads;
    const uint8_t *lut;
    const uint64_t *text_start;     // per alignment of the batch
    const uint32_t *text_len;
    const uint8_t *text_rc;
    const uint64_t *query_start;
    const uint32_t *query_len;
    const uint32_t *max_edits;
    const uint32_t *list;           // this launch screens alignments list[0 .. count)
    uint32_t count;
    uint32_t *keep;                 // per alignment of the batch: set to 0 when rejected
    unsigned long long *cells;      // += (64-row word, text column) steps evaluated
};

constexpr uint32_t kScreenEvery = 16;   // columns between the lane kernel's drop / reject / leave checks

__device__ __forceinline__ int32_t hdelta(uint32_t hpw, uint32_t hmw) { return (int32_t)(hpw >> 31) - (int32_t)(hmw >> 31); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) v += shfl64(v, (int)((threadIdx.x & 63u) ^ (uint32_t)o));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// One alignment per lane, queries of up to 64 * CW bases, texts of any length.
// ---------------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(kWave) void bmv_screen_lane_kernel(ScreenJob J) {
    __shared__ uint32_t lut_w[64];
    __shared__ uint32_t text_planes[kWave * 4];                 // per alignment: the low and the high plane of 64 columns
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lut_w);
    const uint32_t lane = threadIdx.x, slot = blockIdx.x * kWave + lane;
    const bool have = slot < J.count;
    const uint32_t a = J.list[have ? slot : 0u];
    const uint32_t n = have ? J.text_len[a] : 0u, m = have ? J.query_len[a] : 0u;
    const int32_t k = have ? (int32_t)J.max_edits[a] : 0;       // (the host screens only k < m <= 512)
    const uint32_t W = (m + 63u) >> 6;
    lut_w[lane] = reinterpret_cast<const uint32_t *>(J.lut)[lane];
    __syncthreads();

    // the query's bit planes, lane by lane's own (rows past the end: rank 0, as in the aligning kernels)
    uint64_t q0[CW], q1[CW];
#pragma unroll
    for (int c = 0; c < CW; c++) {
        uint64_t p0 = 0, p1 = 0;
        if ((uint32_t)c < W) {
            const uint32_t row0 = (uint32_t)c * 64u, rows = m - row0 < 64u ? m - row0 : 64u;
            const uint8_t *q = J.reads + J.query_start[a] + row0;
#pragma unroll 8
            for (uint32_t r = 0; r < 64u; r++) {
                const uint64_t v = r < rows ? lut[q[r]] : 0u;
                p0 |= (v & 1u) << r;
                p1 |= (v >> 1) << r;
            }
        }
        q0[c] = p0;
        q1[c] = p1;
    }
    const uint64_t t_at = have ? J.text_start[a] : 0u;
    const uint32_t rc = have ? J.text_rc[a] : 0u;

    uint64_t pv[CW], mv[CW];
#pragma unroll
    for (int c = 0; c < CW; c++) {
        pv[c] = ~0ull;                                          // column 0: H[i][0] = i
        mv[c] = 0;
    }
    // column 0: rows 1 .. k are within the bound
    uint32_t nw = W ? ((uint32_t)k / 64u + 1u < W ? (uint32_t)k / 64u + 1u : W) : 0u;
    int32_t B = (int32_t)(64u * nw);
    bool rejected = false;
    auto reject_test = [&](uint32_t j) {
        if (W && B > k && (int32_t)m - ((int32_t)(64u * nw) - (B - k)) > (int32_t)n - (int32_t)j) rejected = true;
    };
    reject_test(0u);                                            // (a text too short for the query within k insertions)
    const int32_t reached = k + (int32_t)(64u * W - m);         // B at or below this in the last word: row m may be within k
    bool active = have && W != 0u && n != 0u && !rejected;
    uint32_t steps = active ? n : 0u;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)steps, o, kWave);
        steps = other > steps ? other : steps;
    }
    unsigned long long my_cells = 0;
    uint64_t tlo = 0, thi = 0;
    uint32_t wave_nw = CW;
    for (uint32_t t = 1; t <= steps; t++) {
        const uint32_t x = (t - 1u) & 63u;
        if (x == 0u) {
            // the next 64 columns of every alignment still running, fetched by the whole wave (one line per alignment),
            // reverse-complemented if asked (bucket_locator.h:562-567)
            const uint64_t running = __ballot(active);
            __syncthreads();
            // (eight alignments' loads in flight at a time, none under a condition: a lane past a window's end reads its last
            // base again, an alignment that is not running the byte its window begins at -- the genome has slack for that)
            for (uint32_t g0 = 0; g0 < kWave; g0 += 8u) {
                if (((running >> g0) & 0xFFull) == 0ull) continue;
                uint32_t raw[8];
#pragma unroll
                for (uint32_t u = 0; u < 8u; u++) {
                    const uint32_t g = g0 + u;
                    const uint32_t ng = (uint32_t)__builtin_amdgcn_readlane((int)n, (int)g);
                    const uint8_t *src = J.genome + readlane64(t_at, g);
                    const bool rcg = __builtin_amdgcn_readlane((int)rc, (int)g) != 0;
                    const uint32_t last = ng ? ng - 1u : 0u;
                    uint32_t col = t - 1u + lane;               // 0-based, clamped into the window
                    col = col < last ? col : last;
                    raw[u] = src[rcg ? last - col : col];
                }
#pragma unroll
                for (uint32_t u = 0; u < 8u; u++) {
                    const uint32_t g = g0 + u;
                    const bool rcg = __builtin_amdgcn_readlane((int)rc, (int)g) != 0;
                    const uint32_t r = lut[raw[u]] ^ (rcg ? 3u : 0u);
                    const uint64_t lo = __ballot((r & 1u) != 0), hi = __ballot((r & 2u) != 0);
                    if (lane == 0) {
                        text_planes[4u * g + 0u] = (uint32_t)lo;
                        text_planes[4u * g + 1u] = (uint32_t)(lo >> 32);
                        text_planes[4u * g + 2u] = (uint32_t)hi;
                        text_planes[4u * g + 3u] = (uint32_t)(hi >> 32);
                    }
                }
            }
            __syncthreads();
            tlo = ((uint64_t)text_planes[4u * lane + 1u] << 32) | text_planes[4u * lane];
            thi = ((uint64_t)text_planes[4u * lane + 3u] << 32) | text_planes[4u * lane + 2u];
        }
        // a word brought in for this column: upper bounds below B (rare: a branch of the whole wave)
        const bool grow = active && nw < W && B <= k;
        if (__ballot(grow) != 0ull) {
            if (grow) {
#pragma unroll
                for (int c = 1; c < CW; c++) {
                    if ((uint32_t)c == nw) {
                        pv[c] = ~0ull;
                        mv[c] = 0;
                    }
                }
                nw++;
                B += 64;
            }
            wave_nw = CW;                                       // (recounted at the next check)
        }
        if (active) {
            const uint64_t nt0 = not_plane(((tlo >> x) & 1ull) != 0), nt1 = not_plane(((thi >> x) & 1ull) != 0);
            uint32_t hpw = 0, hmw = 0;                          // row 0 is all zeros: free leading text gaps
#pragma unroll
            for (int c = 0; c < CW; c++) {
                if ((uint32_t)c >= wave_nw) break;
                if ((uint32_t)c < nw) {
                    const uint64_t eq0 = match_rows(q0[c], q1[c], nt0, nt1);
                    uint64_t ph, mh, d0;
                    myers_step_carry(eq0, hpw, hmw, pv[c], mv[c], ph, mh, d0);
                }
            }
            B += hdelta(hpw, hmw);                              // what left the band's last word
            my_cells += nw;
            // through the text without a rejection, or the bottom row may have been reached within k: let through
            if (t == n || (nw == W && B <= reached)) active = false;
        }
        if ((t & (kScreenEvery - 1u)) == 0u) {
            if (active) {
#pragma unroll
                for (int c = CW - 1; c >= 1; c--) {
                    if ((uint32_t)c + 1u == nw && B >= k + 64) {
                        const int32_t above = B - (int32_t)__popcll(pv[c]) + (int32_t)__popcll(mv[c]);
                        if (above > k) {                        // (else the next column would bring it back)
                            nw--;
                            B = above;
                        }
                    }
                }
                reject_test(t);
                if (rejected) active = false;
            }
            uint32_t mx = active ? nw : 0u;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t other = (uint32_t)__shfl_xor((int)mx, o, kWave);
                mx = other > mx ? other : mx;
            }
            wave_nw = (uint32_t)__builtin_amdgcn_readfirstlane((int)mx);
            if (wave_nw == 0u) break;                           // every alignment of the wave is decided
        }
        // (words may have been brought in since the last check: wave_nw is CW until the next one)
        if (__ballot(active) == 0ull) break;
    }
    if (have && rejected) J.keep[a] = 0u;
    const unsigned long long total = wave_sum(my_cells);
    if (lane == 0 && total) atomicAdd(J.cells, total);
}

// ---------------------------------------------------------------------------------------------------------------------
// One alignment per wave: lane l holds words l * CW .. l * CW + CW - 1 and is at column t - l at step t.  The band only
// grows here (a word that is in stays in).  `on` is how many of the lane's words are in the band; the band is a prefix of
// the query's words, so a lane's own B -- the bottom of its last word that is in -- is the band's B whenever nothing below
// the lane is in.  What travels to the next lane each step: the horizontal delta of the lane's last row, the text base, and
// -- when the lane is full and its B <= k -- B + 1, the call to come in.
// ---------------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(kWave) void bmv_screen_wave_kernel(ScreenJob J) {
    __shared__ uint32_t lut_w[64];
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lut_w);
    const uint32_t lane = threadIdx.x;
    const uint32_t a = J.list[blockIdx.x];                      // (grid = count)
    const uint32_t n = J.text_len[a], m = J.query_len[a];
    const int32_t k = (int32_t)J.max_edits[a];                  // (the host screens only k < m <= 65 536)
    const uint32_t W = (m + 63u) >> 6;
    const uint32_t cap = W < 64u * CW ? W : 64u * CW;           // words this wave can hold
    lut_w[lane] = reinterpret_cast<const uint32_t *>(J.lut)[lane];
    __syncthreads();
    const uint32_t nw0 = (uint32_t)k / 64u + 1u < W ? (uint32_t)k / 64u + 1u : W;      // column 0: rows 1 .. k
    // a text too short for the query within k insertions; a band that does not fit from the start: let through
    if ((int32_t)m - k > (int32_t)n) {
        if (lane == 0) J.keep[a] = 0u;
        return;
    }
    if (nw0 > cap || n == 0u) return;

    uint64_t q0[CW], q1[CW], pv[CW], mv[CW];
#pragma unroll
    for (int c = 0; c < CW; c++) {
        uint64_t p0 = 0, p1 = 0;
        const uint32_t w = lane * CW + (uint32_t)c;
        if (w < cap) {
            const uint32_t row0 = w * 64u, rows = m - row0 < 64u ? m - row0 : 64u;
            const uint8_t *q = J.reads + J.query_start[a] + row0;
#pragma unroll 8
            for (uint32_t r = 0; r < 64u; r++) {
                const uint64_t v = r < rows ? lut[q[r]] : 0u;
                p0 |= (v & 1u) << r;
                p1 |= (v >> 1) << r;
            }
        }
        q0[c] = p0;
        q1[c] = p1;
        pv[c] = ~0ull;                                          // column 0: H[i][0] = i
        mv[c] = 0;
    }
    const uint8_t *src = J.genome + J.text_start[a];
    const bool rc = J.text_rc[a] != 0;
    const int32_t reached = k + (int32_t)(64u * W - m);         // B at or below this in the last word: row m may be within k
    const uint32_t w_first = lane * CW;
    uint32_t on = nw0 > w_first ? (nw0 - w_first < CW ? nw0 - w_first : CW) : 0u;
    int32_t B = (int32_t)(64u * (w_first + on));
    bool below_on = nw0 > w_first + CW;                         // words of the next lanes are in
    uint32_t hp_prev = 0, hm_prev = 0, ch_prev = 0, call_prev = 0;
    uint32_t chunk = 0;                                         // ranks of 64 text columns, column 64 q + lane
    bool rejected = false, leave = false;
    unsigned long long my_cells = 0;
    const uint32_t steps = n + (cap + CW - 1u) / CW - 1u;
    for (uint32_t t = 1; t <= steps; t++) {
        if (((t - 1u) & 63u) == 0u) {
            uint32_t col = t - 1u + lane;                       // 0-based, clamped into the window
            col = col < n ? col : n - 1u;
            chunk = lut[src[rc ? n - 1u - col : col]] ^ (rc ? 3u : 0u);
        }
        // from the lane before: what it produced a step ago (wave_shr:1; lane 0 takes the text and row 0's zeros)
        uint32_t hpw = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hp_prev, 0x138, 0xF, 0xF, false);
        uint32_t hmw = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hm_prev, 0x138, 0xF, 0xF, false);
        uint32_t ch = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ch_prev, 0x138, 0xF, 0xF, false);
        const uint32_t call = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)call_prev, 0x138, 0xF, 0xF, false);
        const uint32_t fresh = (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)((t - 1u) & 63u));
        if (lane == 0) {
            ch = fresh;
            hpw = hmw = 0;
        }
        ch_prev = ch;
        const uint32_t j = t - lane;                            // 1-based text column of this lane
        call_prev = 0;
        if (on != 0u && t > lane && j <= n) {
            const uint64_t nt0 = not_plane((ch & 1u) != 0), nt1 = not_plane((ch & 2u) != 0);
#pragma unroll
            for (int c = 0; c < CW; c++) {
                if ((uint32_t)c < on) {
                    const uint64_t eq0 = match_rows(q0[c], q1[c], nt0, nt1);
                    uint64_t ph, mh, d0;
                    myers_step_carry(eq0, hpw, hmw, pv[c], mv[c], ph, mh, d0);
                }
            }
            hp_prev = hpw;
            hm_prev = hmw;
            B += hdelta(hpw, hmw);
            my_cells += on;
            const uint32_t in = w_first + on;                   // words of the band down to this lane's last
            if (in == W && B <= reached) leave = true;          // the bottom row may have been reached within k: let through
            if (B <= k) {
                // the next word comes in for column j + 1, from upper bounds below B
                if (in >= cap) {
                    if (cap < W) leave = true;                  // the band outgrows the wave: let through
                } else if (on < CW) {
#pragma unroll
                    for (int c = 1; c < CW; c++) {
                        if ((uint32_t)c == on) {
                            pv[c] = ~0ull;
                            mv[c] = 0;
                        }
                    }
                    on++;
                    B += 64;
                } else {
                    call_prev = (uint32_t)B + 1u;
                    below_on = true;
                }
            } else if (!leave && !(on == CW && below_on)) {
                // this lane's last word is the band's: la <= 64 in - (B - k)
                if ((int32_t)m - ((int32_t)(64u * in) - (B - k)) > (int32_t)n - (int32_t)j) rejected = true;
            }
            if (j == n && !(on == CW && below_on)) leave = true;   // the band's end has passed the text: let through
        } else if (on == 0u && call != 0u) {
            // called in by the lane before, which has just passed the column this lane is at: the first word starts from
            // upper bounds there and runs from the next step on
            on = 1u;
            B = (int32_t)call - 1 + 64;
        }
        if (__ballot(rejected || leave) != 0ull) break;
    }
    if (__ballot(rejected) != 0ull && lane == 0) J.keep[a] = 0u;
    const unsigned long long total = wave_sum(my_cells);
    if (lane == 0 && total) atomicAdd(J.cells, total);
}

// survivors' indices in batch order: where[a] is the exclusive sum of keep (defined in bmv_screen.hip)
__global__ void bmv_screen_compact_kernel(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ where, uint32_t n,
                                          uint32_t *__restrict__ out);

// instantiated in bmv_screen.hip
extern template __global__ void bmv_screen_lane_kernel<1>(ScreenJob);
extern template __global__ void bmv_screen_lane_kernel<2>(ScreenJob);
extern template __global__ void bmv_screen_lane_kernel<3>(ScreenJob);
extern template __global__ void bmv_screen_lane_kernel<4>(ScreenJob);
extern template __global__ void bmv_screen_lane_kernel<5>(ScreenJob);
extern template __global__ void bmv_screen_lane_kernel<6>(ScreenJob);
extern template __global__ void bmv_screen_lane_kernel<7>(ScreenJob);
extern template __global__ void bmv_screen_lane_kernel<8>(ScreenJob);
extern template __global__ void bmv_screen_wave_kernel<1>(ScreenJob);
extern template __global__ void bmv_screen_wave_kernel<2>(ScreenJob);
extern template __global__ void bmv_screen_wave_kernel<4>(ScreenJob);

}  // namespace bmv
