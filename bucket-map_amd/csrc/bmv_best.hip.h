// bmv_best.hip.h -- the distance round and the pick of bmv_align_best (include/bmv.h): of a read's candidate alignments only
// the best needs a traceback; every other one needs its exact semi-global edit distance d and end column, or the proof that
// d lies beyond k = (the seed's edits) + margin.
//
// The distance kernels are the score-only screen of bmv_align_bounded (bmv_screen.hip.h: the same recurrence, the same
// Ukkonen cut-off at the lower end of the column, the same two mappings) made to DECIDE instead of to reject.  They rest on
// the screen's invariant -- every cell below the band has D > k; every cell IN the band with D <= k is exact and every other
// one is not below its true value -- and differ in what they do with it:
//   * They watch row m, the query's last, while the band holds it: its computed score s is kept along (from the horizontal
//     delta of its bit in the last word), and a column with s <= k -- then s is exact -- goes into a running minimum in which
//     a tie is won by the LATER column: tie rule (1) of bmv.h, so the column is the alignment's exclusive end, begin + R.
//     A column in which the band does not hold row m, or holds it with s > k, has D[m][j] > k by the invariant.
//   * They run to the text's last column and leave early only on the screen's rejection test, which says that no path within
//     k passes through column j or any later one (row 0 is free, so a path that begins later passes column j in row 0): the
//     running minimum of the columns before j is then final.
//   * The wave kernel's band only grows.  When it would outgrow the wave's 64 * CW words the alignment is UNDECIDED and the
//     host sends it through the full aligner: time, never correctness.  The rejection test fires in the lane that holds the
//     band's bottom; when that lane is above the one holding row m, row m has never been in the band and the answer is
//     "beyond"; when it is that lane, the minimum is its own and complete up to its column.
// Copied from the screen rather than shared with it (as bmv_clip copied bmv_annotate's walk): the screen's device code stays
// what it was.  Results are plain vector stores.
//
// The pick: a segmented pass over the groups.  A lane takes a group of up to 64 members, the whole wave one beyond that.  It
// finds best = min d, the winner as the minimum over (d, batch index), masks edits / end to d <= best + margin, and flags the
// groups whose winner has no full alignment yet (bm_scan.hip.h then compacts them).
#pragma once

#include "bmv_kernels.hip.h"

namespace bmv {

constexpr uint32_t kBestBeyond = 0xFFFFFFFFu;       // BMV_BEYOND
constexpr uint32_t kBestUndecided = 0xFFFFFFFEu;    // (never leaves the library: such alignments are aligned in full)

struct BestJob {
    const uint8_t *genome;
    const uint8_t *reads;
    const uint8_t *lut;
    const uint64_t *text_start;     // per alignment of the batch
    const uint32_t *text_len;
    const uint8_t *text_rc;
    const uint64_t *query_start;
    const uint32_t *query_len;
    const uint32_t *bound;          // k per alignment, <= query_len
    const uint32_t *list;           // this launch decides alignments list[0 .. count)
    uint32_t count;
    uint32_t *d;                    // per alignment of the batch: the distance, kBestBeyond or kBestUndecided
    uint32_t *end;                  // the exclusive end column (0 unless d is a distance)
    unsigned long long *cells;      // += (64-row word, text column) steps evaluated
};

struct PickJob {
    const uint32_t *d;              // per alignment: a distance or kBestBeyond
    const uint32_t *end;
    const uint32_t *full;           // per alignment: != 0 when its full alignment is at hand (seeds, undecided ones)
    const uint32_t *group_offset;   // n_groups + 1
    const uint32_t *margin;         // n_groups
    uint32_t n_groups;
    uint32_t *winner;               // n_groups
    uint32_t *need;                 // n_groups: 1 when the winner still has to be aligned in full
    uint32_t *out_edits;            // per alignment
    uint32_t *out_end;
};

constexpr uint32_t kBestEvery = 16;     // columns between the lane kernel's drop / reject / leave checks

__device__ __forceinline__ int32_t best_hdelta(uint32_t hpw, uint32_t hmw) { return (int32_t)(hpw >> 31) - (int32_t)(hmw >> 31); }

__device__ __forceinline__ unsigned long long best_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) v += shfl64(v, (int)((threadIdx.x & 63u) ^ (uint32_t)o));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// One alignment per lane, queries of 1 .. 64 * CW bases, texts of 1 base and more.  A lane holds every word of its query, so
// nothing is ever undecided here.
// ---------------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(kWave) void bmv_best_lane_kernel(BestJob J) {
    __shared__ uint32_t lut_w[64];
    __shared__ uint32_t text_planes[kWave * 4];                 // per alignment: the low and the high plane of 64 columns
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lut_w);
    const uint32_t lane = threadIdx.x, slot = blockIdx.x * kWave + lane;
    const bool have = slot < J.count;
    const uint32_t a = J.list[have ? slot : 0u];
    const uint32_t n = have ? J.text_len[a] : 0u, m = have ? J.query_len[a] : 0u;
    const int32_t k = have ? (int32_t)J.bound[a] : 0;           // (the host sends 1 <= m <= 64 CW, k <= m)
    const uint32_t W = (m + 63u) >> 6;
    const uint32_t last_w = W ? W - 1u : 0u, last_bit = (m - 1u) & 63u;     // where row m lives
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
    int32_t sm = (int32_t)m;                                    // row m's computed score; means something while nw == W
    uint32_t best_d = kBestBeyond, best_end = 0u;               // (column 0 never wins: D[m][j] <= m = D[m][0] for every j)
    bool rejected = false;
    auto reject_test = [&](uint32_t j) {
        if (W && B > k && (int32_t)m - ((int32_t)(64u * nw) - (B - k)) > (int32_t)n - (int32_t)j) rejected = true;
    };
    reject_test(0u);                                            // (a text too short for the query within k insertions)
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
            // reverse-complemented if asked; a lane past a window's end reads its last base again, an alignment that is not
            // running the byte its window begins at (the genome has slack for that)
            const uint64_t running = __ballot(active);
            __syncthreads();
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
                if (nw == last_w) sm = B + (int32_t)last_bit + 1;   // row m comes in: one more per row below B
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
                    if ((uint32_t)c == last_w) sm += (int32_t)((ph >> last_bit) & 1ull) - (int32_t)((mh >> last_bit) & 1ull);
                }
            }
            B += best_hdelta(hpw, hmw);                         // what left the band's last word
            my_cells += nw;
            // row m within k in this column: exact, and a later column wins a tie
            if (nw == W && sm <= k && (uint32_t)sm <= best_d) {
                best_d = (uint32_t)sm;
                best_end = t;
            }
            if (t == n) active = false;                         // through the text
        }
        if ((t & (kBestEvery - 1u)) == 0u) {
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
    if (have) {
        J.d[a] = best_d;
        J.end[a] = best_end;
    }
    const unsigned long long total = best_wave_sum(my_cells);
    if (lane == 0 && total) atomicAdd(J.cells, total);
}

// ---------------------------------------------------------------------------------------------------------------------
// One alignment per wave: lane l holds words l * CW .. l * CW + CW - 1 and is at column t - l at step t.  The band only grows
// (a word that is in stays in).  `on` is how many of the lane's words are in the band; the band is a prefix of the query's
// words, so a lane's own B -- the bottom of its last word that is in -- is the band's B whenever nothing below the lane is in.
// What travels to the next lane each step: the horizontal delta of the lane's last row, the text base, and -- when the lane
// is full and its B <= k -- B + 1, the call to come in.  Lane `row_lane` holds row m (in its word `row_c`) when the wave holds
// the whole query; it alone keeps the running minimum.
// ---------------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(kWave) void bmv_best_wave_kernel(BestJob J) {
    __shared__ uint32_t lut_w[64];
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lut_w);
    const uint32_t lane = threadIdx.x;
    const uint32_t a = J.list[blockIdx.x];                      // (grid = count)
    const uint32_t n = J.text_len[a], m = J.query_len[a];
    const int32_t k = (int32_t)J.bound[a];                      // (the host sends 1 <= m <= 65 536, n >= 1, k <= m)
    const uint32_t W = (m + 63u) >> 6;
    const uint32_t cap = W < 64u * CW ? W : 64u * CW;           // words this wave can hold
    lut_w[lane] = reinterpret_cast<const uint32_t *>(J.lut)[lane];
    __syncthreads();
    const uint32_t nw0 = (uint32_t)k / 64u + 1u < W ? (uint32_t)k / 64u + 1u : W;      // column 0: rows 1 .. k
    // a text too short for the query within k insertions: beyond; a band that does not fit from the start: undecided
    if ((int32_t)m - k > (int32_t)n) {
        if (lane == 0) {
            J.d[a] = kBestBeyond;
            J.end[a] = 0u;
        }
        return;
    }
    if (nw0 > cap) {
        if (lane == 0) {
            J.d[a] = kBestUndecided;
            J.end[a] = 0u;
        }
        return;
    }

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
    const bool whole = cap == W;                                // the wave holds row m
    const uint32_t row_lane = (W - 1u) / CW, row_c = (W - 1u) % CW, row_bit = (m - 1u) & 63u;
    const uint32_t my_row_c = (whole && lane == row_lane) ? row_c : 0xFFFFFFFFu;    // this lane's word with row m, if any
    const uint32_t w_first = lane * CW;
    uint32_t on = nw0 > w_first ? (nw0 - w_first < CW ? nw0 - w_first : CW) : 0u;
    int32_t B = (int32_t)(64u * (w_first + on));
    int32_t sm = (int32_t)m;                                    // row m's computed score; means something while on > my_row_c
    uint32_t best_d = kBestBeyond, best_end = 0u;
    bool below_on = nw0 > w_first + CW;                         // words of the next lanes are in
    uint32_t hp_prev = 0, hm_prev = 0, ch_prev = 0, call_prev = 0;
    uint32_t chunk = 0;                                         // ranks of 64 text columns, column 64 q + lane
    bool rejected = false, leave = false, undecided = false;
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
                    if ((uint32_t)c == my_row_c) sm += (int32_t)((ph >> row_bit) & 1ull) - (int32_t)((mh >> row_bit) & 1ull);
                }
            }
            hp_prev = hpw;
            hm_prev = hmw;
            B += best_hdelta(hpw, hmw);
            my_cells += on;
            // row m within k in this column: exact, and a later column wins a tie
            if (my_row_c < on && sm <= k && (uint32_t)sm <= best_d) {
                best_d = (uint32_t)sm;
                best_end = j;
            }
            const uint32_t in = w_first + on;                   // words of the band down to this lane's last
            if (B <= k) {
                // the next word comes in for column j + 1, from upper bounds below B
                if (in >= cap) {
                    if (cap < W) undecided = true;              // the band outgrows the wave
                } else if (on < CW) {
#pragma unroll
                    for (int c = 1; c < CW; c++) {
                        if ((uint32_t)c == on) {
                            pv[c] = ~0ull;
                            mv[c] = 0;
                        }
                    }
                    if (on == my_row_c) sm = B + (int32_t)row_bit + 1;      // row m comes in: one more per row below B
                    on++;
                    B += 64;
                } else {
                    call_prev = (uint32_t)B + 1u;
                    below_on = true;
                }
            } else if (!(on == CW && below_on)) {
                // this lane's last word is the band's: la <= 64 in - (B - k)
                if ((int32_t)m - ((int32_t)(64u * in) - (B - k)) > (int32_t)n - (int32_t)j) rejected = true;
            }
            if (j == n && !(on == CW && below_on)) leave = true;   // the band's end has passed the text
        } else if (on == 0u && call != 0u) {
            // called in by the lane before, which has just passed the column this lane is at: the first word starts from
            // upper bounds there and runs from the next step on
            on = 1u;
            B = (int32_t)call - 1 + 64;
            if (my_row_c == 0u) sm = (int32_t)call - 1 + (int32_t)row_bit + 1;
        }
        if (__ballot(rejected || leave || undecided) != 0ull) break;
    }
    const bool und = __ballot(undecided) != 0ull;
    const uint32_t rd = (uint32_t)__shfl((int)best_d, (int)(whole ? row_lane : 0u), kWave);
    const uint32_t re = (uint32_t)__shfl((int)best_end, (int)(whole ? row_lane : 0u), kWave);
    if (lane == 0) {
        const bool got = whole && rd != kBestBeyond;
        J.d[a] = und ? kBestUndecided : (got ? rd : kBestBeyond);
        J.end[a] = (!und && got) ? re : 0u;
    }
    const unsigned long long total = best_wave_sum(my_cells);
    if (lane == 0 && total) atomicAdd(J.cells, total);
}

// The pick (defined in bmv_best.hip): a wave per 64 groups.
__global__ void bmv_best_pick_kernel(PickJob P);
// winners still to be aligned in full, in group order: where[g] is the exclusive sum of need
__global__ void bmv_best_compact_kernel(const uint32_t *__restrict__ need, const uint32_t *__restrict__ where,
                                        const uint32_t *__restrict__ winner, uint32_t n_groups, uint32_t *__restrict__ out);

// instantiated in bmv_best.hip
extern template __global__ void bmv_best_lane_kernel<1>(BestJob);
extern template __global__ void bmv_best_lane_kernel<2>(BestJob);
extern template __global__ void bmv_best_lane_kernel<3>(BestJob);
extern template __global__ void bmv_best_lane_kernel<4>(BestJob);
extern template __global__ void bmv_best_lane_kernel<5>(BestJob);
extern template __global__ void bmv_best_lane_kernel<6>(BestJob);
extern template __global__ void bmv_best_lane_kernel<7>(BestJob);
extern template __global__ void bmv_best_lane_kernel<8>(BestJob);
extern template __global__ void bmv_best_wave_kernel<1>(BestJob);
extern template __global__ void bmv_best_wave_kernel<2>(BestJob);
extern template __global__ void bmv_best_wave_kernel<4>(BestJob);

}  // namespace bmv
