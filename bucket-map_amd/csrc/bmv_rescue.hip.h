// bmv_rescue.hip.h -- mate rescue, bmv_rescue (include/bmv.h): a mate without a usable candidate is sought beside a known
// alignment of its partner, the ANCHOR, in the window of the genome where a proper pair would put it.  Three kernels:
//   plan       a thread per job: the view [ws, we) and its strand from the anchor, the fragment range and the contig -- the
//              window definition of bmv.h, here once for the device (host/pair_rescue.h restates it for the host)
//   distance   the exact semi-global distance d of the query against the view and its end column, tie rule (1) of bmv.h
//   finish     a thread per job: d <= k, and bmv_pair's proper(anchor, rescued)
//
// The distance kernel is shaped for this batch: a SHORT query (a mate of 100 - 300 bases, up to 512) against a LONG text
// (about max_frag - min_frag + 2 m + k columns).  Row 0 is free and the placement is unknown, so nothing bounds the distance
// from above and there is no Ukkonen band to keep: a lane holds every word of its query (CW = its word count, 1 .. 8) and runs
// the plain recurrence over every column, fetching the text 64 columns at a time the way bmv_best_lane_kernel does, and
// watches row m for s <= k, a later column winning a tie.
//
// Jobs are few, so a job is cut along the text into `parts` (a power of two, 1 .. 64) that sit in neighbouring lanes of one
// wave.  With n the view's length and b_p = floor(p n / parts), part p starts from a fresh column-0 state at column
// max(0, b_p - m - k), runs to column b_{p+1} and takes into its minimum only end columns in (b_p, b_{p+1}].  Exact: an
// alignment within k edits that ends at column e begins at or after e - m - k, so for e > b_p it lies inside what the part
// walked; the part's value is never below the true one (it sees less text) and is therefore within k exactly when the true
// one is, and then equal to it.  The parts' minima meet across the lane group by shuffles: the smaller distance, then the
// later column.  Results are plain vector stores.
#pragma once

#include "bmv_best.hip.h"

namespace bmv {

constexpr uint32_t kRescueLaneWords = 8;            // queries of up to 64 x this many bases; longer ones: the full aligner

struct RescueJob {
    // the anchors and the range: what plan and finish read
    const uint64_t *anchor_text_start;
    const uint32_t *anchor_text_len;
    const uint8_t *anchor_text_rc;
    const uint32_t *anchor_query_len, *anchor_end;
    const uint64_t *contig_start, *contig_end;
    const uint32_t *max_edits;
    uint32_t n;                     // jobs
    int64_t min_frag, max_frag;
    // the views: plan writes them, distance and finish read them
    const uint8_t *genome;
    const uint8_t *reads;
    const uint8_t *lut;
    uint64_t *text_start;
    uint32_t *text_len;
    uint8_t *text_rc;
    const uint64_t *query_start;
    const uint32_t *query_len;
    // distance: this launch takes the jobs list[0 .. count), parts = 1 << parts_log2 lanes each
    const uint32_t *list;
    uint32_t count, parts_log2;
    uint32_t *d;                    // per job: the distance when it is within k, else kBestBeyond
    uint32_t *end;                  // the exclusive end column (0 unless d is a distance)
    unsigned long long *cells;      // += (64-row word, text column) steps evaluated
    // finish
    uint32_t *out_edits, *out_end;
    uint8_t *out_proper;
};

// L and R of the anchor of job j, bmv_pair's two formulas
__device__ __forceinline__ void rescue_anchor(const RescueJob &J, uint32_t j, int64_t &la, int64_t &ra) {
    const int64_t ts = (int64_t)J.anchor_text_start[j], end = (int64_t)J.anchor_end[j], m = (int64_t)J.anchor_query_len[j];
    if (J.anchor_text_rc[j] != 0) {
        la = ts + (int64_t)J.anchor_text_len[j] - end;
        ra = la + m;
    } else {
        ra = ts + end;
        la = ra - m;
    }
}

__device__ __forceinline__ int64_t rescue_max(int64_t a, int64_t b) { return a > b ? a : b; }
__device__ __forceinline__ int64_t rescue_min(int64_t a, int64_t b) { return a < b ? a : b; }

// ---------------------------------------------------------------------------------------------------------------------
// One part of one job per lane: queries of 1 .. 64 * CW bases (the host lists a job under the CW that is its word count), views
// of any length.  Slot s of the launch is part s % parts of job list[s / parts], so a job's parts are neighbouring lanes.
// ---------------------------------------------------------------------------------------------------------------------
template <int CW>
__global__ __launch_bounds__(kWave) void bmv_rescue_lane_kernel(RescueJob J) {
    __shared__ uint32_t lut_w[64];
    __shared__ uint32_t text_planes[kWave * 4];                 // per lane: the low and the high plane of 64 columns
    const uint8_t *lut = reinterpret_cast<const uint8_t *>(lut_w);
    const uint32_t lane = threadIdx.x, lg = J.parts_log2, parts = 1u << lg;
    const uint64_t slot = (uint64_t)blockIdx.x * kWave + lane;
    const uint32_t p = (uint32_t)slot & (parts - 1u);
    const bool have = (slot >> lg) < (uint64_t)J.count;
    const uint32_t a = J.list[have ? (uint32_t)(slot >> lg) : 0u];
    const uint32_t n = have ? J.text_len[a] : 0u, m = have ? J.query_len[a] : 0u;     // (the host sends 1 <= m <= 64 CW)
    const uint32_t me = have ? J.max_edits[a] : 0u;
    const int32_t k = (int32_t)(me < m ? me : m);
    const uint32_t W = (m + 63u) >> 6;
    const uint32_t last_w = W ? W - 1u : 0u, last_bit = (m - 1u) & 63u;     // where row m lives
    // this part: end columns in (b0, b1], walked from column `from` on
    const uint32_t b0 = (uint32_t)(((uint64_t)p * n) >> lg), b1 = (uint32_t)(((uint64_t)(p + 1u) * n) >> lg);
    const uint32_t warm = m + (uint32_t)k;
    const uint32_t from = b0 > warm ? b0 - warm : 0u;
    const uint32_t skip = b0 - from;                            // local columns that only warm the state up
    bool active = have && W != 0u && b1 > b0;
    const uint32_t len = active ? b1 - from : 0u;
    lut_w[lane] = reinterpret_cast<const uint32_t *>(J.lut)[lane];
    __syncthreads();

    // the query's bit planes (rows past the end: rank 0, as in the aligning kernels)
    uint64_t q0[CW], q1[CW];
#pragma unroll
    for (int c = 0; c < CW; c++) {
        uint64_t p0 = 0, p1 = 0;
        if (active && (uint32_t)c < W) {
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
    const uint64_t t_at = active ? J.text_start[a] : 0u;       // (a lane without work fetches the genome's first byte)
    const uint32_t n_at = active ? n : 0u;
    const uint32_t rc = active ? J.text_rc[a] : 0u;

    uint64_t pv[CW], mv[CW];
#pragma unroll
    for (int c = 0; c < CW; c++) {
        pv[c] = ~0ull;                                          // column `from`: H[i] = i
        mv[c] = 0;
    }
    int32_t sm = (int32_t)m;                                    // row m's score
    uint32_t best_d = kBestBeyond, best_end = 0u;
    uint32_t steps = len;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)steps, o, kWave);
        steps = other > steps ? other : steps;
    }
    unsigned long long my_cells = 0;
    uint64_t tlo = 0, thi = 0;
    for (uint32_t t = 1; t <= steps; t++) {
        const uint32_t x = (t - 1u) & 63u;
        if (x == 0u) {
            // the next 64 columns of every part still running, fetched by the whole wave (one line per part),
            // reverse-complemented if asked; a lane past the view's end reads its last base again
            const uint64_t running = __ballot(active);
            __syncthreads();
            for (uint32_t g0 = 0; g0 < kWave; g0 += 8u) {
                if (((running >> g0) & 0xFFull) == 0ull) continue;
                uint32_t raw[8];
#pragma unroll
                for (uint32_t u = 0; u < 8u; u++) {
                    const uint32_t g = g0 + u;
                    const uint32_t ng = (uint32_t)__builtin_amdgcn_readlane((int)n_at, (int)g);
                    const uint32_t fg = (uint32_t)__builtin_amdgcn_readlane((int)from, (int)g);
                    const uint8_t *src = J.genome + readlane64(t_at, g);
                    const bool rcg = __builtin_amdgcn_readlane((int)rc, (int)g) != 0;
                    const uint32_t last = ng ? ng - 1u : 0u;
                    uint64_t col = (uint64_t)fg + (t - 1u) + lane;  // 0-based in the view as walked, clamped into it
                    col = col < last ? col : last;
                    raw[u] = src[rcg ? last - (uint32_t)col : (uint32_t)col];
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
        if (active) {
            const uint64_t nt0 = not_plane(((tlo >> x) & 1ull) != 0), nt1 = not_plane(((thi >> x) & 1ull) != 0);
            uint32_t hpw = 0, hmw = 0;                          // row 0 is all zeros: free leading text gaps
#pragma unroll
            for (int c = 0; c < CW; c++) {
                if ((uint32_t)c < W) {
                    const uint64_t eq0 = match_rows(q0[c], q1[c], nt0, nt1);
                    uint64_t ph, mh, d0;
                    myers_step_carry(eq0, hpw, hmw, pv[c], mv[c], ph, mh, d0);
                    if ((uint32_t)c == last_w) sm += (int32_t)((ph >> last_bit) & 1ull) - (int32_t)((mh >> last_bit) & 1ull);
                }
            }
            my_cells += W;
            // row m within k at one of this part's own end columns: a later column wins a tie
            if (t > skip && sm <= k && (uint32_t)sm <= best_d) {
                best_d = (uint32_t)sm;
                best_end = from + t;
            }
            if (t == len) active = false;                       // through the part
        }
        if (__ballot(active) == 0ull) break;
    }
    // the parts of a job: the smallest distance, then the latest column
    uint64_t key = ((uint64_t)best_d << 32) | (uint64_t)(~best_end);
    for (uint32_t o = 1; o < parts; o <<= 1) {
        const uint64_t other = shfl64(key, (int)(lane ^ o));
        key = other < key ? other : key;
    }
    if (have && p == 0u) {
        const uint32_t d = (uint32_t)(key >> 32);
        J.d[a] = d;
        J.end[a] = d == kBestBeyond ? 0u : ~(uint32_t)key;
    }
    const unsigned long long total = best_wave_sum(my_cells);
    if (lane == 0 && total) atomicAdd(J.cells, total);
}

// plan and finish (bmv_rescue.hip): a thread per job
__global__ void bmv_rescue_plan_kernel(RescueJob J);
__global__ void bmv_rescue_finish_kernel(RescueJob J);

extern template __global__ void bmv_rescue_lane_kernel<1>(RescueJob);
extern template __global__ void bmv_rescue_lane_kernel<2>(RescueJob);
extern template __global__ void bmv_rescue_lane_kernel<3>(RescueJob);
extern template __global__ void bmv_rescue_lane_kernel<4>(RescueJob);
extern template __global__ void bmv_rescue_lane_kernel<5>(RescueJob);
extern template __global__ void bmv_rescue_lane_kernel<6>(RescueJob);
extern template __global__ void bmv_rescue_lane_kernel<7>(RescueJob);
extern template __global__ void bmv_rescue_lane_kernel<8>(RescueJob);

}  // namespace bmv
