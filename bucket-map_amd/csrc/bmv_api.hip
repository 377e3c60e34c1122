// bmv_api.hip -- C ABI (include/bmv.h) over the alignment-verification kernels in bmv_kernels.hip.h.
// Host side only: validation, choice of the kernel shape for the longest query of the batch, chunking so
// that the traceback bits of one chunk fit the scratch budget, offsets of the packed CIGAR output
// (bm_scan.hip.h's exclusive sum).
// The steps every entry point shares -- checking and uploading a batch's views, a sub-batch through bmv_align_long, the
// band lists of the screen and the distance round, CIGARs to the host, the two passes of annotate and clip -- are the
// helpers in front of `extern "C"`; the kernels a step launches are instantiated in the files their headers name.
#include "../../include/bmv.h"

#include "bm_hip_util.h"
#include "bm_scan.hip.h"
#include "bmv_annotate.hip.h"
#include "bmv_best.hip.h"
#include "bmv_clip.hip.h"
#include "bmv_overlap.hip.h"
#include "bmv_frag.hip.h"
#include "bmv_leftalign.hip.h"
#include "bmv_long.hip.h"
#include "bmv_pair.hip.h"
#include "bmv_realign.hip.h"
#include "bmv_rescue.hip.h"
#include "bmv_screen.hip.h"
#include "bmv_split.hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <type_traits>
#include <vector>

namespace bmv {

// CIGAR entries of one chunk, reversed into reading order at their final offsets.
__global__ void bmv_gather_kernel(const uint32_t *__restrict__ ops_rev, uint32_t ops_stride,
                                  const uint32_t *__restrict__ nops, const uint32_t *__restrict__ offsets,
                                  uint32_t count, uint32_t *__restrict__ out) {
    const uint32_t slot = blockIdx.x * (blockDim.x / 8u) + threadIdx.x / 8u, t = threadIdx.x % 8u;
    if (slot >= count) return;
    const uint32_t c = nops[slot];
    const uint32_t *src = ops_rev + (size_t)slot * ops_stride;
    uint32_t *dst = out + offsets[slot];
    for (uint32_t x = t; x < c; x += 8u) dst[x] = src[c - 1u - x];
}

}  // namespace bmv

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMV_ERR_HIP)

using bmhip::DevBuf;

namespace {

using align_fn = void (*)(bmv::Job);

struct Shape {
    uint32_t group;   // lanes per alignment
    int cw;           // 64-row words per lane
    align_fn fn;
    bool per_lane;    // bmv_align_lane_kernel: one alignment per lane (group 1), its own trace and text layout
};

// A group is as many lanes as the longest query has words, over CW words per lane; the kernel variant fixes CW and how many
// of the group's lanes hold the traceback's 16 pairs of trace words.  CW is chosen by what a wave then spends per
// alignment: the cost of a column step at that CW (the table below: what a step pays once -- the neighbour lane's delta,
// the text base, the loop -- is worth about two words' recurrences), times n + group - 1 steps (the skew), over the
// 64 / group alignments that share them.  A 5-kbp read (79 words) is 4 alignments of 16 lanes x 5 words per wave, not
// one of 40 x 2; a 10-kbp read (157 words) is 2 of 32 x 5, not one of 40 x 4; an 8-kbp read (125 words) 4 of 16 x 8.
constexpr int kMaxCw = 8;
// what one column step of a wave costs at CW words per lane, measured (ns of the whole card per wave and step,
// tools/bench_verify_cw.sh, profiles/r02/verify_shapes.txt; only the ratios matter): about 1.9 + CW words' recurrences --
// what a step pays once (the neighbour lane's delta, the text base, the loop) is worth two words
constexpr double kStepCost[kMaxCw + 1] = {0, 0.206, 0.290, 0.356, 0.440, 0.545, 0.645, 0.700, 0.810};
constexpr uint32_t kStripsBeyond = 64u * kMaxCw;                 // words: longer queries go through in strips

// Queries of up to this many words go one per lane (bmv_align_lane_kernel): 64 alignments share every instruction of a
// column step.  BMV_LANE_MAX=0 switches it off (experiments; tests run both ways).
constexpr uint32_t kLaneWords = 8;
constexpr uint32_t kLaneMaxText = 2048;

Shape pick_shape(uint32_t words, uint32_t max_n) {
    // (64 text windows in LDS, 2 bits a base: 33 KB at 2 048 bases -- longer windows would leave a CU fewer than four waves)
    if (max_n <= kLaneMaxText) {
        static const align_fn per_lane[kLaneWords + 1] = {nullptr,
                                                          bmv::bmv_align_lane_kernel<1>, bmv::bmv_align_lane_kernel<2>,
                                                          bmv::bmv_align_lane_kernel<3>, bmv::bmv_align_lane_kernel<4>,
                                                          bmv::bmv_align_lane_kernel<5>, bmv::bmv_align_lane_kernel<6>,
                                                          bmv::bmv_align_lane_kernel<7>, bmv::bmv_align_lane_kernel<8>};
        const char *env = getenv("BMV_LANE_MAX");
        const uint32_t lane_max = env ? std::min<uint32_t>((uint32_t)atoi(env), kLaneWords) : kLaneWords;
        if (words <= lane_max) return Shape{1u, (int)words, per_lane[words], true};
    }
    // strips of 64 * CW words, one after the other (max_query_len = 65 536 bases: two of them)
    if (words > kStripsBeyond)
        return words <= 2u * 64u * 6u ? Shape{64u, 6, bmv::bmv_align_kernel<4, 6, true>, false} : Shape{64u, 8, bmv::bmv_align_kernel<4, 8, true>, false};
    // A group's lanes share the traceback's trace words, 16 / SLOTS lanes to a (word, block) cell and SLOTS columns each, and
    // a round of the traceback recomputes as many cells as the group has lanes for: groups of 8 lanes and more use the
    // SLOTS = 4 kernels (GROUP / 4 cells), groups of 2..7 lanes the SLOTS = 8 ones (GROUP / 2 cells: 1 kbp as 4 lanes x 4
    // words 12.7 -> 11.8 ms, 600 bases as 2 x 5 instead of 4 x 3 8.6 -> 6.7 ms), a lone lane SLOTS = 16 (CW = 1; only with
    // BMV_LANE_MAX=0 or a text window too long for the lane kernel).
    constexpr uint32_t kEightBelow = 8;
    static const align_fn four_cols[kMaxCw + 1] = {nullptr,
                                                   bmv::bmv_align_kernel<4, 1, false>, bmv::bmv_align_kernel<4, 2, false>,
                                                   bmv::bmv_align_kernel<4, 3, false>, bmv::bmv_align_kernel<4, 4, false>,
                                                   bmv::bmv_align_kernel<4, 5, false>, bmv::bmv_align_kernel<4, 6, false>,
                                                   bmv::bmv_align_kernel<4, 7, false>, bmv::bmv_align_kernel<4, 8, false>};
    static const align_fn eight_cols[kMaxCw + 1] = {nullptr,
                                                    bmv::bmv_align_kernel<8, 1, false>, bmv::bmv_align_kernel<8, 2, false>,
                                                    bmv::bmv_align_kernel<8, 3, false>, bmv::bmv_align_kernel<8, 4, false>,
                                                    bmv::bmv_align_kernel<8, 5, false>, bmv::bmv_align_kernel<8, 6, false>,
                                                    bmv::bmv_align_kernel<8, 7, false>, bmv::bmv_align_kernel<8, 8, false>};
    int cw = 0;
    double best = 0;
    const char *env = getenv("BMV_CW");                          // experiment / test knob: force CW where it is possible
    const int forced = env ? atoi(env) : 0;
    for (int c = 1; c <= kMaxCw; c++) {
        const uint32_t g = (words + (uint32_t)c - 1u) / (uint32_t)c;
        const int max_cw = g >= 2u ? kMaxCw : 1;
        if (g > 64u || c > max_cw) continue;
        if (forced == c) {
            cw = c;
            break;
        }
        const double cost = kStepCost[c] * (double)(max_n + g - 1u) / (double)(64u / g);
        if (cw == 0 || cost < best * 0.98) {
            best = cost;
            cw = c;
        }
    }
    const uint32_t g = std::max(1u, (words + (uint32_t)cw - 1u) / (uint32_t)cw);
    if (g >= kEightBelow) return {g, cw, four_cols[cw], false};
    if (g >= 2) return {g, cw, eight_cols[cw], false};
    return {g, 1, bmv::bmv_align_kernel<16, 1, false>, false};
}

// What the two-pass emit of bmv_annotate and bmv_clip writes on the device ...
struct EmitDev {
    DevBuf<uint32_t> nm, pos, ref_len, n_xcigar, n_ref, xcigar;
    DevBuf<uint64_t> xcigar_offset, ref_offset;
    DevBuf<uint8_t> ref_bases;
};
// ... and what it leaves on the host, with the call's stats
struct EmitHost {
    std::vector<uint32_t> nm, pos, ref_len, xcigar;
    std::vector<uint64_t> xcigar_offset, ref_offset;
    std::vector<uint8_t> ref_bases;
    float ms = 0.f;
    uint64_t n_columns = 0;
};

}  // namespace

constexpr uint32_t kSideStreams = 4;

namespace {
struct PairedPending;       // defined beside bmv_paired_begin
}

// Every device buffer is a DevBuf: `delete` frees them all, bmv_destroy handles only what has an order.
struct bmv_ctx {
    bmv_params p{};
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;   // (ev2: bmv_split times two kernels without a sync between them)
    hipStream_t side[kSideStreams] = {};       // length classes of one batch run side by side on these
    hipEvent_t side_done[kSideStreams] = {};
    bool loaded = false;
    uint64_t n_genome = 0;
    size_t scratch_bytes = 0;
    DevBuf<uint8_t> genome, lut, reads, text_rc, scan_tmp;
    DevBuf<uint64_t> text_start, query_start, trace;
    DevBuf<uint32_t> text_len, query_len, ops_rev, nops, offsets, packed, out_begin, order;
    DevBuf<int32_t> out_score;
    DevBuf<uint8_t> long_slots;                // bmv_align_long: the slots of a piece ...
    DevBuf<uint32_t> long_tiles;               // ... and its tiles, launch by launch
    // results of the last bmv_align, host side
    uint32_t n_last = 0;
    std::vector<int32_t> h_score;
    std::vector<uint32_t> h_begin, h_cigar;
    std::vector<uint64_t> h_offset;
    float ms_kernels = 0.f;
    uint64_t n_cells = 0;
    // bmv_align_bounded: the screen's buffers and what bmv_last_bounded_stats reports
    DevBuf<uint32_t> max_edits, keep, keep_at, survivors, screen_list;
    DevBuf<unsigned long long> screen_count;
    uint32_t n_rejected = 0;
    uint64_t screen_cells = 0;
    float ms_screen = 0.f;
    // bmv_annotate and bmv_clip: the inputs beyond the views, and the emit's outputs -- one set on the device (a call's
    // results are on the host when it returns), one per call on the host (bmv_results / bmv_last_stats keep what the last
    // align left, bmv_annotations what the last bmv_annotate left)
    DevBuf<uint32_t> an_begin, an_cigar;
    DevBuf<uint64_t> an_cigar_offset;
    EmitDev emit;
    EmitHost h_an, h_cl;
    // bmv_clip: what it writes beside the emit's outputs
    DevBuf<int64_t> cl_score;
    DevBuf<uint64_t> cl_l, cl_r;
    DevBuf<uint32_t> cl_pos0, cl_left, cl_right;
    std::vector<int64_t> h_cl_score;
    std::vector<uint32_t> h_cl_left, h_cl_right;
    // bmv_overlap: the pair arrays, what its passes hand to each other (the base range, its ends in the genome, the cut and
    // the roles; the final range goes through bmv_clip's buffers), the host results of bmv_overlapped and what
    // bmv_last_overlap_stats reports
    DevBuf<uint32_t> ov_mate, ov_contig, ov_role, ov_found, ov_cut_q, ov_cut;
    DevBuf<uint64_t> ov_l0, ov_r0, ov_edge;
    DevBuf<int64_t> ov_g0, ov_g1, ov_m;
    DevBuf<uint8_t> ov_was_cut;
    EmitHost h_ov;
    std::vector<int64_t> h_ov_score;
    std::vector<uint32_t> h_ov_left, h_ov_right, h_ov_cut;
    std::vector<uint8_t> h_ov_was_cut;
    uint64_t ov_pairs_cut = 0, ov_bases_cut = 0;
    // bmv_align_best: the distance round's and the pick's buffers (the batch's views go through the aligners' own), the
    // host results of bmv_best and what bmv_last_best_stats reports
    DevBuf<uint32_t> bs_bound, bs_list, bs_d, bs_end, bs_full, bs_group_offset, bs_margin, bs_winner, bs_need, bs_need_at,
        bs_realign, bs_edits, bs_out_end;
    DevBuf<unsigned long long> bs_count;
    uint32_t n_best = 0, n_best_groups = 0;
    std::vector<uint32_t> h_bs_winner, h_bs_edits, h_bs_end;
    uint32_t bs_n_seed = 0, bs_n_distance = 0, bs_n_beyond = 0, bs_n_undecided = 0, bs_n_realigned = 0;
    uint64_t bs_cells = 0;
    float ms_distance = 0.f, ms_pick = 0.f;
    // bmv_pair and bmv_align_paired: the pair kernel's buffers beyond the views and bmv_align_best's (edits, end and the group
    // offsets are that call's), the host results of bmv_pairs and what bmv_last_pair_stats reports
    DevBuf<uint32_t> pr_contig, pr_pick, pr_winner;
    DevBuf<uint8_t> pr_proper;
    DevBuf<uint64_t> pr_s1, pr_s2;
    std::vector<uint32_t> h_pr_pick, h_pr_winner;
    std::vector<uint8_t> h_pr_proper;
    std::vector<uint64_t> h_pr_s1, h_pr_s2;
    float ms_pair = 0.f;
    uint64_t pr_combinations = 0;
    // bmv_frag_spans and bmv_paired_begin with cap > 0: the spans and the bins (the inputs are the pair kernel's), the host
    // results of bmv_frag and what bmv_last_frag_stats reports
    DevBuf<uint32_t> fr_span, fr_hist;
    std::vector<uint32_t> h_fr_span;
    std::vector<uint64_t> h_fr_hist;
    float ms_frag = 0.f;
    uint32_t fr_informative = 0;
    // what a successful bmv_paired_begin leaves for bmv_paired_finish; gone after the finish, and after any other call of the
    // bmv_results row
    std::shared_ptr<PairedPending> pending;
    // bmv_rescue: the jobs' arrays (buffers of its own: the aligners' views are the fallback's), the planned views, the host
    // results of bmv_rescued and what bmv_last_rescue_stats reports
    DevBuf<uint64_t> rs_anchor_start, rs_contig_start, rs_contig_end, rs_query_start, rs_text_start;
    DevBuf<uint32_t> rs_anchor_len, rs_anchor_query_len, rs_anchor_end, rs_query_len, rs_max_edits, rs_text_len, rs_list, rs_d, rs_end,
        rs_out_edits, rs_out_end;
    DevBuf<uint8_t> rs_anchor_rc, rs_text_rc, rs_out_proper;
    DevBuf<unsigned long long> rs_count;
    std::vector<uint64_t> h_rs_text_start;
    std::vector<uint32_t> h_rs_text_len, h_rs_edits, h_rs_end;
    std::vector<uint8_t> h_rs_text_rc, h_rs_proper;
    float ms_rescue = 0.f;
    uint64_t rs_cells = 0;
    uint32_t rs_parts = 1;
    uint32_t resident_lanes = 0;                // what the device keeps in flight at once (bmv_create)
    // bmv_realign: the plan per alignment, the direction codes and reversed entries of a piece, the outputs (the inputs go
    // through bmv_annotate's buffers), the host results of bmv_realigned and what bmv_last_realign_stats reports
    DevBuf<uint8_t> ra_pass, ra_codes;
    DevBuf<uint64_t> ra_row_at, ra_ops_at, ra_offset;
    DevBuf<uint32_t> ra_ops_rev, ra_begin, ra_end_lane, ra_nops, ra_cigar;
    DevBuf<int32_t> ra_score;
    std::vector<int32_t> h_ra_score;
    std::vector<uint32_t> h_ra_begin, h_ra_cigar;
    std::vector<uint8_t> h_ra_realigned;
    std::vector<uint64_t> h_ra_offset;
    float ms_realign = 0.f;
    uint64_t ra_cells = 0;
    uint32_t ra_passed = 0;
    // bmv_leftalign: the stack slots of a piece and every alignment's place in them, the outputs (the inputs go through
    // bmv_annotate's buffers), the host results of bmv_leftaligned and what bmv_last_leftalign_stats reports
    DevBuf<uint64_t> la_slot_at, la_offset, la_compared;
    DevBuf<uint32_t> la_stack, la_begin, la_nops, la_dropped, la_merges, la_cigar;
    DevBuf<uint8_t> la_changed;
    std::vector<uint32_t> h_la_begin, h_la_dropped, h_la_cigar;
    std::vector<uint8_t> h_la_changed;
    std::vector<uint64_t> h_la_offset;
    float ms_leftalign = 0.f;
    uint64_t la_n_compared = 0, la_n_merges = 0, la_n_dropped = 0;
    uint32_t la_n_changed = 0;
    // bmv_split and bmv_split_pick: the range kernel's outputs, which are the pick kernel's inputs (the views, begin and the
    // entries go through bmv_annotate's buffers), the pick's outputs, the host results of bmv_segments and what
    // bmv_last_split_stats reports
    DevBuf<int64_t> sp_score, sp_g_lo, sp_g_hi, sp_s2;
    DevBuf<uint32_t> sp_q_lo, sp_q_hi, sp_contig, sp_group_offset, sp_n_seg, sp_seg;
    std::vector<int64_t> h_sp_score, h_sp_g_lo, h_sp_g_hi, h_sp_s2;
    std::vector<uint32_t> h_sp_q_lo, h_sp_q_hi, h_sp_n_seg, h_sp_seg;
    float ms_sp_range = 0.f, ms_sp_pick = 0.f;
    uint64_t sp_columns = 0, sp_segments = 0;
};

namespace {

// Grow with headroom: the longest read differs a little from call to call, and a reallocation is a free, an
// allocation and a synchronisation of the device each time (the calls themselves are cheap: 0.2-0.5 ms for 45 GiB,
// tools/malloc_probe.py).
size_t with_headroom(size_t need, size_t have) { return need <= have ? have : need + need / 4; }

// experiment / test knob: every query of at least this many bases takes the long path (0: off)
uint32_t long_from() { return getenv("BMV_LONG_FROM") ? (uint32_t)strtoul(getenv("BMV_LONG_FROM"), nullptr, 10) : 0u; }

// an alignment bmv_align does not take: beyond the context's limits, or from BMV_LONG_FROM on
bool goes_long(const bmv_ctx *c, uint32_t m, uint32_t text_len, uint32_t from) {
    return m > c->p.max_query_len || text_len > c->p.max_text_len || (from && m >= from);
}

// every buffer to at least n elements
template <typename... B>
hipError_t need_exact_all(size_t n, B &...buf) {
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? buf.need_exact(n) : e), ...);
    return e;
}

template <typename T, typename V>
void copy_out(T *dst, const V &src) {
    if (dst && !src.empty()) memcpy(dst, src.data(), src.size() * sizeof src[0]);
}

// ---- the host view of a batch: the eight arguments every entry point takes ----
struct Views {
    const uint8_t *reads;
    uint64_t n_read_bytes;
    const uint64_t *text_start;
    const uint32_t *text_len;
    const uint8_t *text_rc;
    const uint64_t *query_start;
    const uint32_t *query_len;
    uint32_t n;
};

// The null and state checks of the call `who`, in the order every entry point makes them.  outputs_ok: the pointers the call
// needs whatever n is; extras_ok: its per-alignment arrays beyond the views.
int check_view_args(const bmv_ctx *c, const char *who, const Views &v, bool outputs_ok, bool extras_ok) {
    if (!c || !outputs_ok) return fail(BMV_ERR_ARG, "%s: null argument", who);
    if (!c->loaded) return fail(BMV_ERR_STATE, "%s before bmv_load_genome", who);
    if (v.n && (!v.text_start || !v.text_len || !v.text_rc || !v.query_start || !v.query_len || !extras_ok || (v.n_read_bytes && !v.reads)))
        return fail(BMV_ERR_ARG, "%s: null argument", who);
    return BMV_OK;
}

// alignment a: its query inside the read buffer, its text inside the genome
int check_view(const bmv_ctx *c, const Views &v, uint32_t a) {
    if (v.query_start[a] > v.n_read_bytes || v.query_len[a] > v.n_read_bytes - v.query_start[a])
        return fail(BMV_ERR_ARG, "alignment %u: query lies outside the read buffer", a);
    if (v.text_start[a] > c->n_genome || v.text_len[a] > c->n_genome - v.text_start[a])
        return fail(BMV_ERR_ARG, "alignment %u: text lies outside the genome", a);
    return BMV_OK;
}

// ... of every alignment, with the batch's cell count; within_limits: the context's limits hold too (bmv_align)
int check_view_ranges(const bmv_ctx *c, const Views &v, bool within_limits, uint64_t *cells) {
    *cells = 0;
    for (uint32_t a = 0; a < v.n; a++) {
        if (within_limits && v.query_len[a] > c->p.max_query_len)
            return fail(BMV_ERR_ARG, "alignment %u: query of %u bases, max_query_len is %u", a, v.query_len[a], c->p.max_query_len);
        if (within_limits && v.text_len[a] > c->p.max_text_len)
            return fail(BMV_ERR_ARG, "alignment %u: text of %u bases, max_text_len is %u", a, v.text_len[a], c->p.max_text_len);
        if (const int rc = check_view(c, v, a)) return rc;
        *cells += (uint64_t)v.query_len[a] * v.text_len[a];
    }
    return BMV_OK;
}

int check_views(const bmv_ctx *c, const char *who, const Views &v, bool outputs_ok, bool extras_ok, bool within_limits, uint64_t *cells) {
    if (const int rc = check_view_args(c, who, v, outputs_ok, extras_ok)) return rc;
    return check_view_ranges(c, v, within_limits, cells);
}

// The checked batch (n > 0) on its way to the device, on the context's stream (the context's device is current).
int upload_views(bmv_ctx *c, const Views &v) {
    const size_t n = v.n;
    HIP_TRY(c->reads.need_exact((size_t)v.n_read_bytes + 64u));   // (slack: an empty query is still fetched from)
    HIP_TRY(need_exact_all(n, c->text_start, c->text_len, c->text_rc, c->query_start, c->query_len));
    if (v.n_read_bytes) HIP_TRY(hipMemcpyAsync(c->reads.p, v.reads, (size_t)v.n_read_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->text_start.p, v.text_start, n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->text_len.p, v.text_len, n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->text_rc.p, v.text_rc, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->query_start.p, v.query_start, n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->query_len.p, v.query_len, n * 4, hipMemcpyHostToDevice, c->stream));
    return BMV_OK;
}

// the uploaded batch as a kernel sees it: the input pointers the job structs share (AnnotateJob reads no lut; LongJob has the
// two lengths in its slots)
template <typename J>
void fill_views(const bmv_ctx *c, J &j) {
    j.genome = c->genome.p;
    j.reads = c->reads.p;
    j.text_start = c->text_start.p;
    j.text_rc = c->text_rc.p;
    j.query_start = c->query_start.p;
    if constexpr (!std::is_same_v<J, bmv::AnnotateJob>) j.lut = c->lut.p;
    if constexpr (!std::is_same_v<J, bmv::LongJob>) {
        j.text_len = c->text_len.p;
        j.query_len = c->query_len.p;
    }
}

// ---- a sub-batch in full ----
// What bmv_align_long left for the alignments `which` of a batch, taken as a batch of their own: slot s is alignment which[s].
struct SubResults {
    std::vector<int32_t> score;
    std::vector<uint32_t> begin, cigar;
    std::vector<uint64_t> offset;          // size() + 1 entries
    float ms = 0.f;
    uint64_t len(size_t s) const { return offset[s + 1] - offset[s]; }
};

// The alignments `which` of v through bmv_align_long -- which is bmv_align itself for everything within the context's
// limits --, exactly what that call does with them on their own; the context's results move to `out`.
int align_sub_batch(bmv_ctx *c, const Views &v, const std::vector<uint32_t> &which, SubResults &out) {
    const size_t ns = which.size();
    std::vector<uint64_t> ts(ns), qs(ns);
    std::vector<uint32_t> tl(ns), ql(ns);
    std::vector<uint8_t> trc(ns);
    for (size_t s = 0; s < ns; s++) {
        const uint32_t a = which[s];
        ts[s] = v.text_start[a];
        tl[s] = v.text_len[a];
        trc[s] = v.text_rc[a];
        qs[s] = v.query_start[a];
        ql[s] = v.query_len[a];
    }
    uint64_t tot = 0;
    if (int rc = bmv_align_long(c, v.reads, v.n_read_bytes, ts.data(), tl.data(), trc.data(), qs.data(), ql.data(), (uint32_t)ns, &tot)) return rc;
    out.score = std::move(c->h_score);
    out.begin = std::move(c->h_begin);
    out.cigar = std::move(c->h_cigar);
    out.offset = std::move(c->h_offset);
    out.ms = c->ms_kernels;
    return BMV_OK;
}

// The results of a call in batch order -> the context, where bmv_results and bmv_last_stats read them: alignment a's CIGAR is
// the len[a] entries of pool from at[a].
void pack_cigars(bmv_ctx *c, uint32_t n, const std::vector<uint32_t> &pool, const std::vector<uint64_t> &at, const std::vector<uint64_t> &len) {
    c->h_offset.assign((size_t)n + 1, 0);
    uint64_t total = 0;
    for (uint32_t a = 0; a < n; a++) {
        c->h_offset[a] = total;
        total += len[a];
    }
    c->h_offset[n] = total;
    c->h_cigar.resize(total);
    for (uint32_t a = 0; a < n; a++) std::copy_n(pool.data() + at[a], len[a], c->h_cigar.data() + c->h_offset[a]);
}

void store_results(bmv_ctx *c, uint32_t n, uint64_t cells, float ms, std::vector<int32_t> &score, std::vector<uint32_t> &begin,
                   const std::vector<uint32_t> &pool, const std::vector<uint64_t> &at, const std::vector<uint64_t> &len, uint64_t *total_cigar) {
    c->pending.reset();         // the row has a new owner: a bmv_paired_begin before it is no longer pending
    c->n_last = n;
    c->n_cells = cells;
    c->ms_kernels = ms;
    c->h_score = std::move(score);
    c->h_begin = std::move(begin);
    pack_cigars(c, n, pool, at, len);
    *total_cigar = c->h_cigar.size();
}

// what full alignments leave, per alignment of a bmv_align_best batch
struct BestFull {
    std::vector<int32_t> score;
    std::vector<uint32_t> begin, r_len, pool;   // r_len: text columns the alignment spans, its M and D lengths
    std::vector<uint64_t> cig_at, cig_len;      // its CIGAR in pool
    float ms = 0.f;
    explicit BestFull(uint32_t n) : score(n, BMV_REJECTED), begin(n, 0), r_len(n, 0), cig_at(n, 0), cig_len(n, 0) {}
    uint32_t edits(uint32_t a) const { return (uint32_t)(-(int64_t)score[a]); }
    uint32_t end(uint32_t a) const { return begin[a] + r_len[a]; }
};

// the alignments `which` in full, into f
int best_sub_batch(bmv_ctx *c, const Views &v, const std::vector<uint32_t> &which, BestFull &f) {
    if (which.empty()) return BMV_OK;
    SubResults sub;
    if (int rc = align_sub_batch(c, v, which, sub)) return rc;
    for (size_t s = 0; s < which.size(); s++) {
        const uint32_t a = which[s];
        f.score[a] = sub.score[s];
        f.begin[a] = sub.begin[s];
        f.cig_at[a] = f.pool.size() + sub.offset[s];
        f.cig_len[a] = sub.len(s);
        uint32_t r = 0;
        for (uint64_t x = sub.offset[s]; x < sub.offset[s + 1]; x++)
            if ((sub.cigar[x] & 15u) != BMV_OP_I) r += sub.cigar[x] >> 4;
        f.r_len[a] = r;
    }
    f.pool.insert(f.pool.end(), sub.cigar.begin(), sub.cigar.end());
    f.ms += sub.ms;
    return BMV_OK;
}

// ---- the bands of the score-only kernels (the screen of bmv_align_bounded, the distance round of bmv_align_best) ----
// Both come as one kernel per lane for queries of up to kLaneWords words and as a wave per alignment in three variants of
// kWaveCw words a lane.  A wrong locus keeps about 2 k rows within a bound of k edits (random bases: D grows by about half
// a row's worth per row): a longer query goes to the smallest variant whose 64 lanes hold that band, or the whole query.
constexpr uint32_t kWaveCw[3] = {1, 2, 4};

// -1: the lane kernel; else the wave kernel's variant
int band_class(uint32_t m, uint32_t k) {
    const uint32_t words = (m + 63u) / 64u;
    if (words <= kLaneWords) return -1;
    const uint64_t band = std::min<uint64_t>(words, ((uint64_t)k * 9u / 4u + 128u) / 64u + 2u);
    int v = 0;
    while (v + 1 < 3 && band > 64u * kWaveCw[v]) v++;
    return v;
}

struct BandLists {
    std::vector<uint32_t> lane, wave[3];
    std::vector<uint32_t> all;              // the lane list, then the wave lists: what the device gets (upload_band_lists)
    uint32_t lane_words = 1;                // the longest query of the lane list
    void add(uint32_t a, uint32_t m, uint32_t k) {
        const int v = band_class(m, k);
        (v < 0 ? lane : wave[v]).push_back(a);
        if (v < 0) lane_words = std::max(lane_words, (m + 63u) / 64u);
    }
    size_t size() const { return lane.size() + wave[0].size() + wave[1].size() + wave[2].size(); }
};

int upload_band_lists(bmv_ctx *c, BandLists &b, uint32_t *d_list) {
    b.all.reserve(b.size());
    b.all.insert(b.all.end(), b.lane.begin(), b.lane.end());
    for (const auto &w : b.wave) b.all.insert(b.all.end(), w.begin(), w.end());
    HIP_TRY(hipMemcpyAsync(d_list, b.all.data(), b.all.size() * 4, hipMemcpyHostToDevice, c->stream));
    return BMV_OK;
}

// One lane kernel and up to three wave kernels over the segments of the uploaded list, between the context's two events.
template <typename J>
int launch_bands(bmv_ctx *c, const BandLists &b, const uint32_t *d_list, void (*const *per_lane)(J), void (*const *per_wave)(J), J j) {
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    size_t at = 0;
    if (!b.lane.empty()) {
        j.list = d_list;
        j.count = (uint32_t)b.lane.size();
        hipLaunchKernelGGL(per_lane[b.lane_words], dim3((j.count + bmv::kWave - 1u) / bmv::kWave), dim3(bmv::kWave), 0, c->stream, j);
        HIP_TRY(hipGetLastError());
        at += b.lane.size();
    }
    for (uint32_t v = 0; v < 3u; v++) {
        if (b.wave[v].empty()) continue;
        j.list = d_list + at;
        j.count = (uint32_t)b.wave[v].size();
        hipLaunchKernelGGL(per_wave[v], dim3(j.count), dim3(bmv::kWave), 0, c->stream, j);
        HIP_TRY(hipGetLastError());
        at += b.wave[v].size();
    }
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    return BMV_OK;
}

// ---- CIGARs to the host ----
// `count` slots from slot0 of nops / offsets, their reversed entries at ops_rev with ops_stride words a slot
struct GatherPiece {
    const uint32_t *ops_rev;
    uint32_t ops_stride, slot0, count;
};

// CIGARs of `slots` slots (launch order, the pieces' back to back) -> the host, through one exclusive sum and one gather per
// piece: h_nops gets their lengths, h_packed their entries in slot order.
int collect_cigars(bmv_ctx *c, const std::vector<GatherPiece> &pieces, uint32_t slots, std::vector<uint32_t> &h_nops, std::vector<uint32_t> &h_packed) {
    HIP_TRY(c->scan_tmp.need_exact(bmscan::tmp_elems(slots) * sizeof(uint32_t)));
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->nops.p, c->offsets.p, slots, reinterpret_cast<uint32_t *>(c->scan_tmp.p), c->stream));
    uint32_t total = 0;                                         // the scan writes slots + 1 values: the last is the total
    HIP_TRY(hipMemcpyAsync(&total, c->offsets.p + slots, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->packed.need_exact(with_headroom(total, c->packed.cap)));
    for (const GatherPiece &pc : pieces) {
        hipLaunchKernelGGL(bmv::bmv_gather_kernel, dim3((pc.count + 31u) / 32u), dim3(256), 0, c->stream, pc.ops_rev, pc.ops_stride,
                           c->nops.p + pc.slot0, c->offsets.p + pc.slot0, pc.count, c->packed.p);
        HIP_TRY(hipGetLastError());
    }
    h_nops.resize(slots);
    h_packed.resize(total);
    HIP_TRY(hipMemcpyAsync(h_nops.data(), c->nops.p, (size_t)slots * 4, hipMemcpyDeviceToHost, c->stream));
    if (total) HIP_TRY(hipMemcpyAsync(h_packed.data(), c->packed.p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMV_OK;
}

// ---- bmv_align: classes, plans, pieces, rounds ----
// Length classes.  The kernel's shape -- lanes per alignment, words per lane -- is fixed per launch by the longest query
// it holds, and a 5-kbp read run in the shape of a 30-kbp one costs six times what it should: the batch is cut into
// classes of similar query length (in 64-row words; everything up to 8 words -- 512 bases, one alignment per lane -- is
// one class, so a short-read batch stays one launch; then up to 16 words), each class is a launch series of its own over an index list, and the
// results find their way back through that list.
constexpr uint32_t kClassUpTo[] = {kLaneWords, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128, 160, 192, 256, 320, 384, 512, 640, 768, 1024};
constexpr uint32_t kClasses = sizeof kClassUpTo / sizeof kClassUpTo[0];

struct ClassOrder {
    uint32_t lo[kClasses + 1] = {0};        // class k is order[lo[k] .. lo[k + 1])
    uint32_t n_classes = 0;                 // of them, not empty
    std::vector<uint32_t> order;            // the batch by class, file order within a class
};

ClassOrder partition_classes(const uint32_t *query_len, uint32_t n) {
    const bool classes_off = getenv("BMV_ONE_CLASS") != nullptr;    // experiment knob: the whole batch in the longest query's shape
    auto class_of = [&](uint32_t m) {
        const uint32_t words = classes_off ? 0u : (m + 63u) / 64u;
        uint32_t k = 0;
        while (k + 1u < kClasses && words > kClassUpTo[k]) k++;
        return k;
    };
    ClassOrder co;
    for (uint32_t a = 0; a < n; a++) co.lo[class_of(query_len[a]) + 1u]++;
    for (uint32_t k = 0; k < kClasses; k++) {
        co.n_classes += co.lo[k + 1] ? 1u : 0u;
        co.lo[k + 1] += co.lo[k];
    }
    co.order.resize(n);
    uint32_t at[kClasses];
    for (uint32_t k = 0; k < kClasses; k++) at[k] = co.lo[k];
    for (uint32_t a = 0; a < n; a++) co.order[at[class_of(query_len[a])]++] = a;      // stable: file order within a class
    return co;
}

// A batch of one length class (or of a few neighbouring ones: 10-kbp reads with indels straddle a class boundary) gains
// nothing from more alignments in flight than fill the card, and fresh device memory is not free (the first call that
// grew the scratch to 90 GB spent 2 s in hipMalloc): only a batch that really mixes lengths -- three classes or more,
// the longest query at least twice the shortest class's -- may use more than 48 GiB.
size_t scratch_budget(const bmv_ctx *c, const uint32_t *query_len, uint32_t n, uint32_t n_classes) {
    uint32_t lo_m = 0xFFFFFFFFu, hi_m = 0;
    for (uint32_t a = 0; a < n; a++) {
        lo_m = std::min(lo_m, std::max(query_len[a], 1024u));
        hi_m = std::max(hi_m, query_len[a]);
    }
    if (n_classes >= 3 && hi_m >= 2u * lo_m) return c->scratch_bytes;
    return std::min<size_t>(c->scratch_bytes, (size_t)48 << 30);
}

// what a class needs: its kernel, the scratch of one alignment slot, how many slots a launch may hold
struct Plan {
    uint32_t lo, members, max_m, trace_words, gpw, n_blocks, ops_stride, lds_stride;
    Shape sh;
    uint64_t trace_stride, chunk;
    size_t lds;
    uint64_t per_slot() const { return trace_stride / gpw * 8u + (uint64_t)ops_stride * 4u; }   // bytes of scratch
};

// the plan of the class order[lo .. lo + members)
int plan_class(const Views &v, const std::vector<uint32_t> &order, uint32_t lo, uint32_t members, size_t budget, Plan &pl) {
    pl = Plan{};
    pl.lo = lo;
    pl.members = members;
    uint32_t max_m = 0, max_n = 0;
    for (uint32_t s0 = pl.lo; s0 < pl.lo + pl.members; s0++) {
        max_m = std::max(max_m, v.query_len[order[s0]]);
        max_n = std::max(max_n, v.text_len[order[s0]]);
    }
    pl.max_m = max_m;
    // kernel shape for the longest query of the class; scratch per alignment slot
    const uint32_t words = (max_m + 63u) / 64u;
    pl.sh = pick_shape(words ? words : 1u, max_n);
    pl.trace_words = std::max(std::max(words, 1u), pl.sh.group * (uint32_t)pl.sh.cw);   // (more than the words only for strips)
    pl.gpw = 64u / pl.sh.group;
    // checkpoints every 16 columns: (Pv, Mv) per word, plus one 32-bit word of horizontal deltas per word and block
    pl.n_blocks = (max_n + pl.sh.group + 15u) / 16u + 1u;     // blocks of 16 STEPS: the group's last lane is group - 1 steps behind
    const uint64_t n_entries = (uint64_t)pl.n_blocks * pl.gpw * pl.trace_words;
    pl.trace_stride = n_entries * 2u + (n_entries + 1u) / 2u;               // 64-bit words per wave
    pl.trace_stride += 2u * pl.trace_words * pl.gpw;                        // ... and the query's bit planes, for the traceback
    pl.ops_stride = max_m + max_n + 1u;
    pl.lds_stride = (max_n + 15u) / 16u * 4u + 4u;                          // the text as a 2-bit stream
    if (pl.sh.per_lane) pl.lds_stride = (max_n + 63u) / 64u * 16u + 8u;     // ... as two bit planes, 64 columns at a time
    pl.lds = 256 + (size_t)pl.gpw * pl.lds_stride;
    if (pl.lds > 160 * 1024) return fail(BMV_ERR_UNSUPPORTED, "text windows of %u bases need %zu B of LDS", max_n, pl.lds);
    if (pl.lds > 48 * 1024) HIP_TRY(bmhip::raise_dynamic_lds(reinterpret_cast<const void *>(pl.sh.fn), pl.lds));
    uint64_t chunk = std::max<uint64_t>(pl.gpw, budget / pl.per_slot());
    chunk = std::min<uint64_t>(chunk, (uint64_t)pl.gpw << 25);   // one wave per gpw alignments: waves * 64 threads < 2^32
    chunk = std::min<uint64_t>(chunk / pl.gpw * pl.gpw, (uint64_t)pl.members);
    if (chunk == 0) chunk = pl.members;
    // pieces of equal size: 40 000 alignments under a limit of 31 000 are 2 x 20 000, not 31 000 + 9 000 (a piece's
    // last waves run on a card that is emptying, whatever its size)
    const uint64_t n_pieces = (pl.members + chunk - 1u) / chunk;
    const uint64_t even = ((pl.members + n_pieces - 1u) / n_pieces + pl.gpw - 1u) / pl.gpw * pl.gpw;
    pl.chunk = std::min(chunk, even);
    return BMV_OK;
}

// a launch: `count` members of a class from `first`, and the scratch they take
struct Todo {
    const Plan *pl;
    uint64_t first;         // within the class
    uint32_t count;
    size_t trace_words, ops_words;
};

// Rounds.  A launch's scratch (checkpoints + reversed CIGAR entries) is what bounds how many alignments are in flight:
// 19 MB per 30-kbp alignment.  A class of long reads is few waves that each run for tens of milliseconds, so one class
// at a time leaves most of the card idle (measured on 40 000 alignments of 1 .. 30 kbp: 19.8 T cell updates/s against
// 37-41 T for uniform batches).  Every class is therefore cut into pieces of at most a THIRD of the scratch budget (when
// there is more than one class), the pieces -- longest reads first -- are packed into rounds that fit the budget
// together, and the pieces of a round run side by side on a few streams; their CIGARs are collected once per round.
// BMV_SERIAL_CLASSES=1: one piece per round (the old behaviour), for comparison.
std::vector<Todo> cut_pieces(const std::vector<Plan> &plans, size_t budget, bool serial) {
    std::vector<Todo> todo;
    for (size_t i = plans.size(); i-- > 0;) {                   // the longest first: they take the longest
        const Plan &pl = plans[i];
        uint64_t chunk = pl.chunk;
        if (plans.size() > 1 && !serial) {
            const uint64_t third = std::max<uint64_t>(pl.gpw, budget / 3u / pl.per_slot()) / pl.gpw * pl.gpw;
            chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(third, pl.gpw));
            const uint64_t n_pieces = (pl.members + chunk - 1u) / chunk;
            chunk = std::min<uint64_t>(chunk, ((pl.members + n_pieces - 1u) / n_pieces + pl.gpw - 1u) / pl.gpw * pl.gpw);
        }
        for (uint64_t first = 0; first < pl.members; first += chunk) {
            const uint32_t count = (uint32_t)std::min<uint64_t>(chunk, pl.members - first);
            todo.push_back({&pl, first, count, (size_t)((count + pl.gpw - 1u) / pl.gpw * pl.trace_stride), (size_t)count * pl.ops_stride});
        }
    }
    return todo;
}

// the pieces of the round that begins at todo[at]: as many as fit the budget (at least one); returns where it ends
size_t round_end(const std::vector<Todo> &todo, size_t at, size_t budget, bool serial) {
    size_t end = at, sum_trace = 0, sum_ops = 0;
    while (end < todo.size() &&
           (end == at || (!serial && (sum_trace + todo[end].trace_words) * 8u + (sum_ops + todo[end].ops_words) * 4u <= budget))) {
        sum_trace += todo[end].trace_words;
        sum_ops += todo[end].ops_words;
        end++;
    }
    return end;
}

int launch_piece(bmv_ctx *c, const Todo &t, hipStream_t stream, uint64_t *trace, uint32_t *ops_rev, uint32_t *nops, uint32_t stop_after) {
    const Plan &pl = *t.pl;
    bmv::Job j{};
    fill_views(c, j);
    j.order = c->order.p + pl.lo + t.first;
    j.count = t.count;
    j.trace = trace;
    j.trace_stride = pl.trace_stride;
    j.trace_words = pl.trace_words;
    j.trace_blocks = pl.n_blocks;
    j.group = pl.sh.group;
    j.ops_rev = ops_rev;
    j.ops_stride = pl.ops_stride;
    j.text_lds_stride = pl.lds_stride;
    j.out_score = c->out_score.p;
    j.out_begin = c->out_begin.p;
    j.out_nops = nops;
    j.stop_after = stop_after;
    hipLaunchKernelGGL(pl.sh.fn, dim3((t.count + pl.gpw - 1u) / pl.gpw), dim3(bmv::kWave), pl.lds, stream, j);
    HIP_TRY(hipGetLastError());
    return BMV_OK;
}

// Where the CIGARs of the rounds go.  One class: order is the identity and they arrive in place, in c->h_cigar with their
// offsets in c->h_offset.  Else they are kept aside in launch order until every length is known (pack_cigars).
struct CigarStash {
    bool in_place;
    std::vector<uint32_t> pool;
    std::vector<uint64_t> at, len;          // per alignment of the batch
    std::vector<uint32_t> h_nops, h_packed; // a round's, as collect_cigars leaves them
};

// The round todo[at .. end): the pieces launched side by side (alone: on the context's stream), their CIGARs collected into
// `stash`, the round's time added to c->ms_kernels.
int run_round(bmv_ctx *c, const std::vector<Todo> &todo, size_t at, size_t end, const std::vector<uint32_t> &order, uint32_t stop_after,
              CigarStash &stash) {
    size_t sum_trace = 0, sum_ops = 0, slots = 0;
    for (size_t i = at; i < end; i++) {
        sum_trace += todo[i].trace_words;
        sum_ops += todo[i].ops_words;
        slots += todo[i].count;
    }
    HIP_TRY(c->trace.need_exact(with_headroom(sum_trace, c->trace.cap)));
    HIP_TRY(c->ops_rev.need_exact(with_headroom(sum_ops, c->ops_rev.cap)));
    HIP_TRY(c->nops.need_exact(with_headroom(slots, c->nops.cap)));
    HIP_TRY(c->offsets.need_exact(with_headroom(slots + 1, c->offsets.cap)));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));             // the uploads above / the round before
    std::vector<GatherPiece> pieces;
    size_t trace_at = 0, ops_at = 0;
    uint32_t slot_at = 0;
    const bool alone = end - at == 1;
    for (size_t i = at; i < end; i++) {
        const Todo &t = todo[i];
        hipStream_t st = alone ? c->stream : c->side[(i - at) % kSideStreams];
        if (!alone) HIP_TRY(hipStreamWaitEvent(st, c->ev0, 0));
        if (int rc = launch_piece(c, t, st, c->trace.p + trace_at, c->ops_rev.p + ops_at, c->nops.p + slot_at, stop_after)) return rc;
        pieces.push_back({c->ops_rev.p + ops_at, t.pl->ops_stride, slot_at, t.count});
        trace_at += t.trace_words;
        ops_at += t.ops_words;
        slot_at += t.count;
    }
    if (!alone)
        for (uint32_t k = 0; k < kSideStreams; k++) {       // the main stream goes on when all of them are done
            HIP_TRY(hipEventRecord(c->side_done[k], c->side[k]));
            HIP_TRY(hipStreamWaitEvent(c->stream, c->side_done[k], 0));
        }
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    if (int rc = collect_cigars(c, pieces, slot_at, stash.h_nops, stash.h_packed)) return rc;
    std::vector<uint32_t> &dst = stash.in_place ? c->h_cigar : stash.pool;
    uint64_t cig_at = dst.size();
    for (size_t i = at; i < end; i++) {                         // in slot order, and the slots are theirs back to back
        const Todo &t = todo[i];
        for (uint32_t s0 = 0; s0 < t.count; s0++) {
            const uint32_t len = stash.h_nops[pieces[i - at].slot0 + s0];
            if (stash.in_place) {
                c->h_offset[t.first + s0] = cig_at;
            } else {
                const uint32_t a = order[t.pl->lo + t.first + s0];
                stash.len[a] = len;
                stash.at[a] = cig_at;
            }
            cig_at += len;
        }
    }
    dst.insert(dst.end(), stash.h_packed.begin(), stash.h_packed.end());
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->ms_kernels += ms;
    if (getenv("BMV_LOG_CLASSES")) {
        fprintf(stderr, "[bmv] round of %zu piece(s), %.2f ms:", end - at, ms);
        for (size_t i = at; i < end; i++)
            fprintf(stderr, " [up to %u bases: %u of %u alignments, %u lanes x %d words]", todo[i].pl->max_m, todo[i].count,
                    todo[i].pl->members, todo[i].pl->sh.group, todo[i].pl->sh.cw);
        fprintf(stderr, "\n");
    }
    return BMV_OK;
}

// ---- bmv_annotate and bmv_clip ----
// The annotation pass (include/bmv.h, bmv_annotate.hip.h) and the clipping pass (bmv_clip.hip.h) take the same batch.
// Everything a kernel relies on is checked here first -- the views, the CIGAR alphabet, that every CIGAR consumes exactly
// its query and stays inside its window -- so that the kernels index without bounds checks.  `who`: the call, for the message.
int check_annotate_batch(bmv_ctx *c, const char *who, const Views &v, const uint32_t *begin, const uint64_t *cigar_offset,
                         const uint32_t *cigar, uint64_t *out_columns) {
    uint64_t columns = 0;
    for (uint32_t a = 0; a < v.n; a++) {
        if (const int rc = check_view(c, v, a)) return rc;
        if (cigar_offset[a + 1] < cigar_offset[a] || cigar_offset[a + 1] - cigar_offset[a] > 0xFFFFFFFFull - v.query_len[a])
            return fail(BMV_ERR_ARG, "alignment %u: CIGAR offsets %llu .. %llu", a, (unsigned long long)cigar_offset[a],
                        (unsigned long long)cigar_offset[a + 1]);
        if (cigar_offset[a + 1] > cigar_offset[a] && !cigar) return fail(BMV_ERR_ARG, "%s: null argument", who);
        if (cigar_offset[a + 1] == cigar_offset[a]) continue;   // an empty CIGAR: zeros and no entries, whatever the views hold
        uint64_t in_query = 0, in_text = 0, cols = 0;
        uint32_t before = 0xFFFFFFFFu;
        for (uint64_t x = cigar_offset[a]; x < cigar_offset[a + 1]; x++) {
            const uint32_t op = cigar[x] & 15u, len = cigar[x] >> 4;
            const unsigned long long k = (unsigned long long)(x - cigar_offset[a]);
            if (op > BMV_OP_D) return fail(BMV_ERR_ARG, "alignment %u: CIGAR entry %llu has op code %u (M, I and D are taken)", a, k, op);
            if (len == 0) return fail(BMV_ERR_ARG, "alignment %u: CIGAR entry %llu has length 0", a, k);
            if (op == before) return fail(BMV_ERR_ARG, "alignment %u: CIGAR entries %llu and %llu share an op", a, k - 1u, k);
            before = op;
            if (op != BMV_OP_D) in_query += len;
            if (op != BMV_OP_I) in_text += len;
            cols += len;
        }
        if (in_query != v.query_len[a])
            return fail(BMV_ERR_ARG, "alignment %u: the CIGAR consumes %llu query bases, the query has %u", a,
                        (unsigned long long)in_query, v.query_len[a]);
        if ((uint64_t)begin[a] + in_text > v.text_len[a])
            return fail(BMV_ERR_ARG, "alignment %u: begin %u + %llu reference bases run past the window of %u", a, begin[a],
                        (unsigned long long)in_text, v.text_len[a]);
        columns += cols;
    }
    *out_columns = columns;
    return BMV_OK;
}

// The checked batch (n > 0) on its way to the device, on the context's stream; j receives the input pointers.  `rebased` is
// the caller's: the copy out of it may still be under way on return.
int upload_annotate_batch(bmv_ctx *c, const Views &v, const uint32_t *begin, const uint64_t *cigar_offset, const uint32_t *cigar,
                          std::vector<uint64_t> &rebased, bmv::AnnotateJob &j) {
    const size_t n = v.n;
    const uint64_t cig0 = cigar_offset[0], n_cigar = cigar_offset[n] - cig0;
    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(c->an_begin.need_exact(n));
    HIP_TRY(c->an_cigar_offset.need_exact(n + 1u));
    HIP_TRY(c->an_cigar.need((size_t)n_cigar));
    HIP_TRY(c->scan_tmp.need_exact(bmscan::tmp_elems(n) * sizeof(uint64_t)));
    if (const int rc = upload_views(c, v)) return rc;
    HIP_TRY(hipMemcpyAsync(c->an_begin.p, begin, n * 4, hipMemcpyHostToDevice, c->stream));
    rebased.assign(cigar_offset, cigar_offset + n + 1u);                            // the device holds cigar[cig0 ..) only
    for (uint64_t &o : rebased) o -= cig0;
    HIP_TRY(hipMemcpyAsync(c->an_cigar_offset.p, rebased.data(), (n + 1u) * 8, hipMemcpyHostToDevice, c->stream));
    if (n_cigar) HIP_TRY(hipMemcpyAsync(c->an_cigar.p, cigar + cig0, (size_t)n_cigar * 4, hipMemcpyHostToDevice, c->stream));
    fill_views(c, j);
    j.begin = c->an_begin.p;
    j.cigar_offset = c->an_cigar_offset.p;
    j.cigar = c->an_cigar.p;
    j.count = v.n;
    return BMV_OK;
}

// what a call of either leaves before anything runs: n alignments of zeros and no entries
void reset_emit(EmitHost &h, uint32_t n, uint64_t columns) {
    h.nm.assign(n, 0);
    h.pos.assign(n, 0);
    h.ref_len.assign(n, 0);
    h.xcigar_offset.assign((size_t)n + 1, 0);
    h.ref_offset.assign((size_t)n + 1, 0);
    h.xcigar.clear();
    h.ref_bases.clear();
    h.ms = 0.f;
    h.n_columns = columns;
}

// The two passes over an uploaded batch (j's inputs are filled): count pass -> two 64-bit exclusive sums -> the offsets to the
// host -> the outputs sized -> write pass -> download into h.  `count` and `write` launch the caller's kernels on the
// context's stream once j's outputs of that pass are set; `more` queues the caller's own downloads in front of the common
// ones.  who / passes: for the log line.
template <typename Count, typename Write, typename More>
int two_pass_emit(bmv_ctx *c, const char *who, const char *passes, bmv::AnnotateJob &j, EmitHost &h, Count count, Write write, More more,
                  uint64_t *total_xcigar, uint64_t *total_ref_bases) {
    const size_t n = j.count;
    EmitDev &d = c->emit;
    HIP_TRY(need_exact_all(n, d.nm, d.pos, d.ref_len, d.n_xcigar, d.n_ref));
    HIP_TRY(need_exact_all(n + 1u, d.xcigar_offset, d.ref_offset));
    j.nm = d.nm.p;
    j.pos = d.pos.p;
    j.ref_len = d.ref_len.p;
    j.n_xcigar = d.n_xcigar.p;
    j.n_ref = d.n_ref.p;
    uint64_t *scan_tmp = reinterpret_cast<uint64_t *>(c->scan_tmp.p);
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    HIP_TRY(count());
    HIP_TRY(bmscan::exclusive_sum<uint64_t>(d.n_xcigar.p, d.xcigar_offset.p, n, scan_tmp, c->stream));
    HIP_TRY(bmscan::exclusive_sum<uint64_t>(d.n_ref.p, d.ref_offset.p, n, scan_tmp, c->stream));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(h.xcigar_offset.data(), d.xcigar_offset.p, (n + 1u) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h.ref_offset.data(), d.ref_offset.p, (n + 1u) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms_count = 0.f, ms_write = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_count, c->ev0, c->ev1));
    const uint64_t n_x = h.xcigar_offset[n], n_r = h.ref_offset[n];
    HIP_TRY(d.xcigar.need_exact(with_headroom((size_t)n_x, d.xcigar.cap)));
    HIP_TRY(d.ref_bases.need_exact(with_headroom((size_t)n_r, d.ref_bases.cap)));
    j.xcigar_offset = d.xcigar_offset.p;
    j.ref_offset = d.ref_offset.p;
    j.xcigar = d.xcigar.p;
    j.ref_bases = d.ref_bases.p;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    HIP_TRY(write());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    h.xcigar.resize((size_t)n_x);
    h.ref_bases.resize((size_t)n_r);
    HIP_TRY(more());
    HIP_TRY(hipMemcpyAsync(h.nm.data(), d.nm.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h.pos.data(), d.pos.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h.ref_len.data(), d.ref_len.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_x) HIP_TRY(hipMemcpyAsync(h.xcigar.data(), d.xcigar.p, (size_t)n_x * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_r) HIP_TRY(hipMemcpyAsync(h.ref_bases.data(), d.ref_bases.p, (size_t)n_r, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&ms_write, c->ev0, c->ev1));
    h.ms = ms_count + ms_write;
    if (getenv("BMV_LOG_CLASSES"))
        fprintf(stderr, "[bmv] %s: %zu alignments, %s and scans %.3f ms, write pass %.3f ms\n", who, n, passes, ms_count, ms_write);
    *total_xcigar = n_x;
    *total_ref_bases = n_r;
    return BMV_OK;
}

// what bmv_annotations and bmv_clipped share
void copy_emit(const EmitHost &h, uint32_t *out_nm, uint32_t *out_pos, uint32_t *out_ref_len, uint64_t *out_xcigar_offset,
               uint32_t *out_xcigar, uint64_t *out_ref_offset, uint8_t *out_ref_bases) {
    copy_out(out_nm, h.nm);
    copy_out(out_pos, h.pos);
    copy_out(out_ref_len, h.ref_len);
    copy_out(out_xcigar_offset, h.xcigar_offset);
    copy_out(out_xcigar, h.xcigar);
    copy_out(out_ref_offset, h.ref_offset);
    copy_out(out_ref_bases, h.ref_bases);
}

// bmv_load_genome(_records) after their argument checks: the genome is the n_records records back to back (n_bases in all)
int load_genome(bmv_ctx *c, const uint8_t *const *rec, const uint64_t *rec_len, uint32_t n_records, uint64_t n_bases) {
    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(c->genome.need_exact((size_t)n_bases + 64u));       // (slack: an empty text window at the very end is still fetched from)
    HIP_TRY(bmhip::upload_pageable_records(c->genome.p, rec, rec_len, n_records));
    c->n_genome = n_bases;
    c->loaded = true;
    return BMV_OK;
}

// ---- bmv_align_best and bmv_align_paired ----
// group_offset as both take it, and the hints
int check_groups(const char *who, const uint32_t *group_offset, uint32_t n_groups, uint32_t n, const uint32_t *hint) {
    if (group_offset[0] != 0u) return fail(BMV_ERR_ARG, "%s: group_offset[0] is %u, not 0", who, group_offset[0]);
    for (uint32_t g = 0; g < n_groups; g++) {
        if (group_offset[g + 1] < group_offset[g] || group_offset[g + 1] > n)
            return fail(BMV_ERR_ARG, "group %u: group_offset runs from %u to %u (not monotone, or beyond the %u alignments)", g,
                        group_offset[g], group_offset[g + 1], n);
        const uint32_t size = group_offset[g + 1] - group_offset[g];
        if (hint && size && hint[g] >= size) return fail(BMV_ERR_ARG, "group %u: hint %u, the group has %u alignments", g, hint[g], size);
    }
    if (group_offset[n_groups] != n)
        return fail(BMV_ERR_ARG, "group %u: group_offset ends at %u, the batch has %u alignments", n_groups ? n_groups - 1u : 0u,
                    group_offset[n_groups], n);
    return BMV_OK;
}

// what the first three rounds leave on the host
struct BestRounds {
    BestFull f;
    std::vector<uint32_t> full;                 // per alignment: != 0 when f holds its full alignment
    std::vector<uint32_t> d, end;               // per alignment: the distance round's (d, end), exact for every d that matters
    std::vector<uint32_t> winner, edits, out_end, realign;      // the pick's outputs; realign: the winners without a full alignment
    bool on_device = false;                     // bs_edits / bs_out_end / bs_group_offset hold edits / out_end / the offsets
    BestRounds(uint32_t n, uint32_t n_groups)
        : f(n), full(n, 0u), d(n, bmv::kBestUndecided), end(n, 0u), winner(n_groups, bmv::kBestBeyond), edits(n, bmv::kBestBeyond),
          out_end(n, 0u) {}
};

void leave_pending(bmv_ctx *c);         // (beside bmv_paired_begin)

// The rounds bmv_align_best and bmv_align_paired share, on a checked batch: the seeds -- one alignment per group, the hinted
// one -- in full by bmv_align_long; every other alignment through the distance kernels under k = seed's edits + margin, and
// what they leave undecided in full as well; the pick on the device, which restricts (d, end) to d <= best + margin.
int best_rounds(bmv_ctx *c, const char *who, const Views &v, const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin,
                const uint32_t *hint, BestRounds &r) {
    const uint32_t n = v.n;
    const uint32_t *text_len = v.text_len, *query_len = v.query_len;
    const uint32_t from = long_from();
    BestFull &f = r.f;
    std::vector<uint32_t> &full = r.full, &h_d = r.d, &h_end = r.end, &h_winner = r.winner, &h_edits = r.edits, &h_out_end = r.out_end;
    leave_pending(c);           // (a call that fails before its first full alignment has not dropped the pending begin yet)
    c->bs_n_seed = c->bs_n_distance = c->bs_n_beyond = c->bs_n_undecided = c->bs_n_realigned = 0;
    c->bs_cells = 0;
    c->ms_distance = c->ms_pick = 0.f;

    // 1. the seeds
    std::vector<uint32_t> seeds, seed_of(n_groups, bmv::kBestBeyond);
    for (uint32_t g = 0; g < n_groups; g++) {
        if (group_offset[g + 1] == group_offset[g]) continue;
        seed_of[g] = group_offset[g] + (hint ? hint[g] : 0u);
        seeds.push_back(seed_of[g]);
    }
    if (int rc = best_sub_batch(c, v, seeds, f)) return rc;
    for (uint32_t a : seeds) full[a] = 1u;
    c->bs_n_seed = (uint32_t)seeds.size();

    for (uint32_t a : seeds) {
        h_d[a] = f.edits(a);
        h_end[a] = f.end(a);
    }
    if (seeds.size() == n) {
        // every group is its seed alone: nothing to decide
        for (uint32_t g = 0; g < n_groups; g++) h_winner[g] = seed_of[g];
        h_edits = h_d;
        h_out_end = h_end;
        return BMV_OK;
    }
    // 2. the distance round: everything but the seeds, under k = min(seed's edits + margin, query length)
    std::vector<uint32_t> bound(n, 0u), undecided;
    BandLists listed;
    for (uint32_t g = 0; g < n_groups; g++) {
        for (uint32_t a = group_offset[g]; a < group_offset[g + 1]; a++) {
            if (a == seed_of[g]) continue;
            const uint32_t m = query_len[a];
            const uint32_t k = (uint32_t)std::min<uint64_t>((uint64_t)h_d[seed_of[g]] + margin[g], m);
            bound[a] = k;
            if (goes_long(c, m, text_len[a], from) || m == 0u || text_len[a] == 0u)   // (an empty side: the aligner's own conventions)
                undecided.push_back(a);
            else
                listed.add(a, m, k);
        }
    }
    const size_t n_listed = listed.size();
    c->bs_n_distance = (uint32_t)n_listed;
    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(need_exact_all(n, c->bs_d, c->bs_end));
    if (n_listed) {
        HIP_TRY(c->bs_bound.need_exact(n));
        HIP_TRY(c->bs_list.need_exact(n_listed));
        HIP_TRY(c->bs_count.need_exact(1));
        if (const int rc = upload_views(c, v)) return rc;
        HIP_TRY(hipMemcpyAsync(c->bs_bound.p, bound.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        if (const int rc = upload_band_lists(c, listed, c->bs_list.p)) return rc;
        HIP_TRY(hipMemcpyAsync(c->bs_d.p, h_d.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->bs_end.p, h_end.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(c->bs_count.p, 0, sizeof(unsigned long long), c->stream));
        bmv::BestJob j{};
        fill_views(c, j);
        j.bound = c->bs_bound.p;
        j.d = c->bs_d.p;
        j.end = c->bs_end.p;
        j.cells = c->bs_count.p;
        using best_fn = void (*)(bmv::BestJob);
        static const best_fn per_lane[kLaneWords + 1] = {nullptr,
                                                         bmv::bmv_best_lane_kernel<1>, bmv::bmv_best_lane_kernel<2>,
                                                         bmv::bmv_best_lane_kernel<3>, bmv::bmv_best_lane_kernel<4>,
                                                         bmv::bmv_best_lane_kernel<5>, bmv::bmv_best_lane_kernel<6>,
                                                         bmv::bmv_best_lane_kernel<7>, bmv::bmv_best_lane_kernel<8>};
        static const best_fn per_wave[3] = {bmv::bmv_best_wave_kernel<1>, bmv::bmv_best_wave_kernel<2>, bmv::bmv_best_wave_kernel<4>};
        if (const int rc = launch_bands(c, listed, c->bs_list.p, per_lane, per_wave, j)) return rc;
        unsigned long long steps = 0;
        HIP_TRY(hipMemcpyAsync(h_d.data(), c->bs_d.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h_end.data(), c->bs_end.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&steps, c->bs_count.p, sizeof steps, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipEventElapsedTime(&c->ms_distance, c->ev0, c->ev1));
        c->bs_cells = 64u * (uint64_t)steps;
        for (uint32_t a : listed.all) {
            if (h_d[a] == bmv::kBestUndecided) {
                undecided.push_back(a);
                c->bs_n_undecided++;
            } else if (h_d[a] == bmv::kBestBeyond) {
                c->bs_n_beyond++;
            }
        }
        f.ms += c->ms_distance;
        if (getenv("BMV_LOG_CLASSES"))
            fprintf(stderr, "[bmv] best: %zu seeds; distance round %zu per lane, %zu / %zu / %zu per wave at 1 / 2 / 4 words a lane; %u beyond, %u undecided, %.2f ms\n",
                    seeds.size(), listed.lane.size(), listed.wave[0].size(), listed.wave[1].size(), listed.wave[2].size(), c->bs_n_beyond,
                    c->bs_n_undecided, c->ms_distance);
    }
    // what the kernels did not take or gave up on: in full, which gives d and end as well
    std::sort(undecided.begin(), undecided.end());
    if (int rc = best_sub_batch(c, v, undecided, f)) return rc;
    for (uint32_t a : undecided) {
        full[a] = 1u;
        h_d[a] = f.edits(a);
        h_end[a] = f.end(a);
    }

    // 3. the pick
    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(need_exact_all(n, c->bs_full, c->bs_edits, c->bs_out_end));
    HIP_TRY(need_exact_all(n_groups, c->bs_margin, c->bs_winner, c->bs_need, c->bs_realign));
    HIP_TRY(need_exact_all((size_t)n_groups + 1u, c->bs_group_offset, c->bs_need_at));
    HIP_TRY(c->scan_tmp.need_exact(bmscan::tmp_elems(n_groups) * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(c->bs_d.p, h_d.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->bs_end.p, h_end.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->bs_full.p, full.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->bs_group_offset.p, group_offset, ((size_t)n_groups + 1u) * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->bs_margin.p, margin, (size_t)n_groups * 4, hipMemcpyHostToDevice, c->stream));
    bmv::PickJob pj{};
    pj.d = c->bs_d.p;
    pj.end = c->bs_end.p;
    pj.full = c->bs_full.p;
    pj.group_offset = c->bs_group_offset.p;
    pj.margin = c->bs_margin.p;
    pj.n_groups = n_groups;
    pj.winner = c->bs_winner.p;
    pj.need = c->bs_need.p;
    pj.out_edits = c->bs_edits.p;
    pj.out_end = c->bs_out_end.p;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(bmv::bmv_best_pick_kernel, dim3((n_groups + bmv::kWave - 1u) / bmv::kWave), dim3(bmv::kWave), 0, c->stream, pj);
    HIP_TRY(hipGetLastError());
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->bs_need.p, c->bs_need_at.p, n_groups, reinterpret_cast<uint32_t *>(c->scan_tmp.p), c->stream));
    hipLaunchKernelGGL(bmv::bmv_best_compact_kernel, dim3((n_groups + 255u) / 256u), dim3(256), 0, c->stream, c->bs_need.p,
                       c->bs_need_at.p, c->bs_winner.p, n_groups, c->bs_realign.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    uint32_t n_realign = 0;
    HIP_TRY(hipMemcpyAsync(&n_realign, c->bs_need_at.p + n_groups, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_winner.data(), c->bs_winner.p, (size_t)n_groups * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_edits.data(), c->bs_edits.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h_out_end.data(), c->bs_out_end.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->ms_pick, c->ev0, c->ev1));
    f.ms += c->ms_pick;
    if (n_realign > n_groups) return fail(BMV_ERR_STATE, "%s: the pick lists %u winners for %u groups", who, n_realign, n_groups);
    std::vector<uint32_t> &realign = r.realign;
    realign.resize(n_realign);
    if (n_realign) HIP_TRY(hipMemcpy(realign.data(), c->bs_realign.p, (size_t)n_realign * 4, hipMemcpyDeviceToHost));
    for (uint32_t a : realign)
        if (a >= n) return fail(BMV_ERR_STATE, "%s: the pick lists alignment %u of %u", who, a, n);
    r.on_device = true;
    return BMV_OK;
}

// The last round of both: the alignments `which` -- chosen by a pick, without a full alignment so far -- in full; the distance
// round and the aligner are two computations of one quantity.
int best_realign(bmv_ctx *c, const char *who, const Views &v, const std::vector<uint32_t> &which, BestRounds &r) {
    if (int rc = best_sub_batch(c, v, which, r.f)) return rc;
    c->bs_n_realigned = (uint32_t)which.size();
    for (uint32_t a : which) {
        r.full[a] = 1u;
        if (r.f.edits(a) != r.d[a] || r.f.end(a) != r.end[a])
            return fail(BMV_ERR_STATE, "%s: alignment %u has %u edits ending at %u by the distance round, %lld ending at %u in full", who, a,
                        r.d[a], r.end[a], -(long long)r.f.score[a], r.f.end(a));
    }
    return BMV_OK;
}

// The alignments with keep[a] != 0 in batch order, everything else rejected -> the context, with what bmv_best returns.
void store_best(bmv_ctx *c, uint32_t n, uint32_t n_groups, uint64_t cells, const std::vector<uint8_t> &keep, BestRounds &r,
                uint64_t *total_cigar) {
    BestFull &f = r.f;
    for (uint32_t a = 0; a < n; a++) {
        if (keep[a]) continue;
        f.score[a] = BMV_REJECTED;
        f.begin[a] = 0;
        f.cig_len[a] = 0;
    }
    store_results(c, n, cells, f.ms, f.score, f.begin, f.pool, f.cig_at, f.cig_len, total_cigar);
    c->n_best = n;
    c->n_best_groups = n_groups;
    c->h_bs_winner = std::move(r.winner);
    c->h_bs_edits = std::move(r.edits);
    c->h_bs_end = std::move(r.out_end);
}

// ---- bmv_pair ----
// what the pair kernel takes beyond (edits, end): views without reads, the contigs, the groups, the fragment range
struct PairArgs {
    const uint64_t *text_start;
    const uint32_t *text_len;
    const uint8_t *text_rc;
    const uint32_t *query_len, *contig;
    uint32_t n;
    const uint32_t *group_offset;
    uint32_t n_groups, min_frag, max_frag;
};

int check_pair_args(const char *who, const PairArgs &a) {
    if (a.n_groups & 1u) return fail(BMV_ERR_ARG, "%s: %u groups, the mates of pair p are the groups 2p and 2p + 1", who, a.n_groups);
    if (a.min_frag > a.max_frag) return fail(BMV_ERR_ARG, "%s: min_frag %u is larger than max_frag %u", who, a.min_frag, a.max_frag);
    for (uint32_t x = 0; x < a.n; x++)
        if (a.text_start[x] >> 62) return fail(BMV_ERR_ARG, "alignment %u: text_start %llu does not fit the signed coordinates", x, (unsigned long long)a.text_start[x]);
    return BMV_OK;
}

// What the pair kernel and the span kernel read, on its way to the device (the context's device is current, n_groups > 0): the
// views without reads, the contigs and -- unless offsets_there -- the offsets; j's inputs point at them.
int upload_pair_inputs(bmv_ctx *c, const PairArgs &a, const uint32_t *d_edits, const uint32_t *d_end, bool offsets_there, bmv::PairJob &j) {
    const uint32_t n = a.n, n_groups = a.n_groups;
    HIP_TRY(need_exact_all(n, c->text_start, c->text_len, c->text_rc, c->query_len));
    HIP_TRY(c->bs_group_offset.need_exact((size_t)n_groups + 1u));
    if (n) {
        HIP_TRY(hipMemcpyAsync(c->text_start.p, a.text_start, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->text_len.p, a.text_len, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->text_rc.p, a.text_rc, (size_t)n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->query_len.p, a.query_len, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        if (a.contig) {
            HIP_TRY(c->pr_contig.need_exact(n));
            HIP_TRY(hipMemcpyAsync(c->pr_contig.p, a.contig, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        }
    }
    if (!offsets_there)
        HIP_TRY(hipMemcpyAsync(c->bs_group_offset.p, a.group_offset, ((size_t)n_groups + 1u) * 4, hipMemcpyHostToDevice, c->stream));
    j.text_start = c->text_start.p;
    j.text_len = c->text_len.p;
    j.text_rc = c->text_rc.p;
    j.query_len = c->query_len.p;
    j.edits = d_edits;
    j.end = d_end;
    j.contig = (n && a.contig) ? c->pr_contig.p : nullptr;
    j.group_offset = c->bs_group_offset.p;
    j.n_pairs = n_groups / 2u;
    j.min_frag = (int64_t)a.min_frag;
    j.max_frag = (int64_t)a.max_frag;
    return BMV_OK;
}

// The pair kernel over checked arguments, with edits and end where they lie on the device (offsets_there: bs_group_offset holds
// the offsets already); the results to the host, where bmv_pairs reads them.
int run_pair(bmv_ctx *c, const PairArgs &a, const uint32_t *d_edits, const uint32_t *d_end, bool offsets_there) {
    const uint32_t n_groups = a.n_groups, n_pairs = a.n_groups / 2u;
    c->h_pr_pick.assign(n_groups, BMV_BEYOND);
    c->h_pr_winner.assign(n_groups, BMV_BEYOND);
    c->h_pr_proper.assign(n_pairs, 0);
    c->h_pr_s1.assign(n_pairs, BMV_PAIR_NONE);
    c->h_pr_s2.assign(n_pairs, BMV_PAIR_NONE);
    c->ms_pair = 0.f;
    c->pr_combinations = 0;
    if (n_pairs == 0) return BMV_OK;
    for (uint32_t p = 0; p < n_pairs; p++)
        c->pr_combinations += (uint64_t)(a.group_offset[2u * p + 1u] - a.group_offset[2u * p]) * (a.group_offset[2u * p + 2u] - a.group_offset[2u * p + 1u]);
    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(need_exact_all(n_groups, c->pr_pick, c->pr_winner));
    HIP_TRY(need_exact_all(n_pairs, c->pr_proper, c->pr_s1, c->pr_s2));
    bmv::PairJob j{};
    if (const int rc = upload_pair_inputs(c, a, d_edits, d_end, offsets_there, j)) return rc;
    j.pick = c->pr_pick.p;
    j.winner = c->pr_winner.p;
    j.proper = c->pr_proper.p;
    j.s1 = c->pr_s1.p;
    j.s2 = c->pr_s2.p;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(bmv::bmv_pair_kernel, dim3((n_pairs + bmv::kPairWaves - 1u) / bmv::kPairWaves), dim3(bmv::kPairWaves * bmv::kWave), 0,
                       c->stream, j);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_pr_pick.data(), c->pr_pick.p, (size_t)n_groups * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_pr_winner.data(), c->pr_winner.p, (size_t)n_groups * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_pr_proper.data(), c->pr_proper.p, (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_pr_s1.data(), c->pr_s1.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_pr_s2.data(), c->pr_s2.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->ms_pair, c->ev0, c->ev1));
    return BMV_OK;
}

// ---- bmv_frag_spans ----
int check_frag_cap(const char *who, uint32_t cap) {
    if (cap < 1u || cap > bmv::kFragMaxCap) return fail(BMV_ERR_ARG, "%s: cap %u, a fragment cap is 1 .. %u", who, cap, bmv::kFragMaxCap);
    return BMV_OK;
}

// The span and histogram kernels over checked arguments (a.min_frag = 1, a.max_frag = cap), with edits and end where they lie
// on the device; spans and bins to the host, where bmv_frag reads them.  The bins are zeroed here, every call.
int run_frag(bmv_ctx *c, const PairArgs &a, const uint32_t *d_edits, const uint32_t *d_end, bool offsets_there) {
    const uint32_t n_pairs = a.n_groups / 2u, n_bins = a.max_frag + 1u;
    c->h_fr_span.assign(n_pairs, 0u);
    c->h_fr_hist.assign(n_bins, 0u);
    c->ms_frag = 0.f;
    c->fr_informative = 0;
    if (n_pairs == 0) return BMV_OK;
    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(c->fr_span.need_exact(n_pairs));
    HIP_TRY(c->fr_hist.need_exact(n_bins));
    bmv::FragJob j{};
    if (const int rc = upload_pair_inputs(c, a, d_edits, d_end, offsets_there, j.P)) return rc;
    j.span = c->fr_span.p;
    HIP_TRY(hipMemsetAsync(c->fr_hist.p, 0, (size_t)n_bins * 4, c->stream));
    // the histogram's grid: resident, and no more blocks than have n_bins spans each to count (a block's fixed cost is
    // zeroing and flushing its n_bins private bins)
    const bool in_lds = n_bins <= bmv::kFragLdsBins;
    const size_t lds_bytes = in_lds ? (size_t)n_bins * 4 : 0;
    int per_cu = 0, cus = 0;
    if (in_lds)
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bmv::bmv_frag_hist_lds_kernel, (int)bmv::kFragHistThreads, lds_bytes));
    else
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, bmv::bmv_frag_hist_global_kernel, (int)bmv::kFragHistThreads, 0));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->p.device));
    const uint32_t resident = (uint32_t)std::max(per_cu, 1) * (uint32_t)std::max(cus, 1);
    const uint32_t per_block = std::max(in_lds ? n_bins : 0u, bmv::kFragHistThreads * 8u);
    const uint32_t blocks = std::min(resident, (n_pairs + per_block - 1u) / per_block);
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(bmv::bmv_frag_span_kernel, dim3((n_pairs + bmv::kPairWaves - 1u) / bmv::kPairWaves), dim3(bmv::kPairWaves * bmv::kWave), 0,
                       c->stream, j);
    HIP_TRY(hipGetLastError());
    if (in_lds)
        hipLaunchKernelGGL(bmv::bmv_frag_hist_lds_kernel, dim3(blocks), dim3(bmv::kFragHistThreads), lds_bytes, c->stream, c->fr_span.p, n_pairs,
                           n_bins, c->fr_hist.p);
    else
        hipLaunchKernelGGL(bmv::bmv_frag_hist_global_kernel, dim3(blocks), dim3(bmv::kFragHistThreads), 0, c->stream, c->fr_span.p, n_pairs,
                           n_bins, c->fr_hist.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    std::vector<uint32_t> bins(n_bins);
    HIP_TRY(hipMemcpyAsync(c->h_fr_span.data(), c->fr_span.p, (size_t)n_pairs * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(bins.data(), c->fr_hist.p, (size_t)n_bins * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->ms_frag, c->ev0, c->ev1));
    std::copy(bins.begin(), bins.end(), c->h_fr_hist.begin());
    c->fr_informative = n_pairs - bins[0];
    if (getenv("BMV_LOG_CLASSES"))
        fprintf(stderr, "[bmv] frag: %u pairs, %u bins %s, %u blocks of %u lanes (%d resident per CU on %d CUs), %.3f ms\n", n_pairs, n_bins,
                in_lds ? "in LDS" : "by global atomics", blocks, bmv::kFragHistThreads, per_cu, cus, c->ms_frag);
    return BMV_OK;
}

// ---- bmv_paired_begin and bmv_paired_finish ----
// What begin leaves for finish: the caller's arrays (valid and unchanged until finish returns), the checked batch's cell count
// and the rounds' host state.  edits_there / offsets_there: bs_edits and bs_out_end / bs_group_offset still hold the restricted
// (edits, end) / the offsets -- bmv_pair and bmv_frag_spans put arrays of their own there and clear both (leave_pending).
struct PairedPending {
    Views v;
    const uint32_t *group_offset, *contig;
    uint32_t n_groups;
    uint64_t cells;
    BestRounds r;
    bool edits_there = false, offsets_there = false;
    PairedPending(const Views &v_, const uint32_t *group_offset_, const uint32_t *contig_, uint32_t n_groups_, uint64_t cells_)
        : v(v_), group_offset(group_offset_), contig(contig_), n_groups(n_groups_), cells(cells_), r(v_.n, n_groups_) {}
};

// bs_edits, bs_out_end and bs_group_offset are about to hold another call's arrays
void leave_pending(bmv_ctx *c) {
    if (c->pending) c->pending->edits_there = c->pending->offsets_there = false;
}

// edits and end of the rounds to the device, where the rounds themselves did not leave them
int upload_best_outputs(bmv_ctx *c, const BestRounds &r, uint32_t n) {
    if (!n) return BMV_OK;
    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(need_exact_all(n, c->bs_edits, c->bs_out_end));
    HIP_TRY(hipMemcpyAsync(c->bs_edits.p, r.edits.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->bs_out_end.p, r.out_end.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    return BMV_OK;
}

// The first half of bmv_align_paired under the name `who`: its checks except the range, the rounds, and for cap > 0 the spans.
int paired_begin(bmv_ctx *c, const char *who, const Views &v, const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin,
                 const uint32_t *hint, const uint32_t *contig, uint32_t min_frag, uint32_t max_frag, uint32_t cap, bool outputs_ok) {
    if (c) c->pending.reset();      // a new begin, accepted or refused, ends the one before it
    if (const int rc = check_view_args(c, who, v, outputs_ok && group_offset, true)) return rc;
    if (n_groups && !margin) return fail(BMV_ERR_ARG, "%s: null argument", who);
    if (const int rc = check_groups(who, group_offset, n_groups, v.n, hint)) return rc;
    const PairArgs a{v.text_start, v.text_len, v.text_rc, v.query_len, contig, v.n, group_offset, n_groups, min_frag, max_frag};
    if (const int rc = check_pair_args(who, a)) return rc;
    if (cap)
        if (const int rc = check_frag_cap(who, cap)) return rc;
    uint64_t cells = 0;
    if (const int rc = check_view_ranges(c, v, false, &cells)) return rc;

    // 1. and 2.
    auto pend = std::make_shared<PairedPending>(v, group_offset, contig, n_groups, cells);
    BestRounds &r = pend->r;
    if (const int rc = best_rounds(c, who, v, group_offset, n_groups, margin, hint, r)) return rc;
    // (every group its seed alone: the host holds the distances, nothing went to the device)
    if (!r.on_device)
        if (const int rc = upload_best_outputs(c, r, v.n)) return rc;
    pend->edits_there = v.n != 0;
    pend->offsets_there = r.on_device;
    if (cap) {
        PairArgs fa = a;
        fa.min_frag = 1u;
        fa.max_frag = cap;
        if (const int rc = run_frag(c, fa, c->bs_edits.p, c->bs_out_end.p, r.on_device)) return rc;
        r.f.ms += c->ms_frag;
        pend->offsets_there = pend->offsets_there || n_groups >= 2u;
    }
    c->pending = std::move(pend);
    return BMV_OK;
}

// The second half: 3. the pair kernel under the range, 4. the picks that have no full alignment yet, and the results.
int paired_finish(bmv_ctx *c, const char *who, uint32_t min_frag, uint32_t max_frag, uint64_t *total_cigar) {
    if (!c || !total_cigar) return fail(BMV_ERR_ARG, "%s: null argument", who);
    if (!c->pending) return fail(BMV_ERR_STATE, "%s: no bmv_paired_begin is pending (none made, finished already, or another call aligned since)", who);
    if (min_frag > max_frag) return fail(BMV_ERR_ARG, "%s: min_frag %u is larger than max_frag %u", who, min_frag, max_frag);
    const std::shared_ptr<PairedPending> pend = std::move(c->pending);      // (the full alignments below drop the context's)
    c->pending.reset();
    const Views &v = pend->v;
    BestRounds &r = pend->r;
    const uint32_t n = v.n, n_groups = pend->n_groups;
    const uint32_t *group_offset = pend->group_offset;
    const PairArgs a{v.text_start, v.text_len, v.text_rc, v.query_len, pend->contig, n, group_offset, n_groups, min_frag, max_frag};
    if (!pend->edits_there)
        if (const int rc = upload_best_outputs(c, r, n)) return rc;
    if (const int rc = run_pair(c, a, c->bs_edits.p, c->bs_out_end.p, pend->offsets_there)) return rc;
    r.f.ms += c->ms_pair;
    std::vector<uint8_t> picked(n, 0);
    std::vector<uint32_t> realign;
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint32_t x = c->h_pr_pick[g];
        if (x == BMV_BEYOND) continue;
        if (x < group_offset[g] || x >= group_offset[g + 1] || r.edits[x] == bmv::kBestBeyond)
            return fail(BMV_ERR_STATE, "%s: the pair kernel picked alignment %u for group %u", who, x, g);
        picked[x] = 1;
        if (!r.full[x]) realign.push_back(x);
    }
    if (const int rc = best_realign(c, who, v, realign, r)) return rc;
    store_best(c, n, n_groups, pend->cells, picked, r, total_cigar);
    return BMV_OK;
}

// ---- bmv_split and bmv_split_pick ----
// what the pick takes beyond the five arrays per alignment
struct SplitArgs {
    const uint32_t *contig;
    uint32_t n;
    const uint32_t *group_offset;
    uint32_t n_groups, min_score, max_overlap_permille, max_segments;
};

int check_split_args(const char *who, const SplitArgs &a) {
    if (a.min_score < 1u) return fail(BMV_ERR_ARG, "%s: min_score must be at least 1 (got %u)", who, a.min_score);
    if (a.max_overlap_permille > 1000u)
        return fail(BMV_ERR_ARG, "%s: max_overlap_permille must be in 0..1000 (got %u)", who, a.max_overlap_permille);
    if (a.max_segments < 1u || a.max_segments > BMV_SPLIT_MAX_SEGMENTS)
        return fail(BMV_ERR_ARG, "%s: max_segments must be in 1..%u (got %u)", who, BMV_SPLIT_MAX_SEGMENTS, a.max_segments);
    return BMV_OK;
}

// what a checked call of either leaves before anything runs: n alignments of zeros, every group without a segment
void reset_split(bmv_ctx *c, const SplitArgs &a, uint64_t columns) {
    const size_t slots = (size_t)a.n_groups * a.max_segments;
    c->h_sp_score.assign(a.n, 0);
    c->h_sp_g_lo.assign(a.n, 0);
    c->h_sp_g_hi.assign(a.n, 0);
    c->h_sp_q_lo.assign(a.n, 0);
    c->h_sp_q_hi.assign(a.n, 0);
    c->h_sp_n_seg.assign(a.n_groups, 0);
    c->h_sp_seg.assign(slots, BMV_BEYOND);
    c->h_sp_s2.assign(slots, BMV_SPLIT_NONE);
    c->ms_sp_range = c->ms_sp_pick = 0.f;
    c->sp_columns = columns;
    c->sp_segments = 0;
}

// The pick kernel over checked arguments (n_groups > 0), with score, q_lo, q_hi, g_lo, g_hi in sp_* and text_rc in the views'
// buffer on the device -- or about to be written there by `range`, which launches the range kernel on the context's stream
// (bmv_split; bmv_split_pick passes one that launches nothing and says so).  The groups go up first, so that the two kernels
// run back to back between three events.  The pick's results to the host, where bmv_segments reads them.
template <typename Range>
int run_split_pick(bmv_ctx *c, const SplitArgs &a, bool has_range, Range range) {
    const size_t n = a.n, n_groups = a.n_groups, slots = n_groups * a.max_segments;
    HIP_TRY(c->sp_group_offset.need_exact(n_groups + 1u));
    HIP_TRY(c->sp_n_seg.need_exact(n_groups));
    HIP_TRY(need_exact_all(slots, c->sp_seg, c->sp_s2));
    HIP_TRY(hipMemcpyAsync(c->sp_group_offset.p, a.group_offset, (n_groups + 1u) * 4, hipMemcpyHostToDevice, c->stream));
    if (n && a.contig) {
        HIP_TRY(c->sp_contig.need_exact(n));
        HIP_TRY(hipMemcpyAsync(c->sp_contig.p, a.contig, n * 4, hipMemcpyHostToDevice, c->stream));
    }
    bmv::SplitPickJob j{};
    j.score = c->sp_score.p;
    j.q_lo = c->sp_q_lo.p;
    j.q_hi = c->sp_q_hi.p;
    j.g_lo = c->sp_g_lo.p;
    j.g_hi = c->sp_g_hi.p;
    j.text_rc = c->text_rc.p;
    j.contig = (n && a.contig) ? c->sp_contig.p : nullptr;
    j.group_offset = c->sp_group_offset.p;
    j.n_groups = a.n_groups;
    j.min_score = (int64_t)a.min_score;
    j.max_overlap_permille = a.max_overlap_permille;
    j.max_segments = a.max_segments;
    j.n_seg = c->sp_n_seg.p;
    j.seg = c->sp_seg.p;
    j.s2 = c->sp_s2.p;
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    HIP_TRY(range());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    hipLaunchKernelGGL(bmv::bmv_split_pick_kernel, dim3((a.n_groups + bmv::kSplitWaves - 1u) / bmv::kSplitWaves), dim3(bmv::kSplitWaves * 64u),
                       0, c->stream, j);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev2, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_sp_n_seg.data(), c->sp_n_seg.p, n_groups * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_sp_seg.data(), c->sp_seg.p, slots * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_sp_s2.data(), c->sp_s2.p, slots * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->ms_sp_pick, c->ev1, c->ev2));
    if (has_range) HIP_TRY(hipEventElapsedTime(&c->ms_sp_range, c->ev0, c->ev1));
    for (const uint32_t k : c->h_sp_n_seg) c->sp_segments += k;
    return BMV_OK;
}

}  // namespace

extern "C" {

const char *bmv_last_error(void) { return g_err; }

int bmv_create(const bmv_params *params, bmv_ctx **out) {
    if (!params || !out) return fail(BMV_ERR_ARG, "bmv_create: null argument");
    *out = nullptr;
    if (params->max_query_len == 0 || params->max_query_len > 65536)
        return fail(BMV_ERR_UNSUPPORTED, "max_query_len must be in 1..65536 (got %u)", params->max_query_len);
    if (params->max_text_len == 0 || params->max_text_len > 81920)
        return fail(BMV_ERR_UNSUPPORTED, "max_text_len must be in 1..81920 (got %u)", params->max_text_len);
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (params->device < 0 || params->device >= n_dev)
        return fail(BMV_ERR_HIP, "device %d not available (%d HIP devices)", params->device, n_dev);
    HIP_TRY(hipSetDevice(params->device));
    bmv_ctx *c = new bmv_ctx();
    c->p = *params;
    // checkpoints of the alignments in flight: a third of the free HBM, 1..96 GiB (a 30-kbp alignment keeps 19 MB and
    // is one wave: long reads want thousands in flight, and a mixed batch wants several length classes in flight
    // together -- 40 000 alignments of 1 .. 30 kbp: 26.8 / 31.2 / 32.8 / 35.0 T cell updates/s with 48 / 72 / 96 / 140 GB);
    // BMV_SCRATCH_MB overrides (tests use it to force chunking)
    size_t free_b = 0, total_b = 0;
    c->scratch_bytes = (size_t)8 << 30;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        c->scratch_bytes = std::min<size_t>(std::max<size_t>(free_b / 3, (size_t)1 << 30), (size_t)96 << 30);
    if (const char *env = getenv("BMV_SCRATCH_MB")) {
        const long v = strtol(env, nullptr, 10);
        if (v > 0) c->scratch_bytes = (size_t)v << 20;
    }
    uint8_t lut[256];
    bmhip::build_dna4_lut(lut);
    bool side_ok = true;
    for (uint32_t k = 0; k < kSideStreams; k++)
        side_ok = side_ok && hipStreamCreateWithFlags(&c->side[k], hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreateWithFlags(&c->side_done[k], hipEventDisableTiming) == hipSuccess;
    if (!side_ok || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess || hipEventCreate(&c->ev2) != hipSuccess ||
        c->lut.need_exact(256) != hipSuccess || hipMemcpy(c->lut.p, lut, 256, hipMemcpyHostToDevice) != hipSuccess) {
        bmv_destroy(c);
        return fail(BMV_ERR_HIP, "bmv_create: %s", hipGetErrorString(hipGetLastError()));
    }
    *out = c;
    return BMV_OK;
}

// What has an order: the device, the streams drained before anything of theirs goes, the buffers (`delete`: every DevBuf of
// the context frees itself) while the device is still the context's.
void bmv_destroy(bmv_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->p.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (uint32_t k = 0; k < kSideStreams; k++) {
        if (c->side[k]) {
            (void)hipStreamSynchronize(c->side[k]);
            (void)hipStreamDestroy(c->side[k]);
        }
        if (c->side_done[k]) (void)hipEventDestroy(c->side_done[k]);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev2) (void)hipEventDestroy(c->ev2);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmv_load_genome(bmv_ctx *c, const uint8_t *bases, uint64_t n_bases) {
    if (!c || (n_bases && !bases)) return fail(BMV_ERR_ARG, "bmv_load_genome: null argument");
    return load_genome(c, &bases, &n_bases, 1, n_bases);
}

int bmv_load_genome_records(bmv_ctx *c, const uint8_t *const *rec, const uint64_t *rec_len, uint32_t n_records) {
    if (!c || (n_records && (!rec || !rec_len))) return fail(BMV_ERR_ARG, "bmv_load_genome_records: null argument");
    uint64_t n_bases = 0;
    for (uint32_t r = 0; r < n_records; r++) {
        if (rec_len[r] && !rec[r]) return fail(BMV_ERR_ARG, "bmv_load_genome_records: record %u is null", r);
        n_bases += rec_len[r];
    }
    return load_genome(c, rec, rec_len, n_records, n_bases);
}

// The batch by length class (partition_classes), a plan per class (plan_class), the plans cut into pieces (cut_pieces) and
// the pieces packed into rounds (round_end, run_round).
int bmv_align(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
              const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
              uint32_t n, uint64_t *total_cigar) {
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    uint64_t cells = 0;
    if (const int rc = check_views(c, "bmv_align", v, total_cigar != nullptr, true, true, &cells)) return rc;
    c->pending.reset();         // (as store_results: every other call of the row comes through one of the two)
    c->n_last = n;
    c->n_cells = cells;
    c->ms_kernels = 0.f;
    c->h_score.assign(n, 0);
    c->h_begin.assign(n, 0);
    c->h_offset.assign((size_t)n + 1, 0);
    c->h_cigar.clear();
    *total_cigar = 0;
    if (n == 0) return BMV_OK;

    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(need_exact_all(n, c->out_score, c->out_begin, c->order));
    if (const int rc = upload_views(c, v)) return rc;
    const ClassOrder co = partition_classes(query_len, n);
    HIP_TRY(hipMemcpyAsync(c->order.p, co.order.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    CigarStash stash;
    stash.in_place = co.n_classes == 1;                         // then order is the identity and the CIGARs arrive in place
    if (!stash.in_place) {
        stash.len.assign(n, 0);
        stash.at.assign(n, 0);
    }
    const size_t budget = scratch_budget(c, query_len, n, co.n_classes);
    std::vector<Plan> plans;
    for (uint32_t k = 0; k < kClasses; k++) {
        if (co.lo[k + 1] == co.lo[k]) continue;
        Plan pl;
        if (const int rc = plan_class(v, co.order, co.lo[k], co.lo[k + 1] - co.lo[k], budget, pl)) return rc;
        plans.push_back(pl);
    }
    const uint32_t stop_after = getenv("BMV_STOP_AFTER") ? (uint32_t)atoi(getenv("BMV_STOP_AFTER")) : 0u;   // phase timing
    const bool serial = getenv("BMV_SERIAL_CLASSES") != nullptr;
    const std::vector<Todo> todo = cut_pieces(plans, budget, serial);
    for (size_t at = 0; at < todo.size();) {
        const size_t end = round_end(todo, at, budget, serial);
        if (const int rc = run_round(c, todo, at, end, co.order, stop_after, stash)) return rc;
        at = end;
    }
    if (!stash.in_place) pack_cigars(c, n, stash.pool, stash.at, stash.len);
    c->h_offset[n] = c->h_cigar.size();
    HIP_TRY(hipMemcpy(c->h_score.data(), c->out_score.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c->h_begin.data(), c->out_begin.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    *total_cigar = c->h_cigar.size();
    return BMV_OK;
}

// Alignments beyond the context's limits (bmv_long.hip.h): the batch is split, what bmv_align takes goes through bmv_align
// unchanged, the rest through tiles of 64 lanes x kLongCw words x `chunk` steps launched by anti-diagonal.  Their scratch
// (checkpoints, deltas, planes, packed text; reversed CIGAR entries) is planned against scratch_bytes: they are taken in
// pieces that fit it, and one that does not fit alone fails the call before anything runs.
int bmv_align_long(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                   const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                   uint32_t n, uint64_t *total_cigar) {
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    uint64_t cells = 0;
    if (const int rc = check_views(c, "bmv_align_long", v, total_cigar != nullptr, true, false, &cells)) return rc;
    const uint32_t from = long_from();
    std::vector<uint32_t> shorts, longs;
    for (uint32_t a = 0; a < n; a++) (goes_long(c, query_len[a], text_len[a], from) ? longs : shorts).push_back(a);
    if (longs.empty())                                          // nothing beyond the limits: bmv_align's own path
        return bmv_align(c, reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, total_cigar);

    // the long ones: tile shape and scratch of each, refused before anything runs if one cannot fit the budget on its own
    constexpr uint32_t CW = (uint32_t)bmv::kLongCw;
    uint32_t max_chunk = 8192;                                  // time steps per tile (BMV_LONG_CHUNK: experiments)
    if (const char *env = getenv("BMV_LONG_CHUNK")) max_chunk = (uint32_t)std::min<long>(std::max<long>(atol(env), 16), 65536) / 16u * 16u;
    const uint64_t budget = c->scratch_bytes;
    struct Long {
        bmv::LongSlot s;
        uint64_t bytes, ops_stride;
    };
    std::vector<Long> todo;
    std::vector<uint32_t> empty_query;                          // (score 0, begin n, no CIGAR: nothing to run)
    for (uint32_t a : longs) {
        const uint32_t m = query_len[a], nn = text_len[a];
        if (m == 0) {
            empty_query.push_back(a);
            continue;
        }
        bmv::LongSlot s{};
        s.a = a;
        s.m = m;
        s.n = nn;
        s.W = (uint32_t)(((uint64_t)m + 63u) / 64u);
        const uint32_t lanes = (s.W + CW - 1u) / CW;
        s.n_strips = (lanes + 63u) / 64u;
        const uint64_t span = (uint64_t)nn + lanes - 1u;        // time steps: the last lane passes column n at n + lanes - 1
        s.chunk = (uint32_t)std::min<uint64_t>(max_chunk, std::max<uint64_t>(16u, (span + 15u) / 16u * 16u));
        const uint64_t n_chunks = std::max<uint64_t>(1u, (span + s.chunk - 1u) / s.chunk);
        if (n_chunks * s.chunk + 64u >= ((uint64_t)1 << 32))
            return fail(BMV_ERR_UNSUPPORTED, "alignment %u: a query of %u bases against %u text bases does not fit the 32-bit step counter", a, m, nn);
        s.n_chunks = (uint32_t)n_chunks;
        s.n_blocks = (uint32_t)(n_chunks * s.chunk / 16u + 1u);
        const uint64_t bytes = bmv::long_region_bytes(s.W, nn, s.n_blocks), ops_stride = (uint64_t)m + nn + 1u;
        if (bytes + ops_stride * 4u > budget)
            return fail(BMV_ERR_UNSUPPORTED, "alignment %u: a query of %u bases against %u text bases needs %llu bytes of trace; the scratch holds %llu (BMV_SCRATCH_MB)",
                        a, m, nn, (unsigned long long)(bytes + ops_stride * 4u), (unsigned long long)budget);
        todo.push_back({s, bytes, ops_stride});
    }

    std::vector<int32_t> score(n, 0);
    std::vector<uint32_t> begin(n, 0);
    std::vector<uint64_t> cig_at(n, 0), cig_len(n, 0);
    std::vector<uint32_t> pool;                                 // CIGAR entries, alignment by alignment in any order
    float ms_total = 0.f;
    if (!shorts.empty()) {                                      // exactly what bmv_align does with them on their own
        SubResults sub;
        if (int rc = align_sub_batch(c, v, shorts, sub)) return rc;
        for (size_t k = 0; k < shorts.size(); k++) {
            const uint32_t a = shorts[k];
            score[a] = sub.score[k];
            begin[a] = sub.begin[k];
            cig_at[a] = sub.offset[k];
            cig_len[a] = sub.len(k);
        }
        pool = std::move(sub.cigar);
        ms_total += sub.ms;
    }
    for (uint32_t a : empty_query) begin[a] = text_len[a];      // H[0][j] = 0 everywhere: the last column

    HIP_TRY(hipSetDevice(c->p.device));
    HIP_TRY(need_exact_all(n, c->out_score, c->out_begin));
    if (const int rc = upload_views(c, v)) return rc;
    std::vector<bmv::LongSlot> slots;
    std::vector<uint32_t> tiles, h_nops, h_packed;
    std::vector<uint64_t> tile_at;
    std::vector<int32_t> h_score(n);
    std::vector<uint32_t> h_begin(n);
    // pieces: as many as fit the budget together (at least one; the uniform CIGAR stride is the longest's), planned before
    // the scratch is sized once for the largest (growing a 90-GB buffer piece by piece costs seconds in hipMalloc)
    struct LongPiece {
        size_t p0, p1;
        uint64_t sum, ops_stride;
    };
    std::vector<LongPiece> pieces;
    uint64_t max_sum = 0, max_ops = 0, max_count = 0;
    for (size_t p0 = 0; p0 < todo.size();) {
        LongPiece pc{p0, p0, 0, 0};
        while (pc.p1 < todo.size()) {
            const uint64_t st = std::max(pc.ops_stride, todo[pc.p1].ops_stride);
            if (pc.p1 > p0 && pc.sum + todo[pc.p1].bytes + (pc.p1 - p0 + 1u) * st * 4u > budget) break;
            pc.sum += todo[pc.p1].bytes;
            pc.ops_stride = st;
            pc.p1++;
        }
        max_sum = std::max(max_sum, pc.sum);
        max_ops = std::max<uint64_t>(max_ops, (pc.p1 - p0) * pc.ops_stride);
        max_count = std::max<uint64_t>(max_count, pc.p1 - p0);
        pieces.push_back(pc);
        p0 = pc.p1;
    }
    HIP_TRY(c->trace.need_exact((size_t)(max_sum + 7u) / 8u));
    HIP_TRY(c->ops_rev.need_exact((size_t)max_ops));
    HIP_TRY(c->nops.need_exact((size_t)max_count));
    HIP_TRY(c->offsets.need_exact((size_t)max_count + 1u));
    for (const LongPiece &pc : pieces) {
        const size_t p0 = pc.p0, p1 = pc.p1;
        const uint64_t sum = pc.sum, ops_stride = pc.ops_stride;
        const uint32_t count = (uint32_t)(p1 - p0);
        slots.clear();
        uint64_t at = 0, max_items = 1;
        uint32_t max_d = 0, chunk = 16;
        for (size_t q = p0; q < p1; q++) {
            bmv::LongSlot s = todo[q].s;
            s.at = at;
            at += todo[q].bytes;
            slots.push_back(s);
            max_d = std::max(max_d, s.n_strips + s.n_chunks - 2u);
            max_items = std::max<uint64_t>(max_items, std::max(s.W, bmv::long_text_words(s.n)));
            chunk = std::max(chunk, s.chunk);
        }
        // the tiles of launch d: every (slot, strip) with strip + chunk = d
        tiles.clear();
        tile_at.assign((size_t)max_d + 2u, 0);
        for (uint32_t d = 0; d <= max_d; d++) {
            tile_at[d] = tiles.size() / 2u;
            for (uint32_t q = 0; q < count; q++) {
                const bmv::LongSlot &s = slots[q];
                const uint32_t lo = d + 1u > s.n_chunks ? d + 1u - s.n_chunks : 0u, hi = std::min(d, s.n_strips - 1u);
                for (uint32_t st = lo; st <= hi && lo <= hi; st++) {
                    tiles.push_back(q);
                    tiles.push_back(st);
                }
            }
        }
        tile_at[(size_t)max_d + 1u] = tiles.size() / 2u;
        HIP_TRY(c->long_slots.need_exact(slots.size() * sizeof(bmv::LongSlot)));
        HIP_TRY(c->long_tiles.need_exact(tiles.size()));
        HIP_TRY(hipMemcpyAsync(c->long_slots.p, slots.data(), slots.size() * sizeof(bmv::LongSlot), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->long_tiles.p, tiles.data(), tiles.size() * 4u, hipMemcpyHostToDevice, c->stream));
        bmv::LongJob j{};
        fill_views(c, j);
        j.slots = reinterpret_cast<const bmv::LongSlot *>(c->long_slots.p);
        j.count = count;
        j.scratch = reinterpret_cast<uint8_t *>(c->trace.p);
        j.ops_rev = c->ops_rev.p;
        j.ops_stride = (uint32_t)ops_stride;
        j.out_score = c->out_score.p;
        j.out_begin = c->out_begin.p;
        j.out_nops = c->nops.p;
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
        const uint32_t per_slot = (uint32_t)std::min<uint64_t>(256u, (max_items + 255u) / 256u);
        hipLaunchKernelGGL(bmv::bmv_long_prep_kernel<bmv::kLongCw>, dim3(count * per_slot), dim3(256), 0, c->stream, j, per_slot);
        HIP_TRY(hipGetLastError());
        const size_t lds = ((size_t)chunk / 16u + 5u) * 4u;
        for (uint32_t d = 0; d <= max_d; d++) {
            const uint64_t nt = tile_at[(size_t)d + 1u] - tile_at[d];
            if (nt == 0) continue;
            j.tiles = c->long_tiles.p + 2u * tile_at[d];
            j.d = d;
            hipLaunchKernelGGL(bmv::bmv_long_tile_kernel<bmv::kLongCw>, dim3((uint32_t)nt), dim3(bmv::kWave), lds, c->stream, j);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(bmv::bmv_long_traceback_kernel<bmv::kLongCw>, dim3((count + bmv::kWave - 1u) / bmv::kWave), dim3(bmv::kWave), 0,
                           c->stream, j);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        if (int rc = collect_cigars(c, {{c->ops_rev.p, (uint32_t)ops_stride, 0u, count}}, count, h_nops, h_packed)) return rc;
        uint64_t from_at = pool.size();
        for (uint32_t q = 0; q < count; q++) {
            cig_at[slots[q].a] = from_at;
            cig_len[slots[q].a] = h_nops[q];
            from_at += h_nops[q];
        }
        pool.insert(pool.end(), h_packed.begin(), h_packed.end());
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_total += ms;
        if (getenv("BMV_LOG_CLASSES"))
            fprintf(stderr, "[bmv] long piece of %u alignment(s), %zu tiles in %u launches, %.2f GB of scratch, %.2f ms\n", count,
                    tiles.size() / 2u, max_d + 1u, (double)sum / 1e9, ms);
    }
    HIP_TRY(hipMemcpy(h_score.data(), c->out_score.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_begin.data(), c->out_begin.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (const Long &l : todo) {
        score[l.s.a] = h_score[l.s.a];
        begin[l.s.a] = h_begin[l.s.a];
    }
    store_results(c, n, cells, ms_total, score, begin, pool, cig_at, cig_len, total_cigar);   // as bmv_align leaves them
    return BMV_OK;
}

// The batch under an edit bound per alignment (include/bmv.h).  A screen (bmv_screen.hip.h) rejects what it can prove to be
// beyond its bound, the survivors' indices are compacted on the device, the survivors go through bmv_align_long -- which is
// bmv_align itself for everything within the context's limits -- as a batch of their own, and the results are scattered back
// to batch order.  The screen only ever rejects: the bound is applied to every survivor's score afterwards, which is what
// makes the contract exact for the alignments the screen does not take (k >= query length: nothing to reject; beyond the
// limits, or from BMV_LONG_FROM on) or gives up on (a band that outgrows the wave).
int bmv_align_bounded(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start,
                      const uint32_t *text_len, const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len,
                      const uint32_t *max_edits, uint32_t n, uint64_t *total_cigar) {
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    uint64_t cells = 0;
    if (const int rc = check_views(c, "bmv_align_bounded", v, total_cigar != nullptr, max_edits != nullptr, false, &cells)) return rc;
    const uint32_t from = long_from();
    BandLists screened;
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t m = query_len[a], k = max_edits[a];
        if (goes_long(c, m, text_len[a], from) || k >= m) continue;     // not screened: the bound is applied to the score
        screened.add(a, m, k);
    }
    c->n_rejected = 0;
    c->screen_cells = 0;
    c->ms_screen = 0.f;
    if (n == 0) return bmv_align_long(c, reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n, total_cigar);

    std::vector<uint32_t> survivors;
    const size_t n_screened = screened.size();
    if (n_screened == 0) {
        survivors.resize(n);
        for (uint32_t a = 0; a < n; a++) survivors[a] = a;
    } else {
        HIP_TRY(hipSetDevice(c->p.device));
        HIP_TRY(need_exact_all(n, c->max_edits, c->keep, c->survivors));
        HIP_TRY(need_exact_all((size_t)n + 1u, c->keep_at));
        HIP_TRY(c->screen_list.need_exact(n_screened));
        HIP_TRY(c->screen_count.need_exact(1));
        HIP_TRY(c->scan_tmp.need_exact(bmscan::tmp_elems(n) * sizeof(uint32_t)));
        if (const int rc = upload_views(c, v)) return rc;
        HIP_TRY(hipMemcpyAsync(c->max_edits.p, max_edits, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        std::vector<uint32_t> ones(n, 1u);
        HIP_TRY(hipMemcpyAsync(c->keep.p, ones.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        if (const int rc = upload_band_lists(c, screened, c->screen_list.p)) return rc;
        HIP_TRY(hipMemsetAsync(c->screen_count.p, 0, sizeof(unsigned long long), c->stream));
        bmv::ScreenJob j{};
        fill_views(c, j);
        j.max_edits = c->max_edits.p;
        j.keep = c->keep.p;
        j.cells = c->screen_count.p;
        using screen_fn = void (*)(bmv::ScreenJob);
        static const screen_fn per_lane[kLaneWords + 1] = {nullptr,
                                                           bmv::bmv_screen_lane_kernel<1>, bmv::bmv_screen_lane_kernel<2>,
                                                           bmv::bmv_screen_lane_kernel<3>, bmv::bmv_screen_lane_kernel<4>,
                                                           bmv::bmv_screen_lane_kernel<5>, bmv::bmv_screen_lane_kernel<6>,
                                                           bmv::bmv_screen_lane_kernel<7>, bmv::bmv_screen_lane_kernel<8>};
        static const screen_fn per_wave[3] = {bmv::bmv_screen_wave_kernel<1>, bmv::bmv_screen_wave_kernel<2>, bmv::bmv_screen_wave_kernel<4>};
        if (const int rc = launch_bands(c, screened, c->screen_list.p, per_lane, per_wave, j)) return rc;
        // the survivors' indices, compacted on the device
        HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->keep.p, c->keep_at.p, n, reinterpret_cast<uint32_t *>(c->scan_tmp.p), c->stream));
        hipLaunchKernelGGL(bmv::bmv_screen_compact_kernel, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, c->keep.p, c->keep_at.p, n,
                           c->survivors.p);
        HIP_TRY(hipGetLastError());
        uint32_t n_keep = 0;
        unsigned long long steps = 0;
        HIP_TRY(hipMemcpyAsync(&n_keep, c->keep_at.p + n, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&steps, c->screen_count.p, sizeof steps, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        survivors.resize(n_keep);
        if (n_keep) HIP_TRY(hipMemcpy(survivors.data(), c->survivors.p, (size_t)n_keep * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipEventElapsedTime(&c->ms_screen, c->ev0, c->ev1));
        c->screen_cells = 64u * (uint64_t)steps;
        if (getenv("BMV_LOG_CLASSES"))
            fprintf(stderr, "[bmv] screen: %zu per lane, %zu / %zu / %zu per wave at 1 / 2 / 4 words a lane; %u of %u let through, %.2f ms\n",
                    screened.lane.size(), screened.wave[0].size(), screened.wave[1].size(), screened.wave[2].size(), n_keep, n, c->ms_screen);
    }

    // the survivors as a batch of their own, in batch order
    SubResults sub;
    if (int rc = align_sub_batch(c, v, survivors, sub)) return rc;
    // back to batch order; the bound applied to what was let through
    std::vector<int32_t> score(n, BMV_REJECTED);
    std::vector<uint32_t> begin(n, 0);
    std::vector<uint64_t> cig_at(n, 0), cig_len(n, 0);
    uint32_t accepted = 0;
    for (size_t s = 0; s < survivors.size(); s++) {
        const uint32_t a = survivors[s];
        if (-(int64_t)sub.score[s] > (int64_t)max_edits[a]) continue;   // rejected: an empty CIGAR
        score[a] = sub.score[s];
        begin[a] = sub.begin[s];
        cig_at[a] = sub.offset[s];
        cig_len[a] = sub.len(s);
        accepted++;
    }
    store_results(c, n, cells, sub.ms + c->ms_screen, score, begin, sub.cigar, cig_at, cig_len, total_cigar);
    c->n_rejected = n - accepted;
    return BMV_OK;
}

int bmv_last_bounded_stats(bmv_ctx *c, uint32_t *n_rejected, uint64_t *screen_cells, float *ms_screen) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_bounded_stats: null context");
    if (n_rejected) *n_rejected = c->n_rejected;
    if (screen_cells) *screen_cells = c->screen_cells;
    if (ms_screen) *ms_screen = c->ms_screen;
    return BMV_OK;
}

// The best alignment of each group (include/bmv.h, bmv_best.hip.h).  Four rounds: best_rounds' three, then the winners that
// have no full alignment yet in full.  Every full alignment is bmv_align_long's on a batch of its own, so what the winners carry
// is what that call gives them.
int bmv_align_best(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                   const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
                   const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                   uint64_t *total_cigar) {
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    if (const int rc = check_view_args(c, "bmv_align_best", v, total_cigar && group_offset, true)) return rc;
    if (n_groups && !margin) return fail(BMV_ERR_ARG, "bmv_align_best: null argument");
    if (const int rc = check_groups("bmv_align_best", group_offset, n_groups, n, hint)) return rc;
    uint64_t cells = 0;
    if (const int rc = check_view_ranges(c, v, false, &cells)) return rc;

    BestRounds r(n, n_groups);
    if (const int rc = best_rounds(c, "bmv_align_best", v, group_offset, n_groups, margin, hint, r)) return rc;
    // 4. the winners that have no full alignment yet
    if (const int rc = best_realign(c, "bmv_align_best", v, r.realign, r)) return rc;

    // the winners in batch order, everything else rejected
    std::vector<uint8_t> wins(n, 0);
    for (uint32_t g = 0; g < n_groups; g++)
        if (r.winner[g] != bmv::kBestBeyond) wins[r.winner[g]] = 1;
    store_best(c, n, n_groups, cells, wins, r, total_cigar);
    return BMV_OK;
}

// The pair-aware pick alone (include/bmv.h, bmv_pair.hip.h): edits and end go to the device, the kernel runs, bmv_pairs reads.
int bmv_pair(bmv_ctx *c, const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc, const uint32_t *query_len,
             const uint32_t *edits, const uint32_t *end, const uint32_t *contig, uint32_t n, const uint32_t *group_offset,
             uint32_t n_groups, uint32_t min_frag, uint32_t max_frag) {
    if (!c || !group_offset || (n && (!text_start || !text_len || !text_rc || !query_len || !edits || !end)))
        return fail(BMV_ERR_ARG, "bmv_pair: null argument");
    if (const int rc = check_groups("bmv_pair", group_offset, n_groups, n, nullptr)) return rc;
    const PairArgs a{text_start, text_len, text_rc, query_len, contig, n, group_offset, n_groups, min_frag, max_frag};
    if (const int rc = check_pair_args("bmv_pair", a)) return rc;
    HIP_TRY(hipSetDevice(c->p.device));
    leave_pending(c);
    HIP_TRY(need_exact_all(n, c->bs_edits, c->bs_out_end));
    if (n) {
        HIP_TRY(hipMemcpyAsync(c->bs_edits.p, edits, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->bs_out_end.p, end, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
    return run_pair(c, a, c->bs_edits.p, c->bs_out_end.p, false);
}

int bmv_pairs(bmv_ctx *c, uint32_t *out_pick, uint8_t *out_proper, uint64_t *out_s1, uint64_t *out_s2, uint32_t *out_winner) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_pairs: null context");
    copy_out(out_pick, c->h_pr_pick);
    copy_out(out_proper, c->h_pr_proper);
    copy_out(out_s1, c->h_pr_s1);
    copy_out(out_s2, c->h_pr_s2);
    copy_out(out_winner, c->h_pr_winner);
    return BMV_OK;
}

int bmv_last_pair_stats(bmv_ctx *c, float *ms_pair, uint64_t *n_combinations) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_pair_stats: null context");
    if (ms_pair) *ms_pair = c->ms_pair;
    if (n_combinations) *n_combinations = c->pr_combinations;
    return BMV_OK;
}

// bmv_align_best for pairs (include/bmv.h): best_rounds' three rounds leave (edits, end) within best + margin on the device --
// whatever the hints were --, the pair kernel picks over them there, and the picks that have no full alignment yet get one.
int bmv_align_paired(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                     const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
                     const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                     const uint32_t *contig, uint32_t min_frag, uint32_t max_frag, uint64_t *total_cigar) {
    // one copy of the steps: begin without the spans, then finish
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    if (const int rc = paired_begin(c, "bmv_align_paired", v, group_offset, n_groups, margin, hint, contig, min_frag, max_frag, 0u, total_cigar != nullptr))
        return rc;
    return paired_finish(c, "bmv_align_paired", min_frag, max_frag, total_cigar);
}

// bmv_align_paired in two halves (include/bmv.h): between them the caller reads the spans of this and of other contexts and
// settles on one range.
int bmv_paired_begin(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                     const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, uint32_t n,
                     const uint32_t *group_offset, uint32_t n_groups, const uint32_t *margin, const uint32_t *hint,
                     const uint32_t *contig, uint32_t cap) {
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    return paired_begin(c, "bmv_paired_begin", v, group_offset, n_groups, margin, hint, contig, 1u, 1u, cap, true);
}

int bmv_paired_finish(bmv_ctx *c, uint32_t min_frag, uint32_t max_frag, uint64_t *total_cigar) {
    return paired_finish(c, "bmv_paired_finish", min_frag, max_frag, total_cigar);
}

// The spans and their histogram alone (include/bmv.h, bmv_frag.hip.h): edits and end go to the device, the two kernels run,
// bmv_frag reads.
int bmv_frag_spans(bmv_ctx *c, const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc, const uint32_t *query_len,
                   const uint32_t *edits, const uint32_t *end, const uint32_t *contig, uint32_t n, const uint32_t *group_offset,
                   uint32_t n_groups, uint32_t cap) {
    if (!c || !group_offset || (n && (!text_start || !text_len || !text_rc || !query_len || !edits || !end)))
        return fail(BMV_ERR_ARG, "bmv_frag_spans: null argument");
    if (const int rc = check_groups("bmv_frag_spans", group_offset, n_groups, n, nullptr)) return rc;
    const PairArgs a{text_start, text_len, text_rc, query_len, contig, n, group_offset, n_groups, 1u, cap};
    if (const int rc = check_frag_cap("bmv_frag_spans", cap)) return rc;
    if (const int rc = check_pair_args("bmv_frag_spans", a)) return rc;
    HIP_TRY(hipSetDevice(c->p.device));
    leave_pending(c);
    HIP_TRY(need_exact_all(n, c->bs_edits, c->bs_out_end));
    if (n) {
        HIP_TRY(hipMemcpyAsync(c->bs_edits.p, edits, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->bs_out_end.p, end, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
    return run_frag(c, a, c->bs_edits.p, c->bs_out_end.p, false);
}

int bmv_frag(bmv_ctx *c, uint32_t *out_span, uint64_t *out_hist) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_frag: null context");
    copy_out(out_span, c->h_fr_span);
    copy_out(out_hist, c->h_fr_hist);
    return BMV_OK;
}

int bmv_last_frag_stats(bmv_ctx *c, float *ms_kernels, uint32_t *n_informative) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_frag_stats: null context");
    if (ms_kernels) *ms_kernels = c->ms_frag;
    if (n_informative) *n_informative = c->fr_informative;
    return BMV_OK;
}

// Mate rescue (include/bmv.h, bmv_rescue.hip.h): the jobs go to the device, the plan kernel writes their views, the distance
// kernel runs per word count with the call's `parts`, the finish kernel applies the rule; the views and results to the host,
// where bmv_rescued reads them.  Queries beyond the lane kernel's words are aligned in full on their planned views.
int bmv_rescue(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *anchor_text_start, const uint32_t *anchor_text_len,
               const uint8_t *anchor_text_rc, const uint32_t *anchor_query_len, const uint32_t *anchor_end, const uint64_t *contig_start,
               const uint64_t *contig_end, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *max_edits, uint32_t n,
               uint32_t min_frag, uint32_t max_frag) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_rescue: null argument");
    if (!c->loaded) return fail(BMV_ERR_STATE, "bmv_rescue before bmv_load_genome");
    if (n && (!anchor_text_start || !anchor_text_len || !anchor_text_rc || !anchor_query_len || !anchor_end || !contig_start || !contig_end ||
              !query_start || !query_len || !max_edits || (n_read_bytes && !reads)))
        return fail(BMV_ERR_ARG, "bmv_rescue: null argument");
    if (min_frag > max_frag) return fail(BMV_ERR_ARG, "bmv_rescue: min_frag %u is larger than max_frag %u (job 0 and every other)", min_frag, max_frag);
    for (uint32_t j = 0; j < n; j++) {
        if (contig_start[j] > contig_end[j] || contig_end[j] > c->n_genome)
            return fail(BMV_ERR_ARG, "job %u: contig [%llu, %llu) is not a range of the genome's %llu bases", j, (unsigned long long)contig_start[j],
                        (unsigned long long)contig_end[j], (unsigned long long)c->n_genome);
        if (anchor_end[j] > anchor_text_len[j])
            return fail(BMV_ERR_ARG, "job %u: anchor_end %u lies beyond the anchor's view of %u bases", j, anchor_end[j], anchor_text_len[j]);
        if (anchor_text_start[j] >> 62)
            return fail(BMV_ERR_ARG, "job %u: anchor_text_start %llu does not fit the signed coordinates", j, (unsigned long long)anchor_text_start[j]);
        if (anchor_text_start[j] > c->n_genome || anchor_text_len[j] > c->n_genome - anchor_text_start[j])
            return fail(BMV_ERR_ARG, "job %u: the anchor's view lies outside the genome", j);
        if (query_start[j] > n_read_bytes || query_len[j] > n_read_bytes - query_start[j])
            return fail(BMV_ERR_ARG, "job %u: query lies outside the read buffer", j);
        if ((uint64_t)max_frag + std::min(max_edits[j], query_len[j]) > UINT32_MAX)      // (the view holds at most max_frag + k columns)
            return fail(BMV_ERR_ARG, "job %u: a view of max_frag %u plus %u edits does not fit 32 bits", j, max_frag, std::min(max_edits[j], query_len[j]));
    }
    c->h_rs_text_start.assign(n, 0);
    c->h_rs_text_len.assign(n, 0);
    c->h_rs_text_rc.assign(n, 0);
    c->h_rs_edits.assign(n, BMV_BEYOND);
    c->h_rs_end.assign(n, 0);
    c->h_rs_proper.assign(n, 0);
    c->ms_rescue = 0.f;
    c->rs_cells = 0;
    c->rs_parts = 1;
    if (n == 0) return BMV_OK;

    HIP_TRY(hipSetDevice(c->p.device));
    if (c->resident_lanes == 0) {
        int cus = 0, threads = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->p.device));
        HIP_TRY(hipDeviceGetAttribute(&threads, hipDeviceAttributeMaxThreadsPerMultiProcessor, c->p.device));
        c->resident_lanes = (uint32_t)std::max(cus, 1) * (uint32_t)std::max(threads, 64);
    }
    HIP_TRY(c->reads.need_exact((size_t)n_read_bytes + 64u));
    HIP_TRY(need_exact_all(n, c->rs_anchor_start, c->rs_contig_start, c->rs_contig_end, c->rs_query_start, c->rs_text_start));
    HIP_TRY(need_exact_all(n, c->rs_anchor_len, c->rs_anchor_query_len, c->rs_anchor_end, c->rs_query_len, c->rs_max_edits, c->rs_text_len,
                           c->rs_list, c->rs_d, c->rs_end, c->rs_out_edits, c->rs_out_end));
    HIP_TRY(need_exact_all(n, c->rs_anchor_rc, c->rs_text_rc, c->rs_out_proper));
    HIP_TRY(c->rs_count.need_exact(1));
    const size_t n8 = (size_t)n * 8, n4 = (size_t)n * 4;
    if (n_read_bytes) HIP_TRY(hipMemcpyAsync(c->reads.p, reads, (size_t)n_read_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_anchor_start.p, anchor_text_start, n8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_anchor_len.p, anchor_text_len, n4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_anchor_rc.p, anchor_text_rc, n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_anchor_query_len.p, anchor_query_len, n4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_anchor_end.p, anchor_end, n4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_contig_start.p, contig_start, n8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_contig_end.p, contig_end, n8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_query_start.p, query_start, n8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_query_len.p, query_len, n4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_max_edits.p, max_edits, n4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->rs_count.p, 0, sizeof(unsigned long long), c->stream));
    bmv::RescueJob j{};
    j.anchor_text_start = c->rs_anchor_start.p;
    j.anchor_text_len = c->rs_anchor_len.p;
    j.anchor_text_rc = c->rs_anchor_rc.p;
    j.anchor_query_len = c->rs_anchor_query_len.p;
    j.anchor_end = c->rs_anchor_end.p;
    j.contig_start = c->rs_contig_start.p;
    j.contig_end = c->rs_contig_end.p;
    j.max_edits = c->rs_max_edits.p;
    j.n = n;
    j.min_frag = (int64_t)min_frag;
    j.max_frag = (int64_t)max_frag;
    j.genome = c->genome.p;
    j.reads = c->reads.p;
    j.lut = c->lut.p;
    j.text_start = c->rs_text_start.p;
    j.text_len = c->rs_text_len.p;
    j.text_rc = c->rs_text_rc.p;
    j.query_start = c->rs_query_start.p;
    j.query_len = c->rs_query_len.p;
    j.d = c->rs_d.p;
    j.end = c->rs_end.p;
    j.cells = c->rs_count.p;
    j.out_edits = c->rs_out_edits.p;
    j.out_end = c->rs_out_end.p;
    j.out_proper = c->rs_out_proper.p;

    // 1. the views
    const dim3 per_job((n + 255u) / 256u);
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(bmv::bmv_rescue_plan_kernel, per_job, dim3(256), 0, c->stream, j);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_rs_text_start.data(), c->rs_text_start.p, n8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_rs_text_len.data(), c->rs_text_len.p, n4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_rs_text_rc.data(), c->rs_text_rc.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms_plan = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_plan, c->ev0, c->ev1));

    // 2. the jobs by word count; what the lane kernel does not take goes through the aligner (an empty view or query: beyond)
    std::vector<uint32_t> by_words[bmv::kRescueLaneWords + 1], longs;
    uint64_t columns = 0, warm = 0;
    size_t n_listed = 0;
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t m = query_len[a], w = (m + 63u) / 64u;
        if (m == 0u || c->h_rs_text_len[a] == 0u) continue;
        if (w > bmv::kRescueLaneWords) {
            longs.push_back(a);
            continue;
        }
        by_words[w].push_back(a);
        n_listed++;
        columns += c->h_rs_text_len[a];
        warm += (uint64_t)m + std::min(max_edits[a], m);
    }
    std::vector<uint32_t> h_d(n, BMV_BEYOND), h_end(n, 0u);
    float ms_long = 0.f;
    if (!longs.empty()) {
        // bmv_align_long's results are the caller's last alignment call's: kept aside and put back
        const uint32_t keep_n = c->n_last;
        const uint64_t keep_cells = c->n_cells;
        const float keep_ms = c->ms_kernels;
        std::vector<int32_t> keep_score = std::move(c->h_score);
        std::vector<uint32_t> keep_begin = std::move(c->h_begin), keep_cigar = std::move(c->h_cigar);
        std::vector<uint64_t> keep_offset = std::move(c->h_offset);
        const Views v{reads, n_read_bytes, c->h_rs_text_start.data(), c->h_rs_text_len.data(), c->h_rs_text_rc.data(), query_start, query_len, n};
        SubResults sub;
        const int rc = align_sub_batch(c, v, longs, sub);
        c->n_last = keep_n;
        c->n_cells = keep_cells;
        c->ms_kernels = keep_ms;
        c->h_score = std::move(keep_score);
        c->h_begin = std::move(keep_begin);
        c->h_cigar = std::move(keep_cigar);
        c->h_offset = std::move(keep_offset);
        if (rc) return rc;
        for (size_t s = 0; s < longs.size(); s++) {
            uint32_t r = 0;
            for (uint64_t x = sub.offset[s]; x < sub.offset[s + 1]; x++)
                if ((sub.cigar[x] & 15u) != BMV_OP_I) r += sub.cigar[x] >> 4;
            h_d[longs[s]] = (uint32_t)(-(int64_t)sub.score[s]);
            h_end[longs[s]] = sub.begin[s] + r;
            c->rs_cells += (uint64_t)query_len[longs[s]] * c->h_rs_text_len[longs[s]];
        }
        ms_long = sub.ms;
        HIP_TRY(hipSetDevice(c->p.device));
    }

    // 3. parts: as many as fill the card's resident lanes, and no part shorter than its m + k warm-up
    uint32_t parts = 1;
    if (const char *env = getenv("BMV_RESCUE_PARTS")) {
        const long v = atol(env);
        while (parts < 64u && (long)parts * 2 <= v) parts *= 2u;
    } else if (n_listed) {
        while (parts < 64u && (uint64_t)n_listed * parts * 2u <= c->resident_lanes && columns >= warm * parts * 2u) parts *= 2u;
    }
    c->rs_parts = parts;
    uint32_t parts_log2 = 0;
    while ((1u << parts_log2) < parts) parts_log2++;

    // 4. distance and finish
    std::vector<uint32_t> list;
    list.reserve(n_listed);
    for (uint32_t w = 1; w <= bmv::kRescueLaneWords; w++) list.insert(list.end(), by_words[w].begin(), by_words[w].end());
    if (n_listed) HIP_TRY(hipMemcpyAsync(c->rs_list.p, list.data(), n_listed * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_d.p, h_d.data(), n4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->rs_end.p, h_end.data(), n4, hipMemcpyHostToDevice, c->stream));
    using rescue_fn = void (*)(bmv::RescueJob);
    static const rescue_fn per_lane[bmv::kRescueLaneWords + 1] = {nullptr,
                                                                  bmv::bmv_rescue_lane_kernel<1>, bmv::bmv_rescue_lane_kernel<2>,
                                                                  bmv::bmv_rescue_lane_kernel<3>, bmv::bmv_rescue_lane_kernel<4>,
                                                                  bmv::bmv_rescue_lane_kernel<5>, bmv::bmv_rescue_lane_kernel<6>,
                                                                  bmv::bmv_rescue_lane_kernel<7>, bmv::bmv_rescue_lane_kernel<8>};
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    size_t at = 0;
    for (uint32_t w = 1; w <= bmv::kRescueLaneWords; w++) {
        const size_t count = by_words[w].size();
        if (count == 0) continue;
        j.list = c->rs_list.p + at;
        j.count = (uint32_t)count;
        j.parts_log2 = parts_log2;
        const uint64_t waves = ((uint64_t)count * parts + bmv::kWave - 1u) / bmv::kWave;
        hipLaunchKernelGGL(per_lane[w], dim3((uint32_t)waves), dim3(bmv::kWave), 0, c->stream, j);
        HIP_TRY(hipGetLastError());
        at += count;
    }
    hipLaunchKernelGGL(bmv::bmv_rescue_finish_kernel, per_job, dim3(256), 0, c->stream, j);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    unsigned long long steps = 0;
    HIP_TRY(hipMemcpyAsync(c->h_rs_edits.data(), c->rs_out_edits.p, n4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_rs_end.data(), c->rs_out_end.p, n4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_rs_proper.data(), c->rs_out_proper.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&steps, c->rs_count.p, sizeof steps, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms_rest = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_rest, c->ev0, c->ev1));
    c->ms_rescue = ms_plan + ms_long + ms_rest;
    c->rs_cells += 64u * (uint64_t)steps;
    return BMV_OK;
}

int bmv_rescued(bmv_ctx *c, uint64_t *out_text_start, uint32_t *out_text_len, uint8_t *out_text_rc, uint32_t *out_edits, uint32_t *out_end,
                uint8_t *out_proper) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_rescued: null context");
    copy_out(out_text_start, c->h_rs_text_start);
    copy_out(out_text_len, c->h_rs_text_len);
    copy_out(out_text_rc, c->h_rs_text_rc);
    copy_out(out_edits, c->h_rs_edits);
    copy_out(out_end, c->h_rs_end);
    copy_out(out_proper, c->h_rs_proper);
    return BMV_OK;
}

int bmv_last_rescue_stats(bmv_ctx *c, float *ms_kernels, uint64_t *n_cells, uint32_t *parts) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_rescue_stats: null context");
    if (ms_kernels) *ms_kernels = c->ms_rescue;
    if (n_cells) *n_cells = c->rs_cells;
    if (parts) *parts = c->rs_parts;
    return BMV_OK;
}

int bmv_best(bmv_ctx *c, uint32_t *out_winner, uint32_t *out_edits, uint32_t *out_end) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_best: null context");
    if (out_winner && c->n_best_groups) memcpy(out_winner, c->h_bs_winner.data(), (size_t)c->n_best_groups * 4);
    if (out_edits && c->n_best) memcpy(out_edits, c->h_bs_edits.data(), (size_t)c->n_best * 4);
    if (out_end && c->n_best) memcpy(out_end, c->h_bs_end.data(), (size_t)c->n_best * 4);
    return BMV_OK;
}

int bmv_last_best_stats(bmv_ctx *c, uint32_t *n_seed, uint32_t *n_distance, uint32_t *n_beyond, uint32_t *n_undecided,
                        uint32_t *n_realigned, uint64_t *distance_cells, float *ms_distance, float *ms_pick) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_best_stats: null context");
    if (n_seed) *n_seed = c->bs_n_seed;
    if (n_distance) *n_distance = c->bs_n_distance;
    if (n_beyond) *n_beyond = c->bs_n_beyond;
    if (n_undecided) *n_undecided = c->bs_n_undecided;
    if (n_realigned) *n_realigned = c->bs_n_realigned;
    if (distance_cells) *distance_cells = c->bs_cells;
    if (ms_distance) *ms_distance = c->ms_distance;
    if (ms_pick) *ms_pick = c->ms_pick;
    return BMV_OK;
}

// bmv_annotate: upload, the count pass, two exclusive sums, the write pass, download (two_pass_emit).
int bmv_annotate(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                 const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                 const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint64_t *total_xcigar, uint64_t *total_ref_bases) {
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    if (const int rc = check_view_args(c, "bmv_annotate", v, total_xcigar && total_ref_bases, begin && cigar_offset)) return rc;
    uint64_t columns = 0;
    if (const int rc = check_annotate_batch(c, "bmv_annotate", v, begin, cigar_offset, cigar, &columns)) return rc;
    reset_emit(c->h_an, n, columns);
    *total_xcigar = 0;
    *total_ref_bases = 0;
    if (n == 0) return BMV_OK;

    bmv::AnnotateJob j{};
    std::vector<uint64_t> rebased;
    if (const int rc = upload_annotate_batch(c, v, begin, cigar_offset, cigar, rebased, j)) return rc;
    const dim3 grid((n + bmv::kAnnotateWaves - 1u) / bmv::kAnnotateWaves), block(64u * bmv::kAnnotateWaves);
    return two_pass_emit(
        c, "annotate", "count pass", j, c->h_an,
        [&] {
            hipLaunchKernelGGL(bmv::bmv_annotate_kernel<false>, grid, block, 0, c->stream, j);
            return hipGetLastError();
        },
        [&] {
            hipLaunchKernelGGL(bmv::bmv_annotate_kernel<true>, grid, block, 0, c->stream, j);
            return hipGetLastError();
        },
        [] { return hipSuccess; }, total_xcigar, total_ref_bases);
}

int bmv_annotations(bmv_ctx *c, uint32_t *out_nm, uint32_t *out_pos, uint32_t *out_ref_len, uint64_t *out_xcigar_offset,
                    uint32_t *out_xcigar, uint64_t *out_ref_offset, uint8_t *out_ref_bases) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_annotations: null context");
    copy_emit(c->h_an, out_nm, out_pos, out_ref_len, out_xcigar_offset, out_xcigar, out_ref_offset, out_ref_bases);
    return BMV_OK;
}

int bmv_last_annotate_stats(bmv_ctx *c, float *ms_kernels, uint64_t *n_columns) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_annotate_stats: null context");
    if (ms_kernels) *ms_kernels = c->h_an.ms;
    if (n_columns) *n_columns = c->h_an.n_columns;
    return BMV_OK;
}

// The clipping pass (include/bmv.h, bmv_clip.hip.h): bmv_annotate's checks and upload, then the range pass in front of the
// count pass, two exclusive sums, the write pass, download (two_pass_emit) -- into results of its own.
int bmv_clip(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
             const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
             const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint32_t match, uint32_t penalty,
             uint64_t *total_xcigar, uint64_t *total_ref_bases) {
    if (!c || !total_xcigar || !total_ref_bases) return fail(BMV_ERR_ARG, "bmv_clip: null argument");
    if (match < 1u || match > 1024u || penalty < 1u || penalty > 1024u)
        return fail(BMV_ERR_ARG, "bmv_clip: match and penalty must be in 1..1024 (got %u and %u)", match, penalty);
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    if (const int rc = check_view_args(c, "bmv_clip", v, true, begin && cigar_offset)) return rc;
    uint64_t columns = 0;
    if (const int rc = check_annotate_batch(c, "bmv_clip", v, begin, cigar_offset, cigar, &columns)) return rc;
    c->h_cl_score.assign(n, 0);
    c->h_cl_left.assign(n, 0);
    c->h_cl_right.assign(n, 0);
    reset_emit(c->h_cl, n, columns);
    *total_xcigar = 0;
    *total_ref_bases = 0;
    if (n == 0) return BMV_OK;

    bmv::ClipJob j{};
    std::vector<uint64_t> rebased;
    if (const int rc = upload_annotate_batch(c, v, begin, cigar_offset, cigar, rebased, j.a)) return rc;
    HIP_TRY(need_exact_all(n, c->cl_score, c->cl_l, c->cl_r, c->cl_pos0, c->cl_left, c->cl_right));
    j.match = match;
    j.penalty = penalty;
    j.score = c->cl_score.p;
    j.l = c->cl_l.p;
    j.r = c->cl_r.p;
    j.pos0 = c->cl_pos0.p;
    j.clip_left = c->cl_left.p;
    j.clip_right = c->cl_right.p;
    const dim3 grid((n + bmv::kAnnotateWaves - 1u) / bmv::kAnnotateWaves), block(64u * bmv::kAnnotateWaves);
    return two_pass_emit(
        c, "clip", "range and count passes", j.a, c->h_cl,
        [&] {
            hipLaunchKernelGGL(bmv::bmv_clip_range_kernel<bmv::kAnnotateWaves>, grid, block, 0, c->stream, j);
            if (const hipError_t e = hipGetLastError()) return e;
            hipLaunchKernelGGL(bmv::bmv_clip_emit_kernel<false>, grid, block, 0, c->stream, j);
            return hipGetLastError();
        },
        [&] {
            hipLaunchKernelGGL(bmv::bmv_clip_emit_kernel<true>, grid, block, 0, c->stream, j);
            return hipGetLastError();
        },
        [&] {
            if (const hipError_t e = hipMemcpyAsync(c->h_cl_score.data(), c->cl_score.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream)) return e;
            if (const hipError_t e = hipMemcpyAsync(c->h_cl_left.data(), c->cl_left.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)) return e;
            return hipMemcpyAsync(c->h_cl_right.data(), c->cl_right.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
        },
        total_xcigar, total_ref_bases);
}

int bmv_clipped(bmv_ctx *c, int64_t *out_score, uint32_t *out_clip_left, uint32_t *out_clip_right, uint32_t *out_nm,
                uint32_t *out_pos, uint32_t *out_ref_len, uint64_t *out_xcigar_offset, uint32_t *out_xcigar,
                uint64_t *out_ref_offset, uint8_t *out_ref_bases) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_clipped: null context");
    copy_out(out_score, c->h_cl_score);
    copy_out(out_clip_left, c->h_cl_left);
    copy_out(out_clip_right, c->h_cl_right);
    copy_emit(c->h_cl, out_nm, out_pos, out_ref_len, out_xcigar_offset, out_xcigar, out_ref_offset, out_ref_bases);
    return BMV_OK;
}

int bmv_last_clip_stats(bmv_ctx *c, float *ms_kernels, uint64_t *n_columns) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_clip_stats: null context");
    if (ms_kernels) *ms_kernels = c->h_cl.ms;
    if (n_columns) *n_columns = c->h_cl.n_columns;
    return BMV_OK;
}

// The overlap pass (include/bmv.h, bmv_overlap.hip.h): bmv_clip's checks and upload; the base range (bmv_clip's range kernel, or
// all columns), the span, decide, restrict and commit passes in front of bmv_clip's count pass, the score pass behind it, two
// exclusive sums, bmv_clip's write pass, download (two_pass_emit) -- into results of its own.
int bmv_overlap(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                const uint64_t *cigar_offset, const uint32_t *cigar, const uint32_t *mate, const uint32_t *contig, uint32_t n,
                uint32_t match, uint32_t penalty, uint64_t *total_xcigar, uint64_t *total_ref_bases) {
    if (!c || !total_xcigar || !total_ref_bases || (n && !mate)) return fail(BMV_ERR_ARG, "bmv_overlap: null argument");
    const bool scored = match != 0u || penalty != 0u;
    if (scored && (match < 1u || match > 1024u || penalty < 1u || penalty > 1024u))
        return fail(BMV_ERR_ARG, "bmv_overlap: match and penalty must be 0 and 0 or in 1..1024 (got %u and %u)", match, penalty);
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    if (const int rc = check_view_args(c, "bmv_overlap", v, true, begin && cigar_offset)) return rc;
    uint64_t columns = 0;
    if (const int rc = check_annotate_batch(c, "bmv_overlap", v, begin, cigar_offset, cigar, &columns)) return rc;
    for (uint32_t a = 0; a < n; a++) {
        if (text_start[a] >= (1ull << 62))
            return fail(BMV_ERR_ARG, "alignment %u: text_start %llu is not below 2^62", a, (unsigned long long)text_start[a]);
        if (mate[a] == BMV_NO_MATE) continue;
        if (mate[a] >= n) return fail(BMV_ERR_ARG, "alignment %u: mate %u, the batch has %u alignments", a, mate[a], n);
        if (mate[a] == a) return fail(BMV_ERR_ARG, "alignment %u: it is its own mate", a);
        if (mate[mate[a]] != a)
            return fail(BMV_ERR_ARG, "alignment %u: its mate %u names %u as its mate", a, mate[a], mate[mate[a]]);
    }
    c->h_ov_score.assign(n, 0);
    c->h_ov_left.assign(n, 0);
    c->h_ov_right.assign(n, 0);
    c->h_ov_cut.assign(n, 0);
    c->h_ov_was_cut.assign(n, 0);
    c->ov_pairs_cut = c->ov_bases_cut = 0;
    reset_emit(c->h_ov, n, columns);
    *total_xcigar = 0;
    *total_ref_bases = 0;
    if (n == 0) return BMV_OK;

    bmv::OverlapJob j{};
    std::vector<uint64_t> rebased;
    if (const int rc = upload_annotate_batch(c, v, begin, cigar_offset, cigar, rebased, j.c.a)) return rc;
    HIP_TRY(need_exact_all(n, c->cl_score, c->cl_l, c->cl_r, c->cl_pos0, c->cl_left, c->cl_right));
    HIP_TRY(need_exact_all(n, c->ov_mate, c->ov_role, c->ov_found, c->ov_cut_q, c->ov_cut, c->ov_l0, c->ov_r0, c->ov_edge, c->ov_g0,
                           c->ov_g1, c->ov_m, c->ov_was_cut));
    HIP_TRY(hipMemcpyAsync(c->ov_mate.p, mate, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (contig) {
        HIP_TRY(c->ov_contig.need_exact(n));
        HIP_TRY(hipMemcpyAsync(c->ov_contig.p, contig, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
    j.c.match = match;
    j.c.penalty = penalty;
    j.c.score = c->cl_score.p;
    j.c.l = c->cl_l.p;
    j.c.r = c->cl_r.p;
    j.c.pos0 = c->cl_pos0.p;
    j.c.clip_left = c->cl_left.p;
    j.c.clip_right = c->cl_right.p;
    j.mate = c->ov_mate.p;
    j.contig = contig ? c->ov_contig.p : nullptr;
    j.l0 = c->ov_l0.p;
    j.r0 = c->ov_r0.p;
    j.g0 = c->ov_g0.p;
    j.g1 = c->ov_g1.p;
    j.m = c->ov_m.p;
    j.role = c->ov_role.p;
    j.edge = c->ov_edge.p;
    j.found = c->ov_found.p;
    j.cut_q = c->ov_cut_q.p;
    j.cut = c->ov_cut.p;
    j.was_cut = c->ov_was_cut.p;
    const dim3 grid((n + bmv::kAnnotateWaves - 1u) / bmv::kAnnotateWaves), block(64u * bmv::kAnnotateWaves);
    const dim3 tgrid((n + bmv::kOverlapThreads - 1u) / bmv::kOverlapThreads), tblock(bmv::kOverlapThreads);
    const int rc = two_pass_emit(
        c, "overlap", "range, span, decide, restrict, commit, count and score passes", j.c.a, c->h_ov,
        [&] {
            if (scored) {
                bmv::ClipJob base = j.c;                            // bmv_clip's range kernel writes the BASE range
                base.l = j.l0;
                base.r = j.r0;
                hipLaunchKernelGGL(bmv::bmv_clip_range_kernel<bmv::kAnnotateWaves>, grid, block, 0, c->stream, base);
                if (const hipError_t e = hipGetLastError()) return e;
                hipLaunchKernelGGL(bmv::bmv_overlap_span_kernel<true>, grid, block, 0, c->stream, j);
            } else {
                hipLaunchKernelGGL(bmv::bmv_overlap_span_kernel<false>, grid, block, 0, c->stream, j);
            }
            if (const hipError_t e = hipGetLastError()) return e;
            hipLaunchKernelGGL(bmv::bmv_overlap_decide_kernel<bmv::kOverlapThreads>, tgrid, tblock, 0, c->stream, j);
            if (const hipError_t e = hipGetLastError()) return e;
            hipLaunchKernelGGL(bmv::bmv_overlap_restrict_kernel<bmv::kAnnotateWaves>, grid, block, 0, c->stream, j);
            if (const hipError_t e = hipGetLastError()) return e;
            hipLaunchKernelGGL(bmv::bmv_overlap_commit_kernel<bmv::kOverlapThreads>, tgrid, tblock, 0, c->stream, j);
            if (const hipError_t e = hipGetLastError()) return e;
            hipLaunchKernelGGL(bmv::bmv_clip_emit_kernel<false>, grid, block, 0, c->stream, j.c);
            if (const hipError_t e = hipGetLastError()) return e;
            hipLaunchKernelGGL(bmv::bmv_overlap_score_kernel<bmv::kOverlapThreads>, tgrid, tblock, 0, c->stream, j);
            return hipGetLastError();
        },
        [&] {
            hipLaunchKernelGGL(bmv::bmv_clip_emit_kernel<true>, grid, block, 0, c->stream, j.c);
            return hipGetLastError();
        },
        [&] {
            if (const hipError_t e = hipMemcpyAsync(c->h_ov_score.data(), c->cl_score.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream)) return e;
            if (const hipError_t e = hipMemcpyAsync(c->h_ov_left.data(), c->cl_left.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)) return e;
            if (const hipError_t e = hipMemcpyAsync(c->h_ov_right.data(), c->cl_right.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)) return e;
            if (const hipError_t e = hipMemcpyAsync(c->h_ov_cut.data(), c->ov_cut.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream)) return e;
            return hipMemcpyAsync(c->h_ov_was_cut.data(), c->ov_was_cut.p, (size_t)n, hipMemcpyDeviceToHost, c->stream);
        },
        total_xcigar, total_ref_bases);
    if (rc) return rc;
    uint64_t mates_cut = 0;
    for (uint32_t a = 0; a < n; a++) {
        mates_cut += c->h_ov_was_cut[a] != 0;
        c->ov_bases_cut += c->h_ov_cut[a];
    }
    c->ov_pairs_cut = mates_cut / 2u;
    return BMV_OK;
}

int bmv_overlapped(bmv_ctx *c, int64_t *out_score, uint32_t *out_clip_left, uint32_t *out_clip_right, uint32_t *out_nm,
                   uint32_t *out_pos, uint32_t *out_ref_len, uint64_t *out_xcigar_offset, uint32_t *out_xcigar,
                   uint64_t *out_ref_offset, uint8_t *out_ref_bases, uint32_t *out_cut) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_overlapped: null context");
    copy_out(out_score, c->h_ov_score);
    copy_out(out_clip_left, c->h_ov_left);
    copy_out(out_clip_right, c->h_ov_right);
    copy_out(out_cut, c->h_ov_cut);
    copy_emit(c->h_ov, out_nm, out_pos, out_ref_len, out_xcigar_offset, out_xcigar, out_ref_offset, out_ref_bases);
    return BMV_OK;
}

int bmv_last_overlap_stats(bmv_ctx *c, float *ms_kernels, uint64_t *n_columns, uint64_t *pairs_cut, uint64_t *bases_cut) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_overlap_stats: null context");
    if (ms_kernels) *ms_kernels = c->h_ov.ms;
    if (n_columns) *n_columns = c->h_ov.n_columns;
    if (pairs_cut) *pairs_cut = c->ov_pairs_cut;
    if (bases_cut) *bases_cut = c->ov_bases_cut;
    return BMV_OK;
}

// Split alignments (include/bmv.h, bmv_split.hip.h): bmv_clip's checks and bmv_annotate's upload, then the range kernel and
// the pick kernel back to back on the stream -- the ranges never visit the host on their way to the pick.
int bmv_split(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
              const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
              const uint64_t *cigar_offset, const uint32_t *cigar, const uint32_t *contig, uint32_t n, const uint32_t *group_offset,
              uint32_t n_groups, uint32_t match, uint32_t penalty, uint32_t min_score, uint32_t max_overlap_permille,
              uint32_t max_segments) {
    if (!c || !group_offset) return fail(BMV_ERR_ARG, "bmv_split: null argument");
    if (match < 1u || match > 1024u || penalty < 1u || penalty > 1024u)
        return fail(BMV_ERR_ARG, "bmv_split: match and penalty must be in 1..1024 (got %u and %u)", match, penalty);
    const SplitArgs s{contig, n, group_offset, n_groups, min_score, max_overlap_permille, max_segments};
    if (const int rc = check_split_args("bmv_split", s)) return rc;
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    if (const int rc = check_view_args(c, "bmv_split", v, true, begin && cigar_offset)) return rc;
    if (const int rc = check_groups("bmv_split", group_offset, n_groups, n, nullptr)) return rc;
    uint64_t columns = 0;
    if (const int rc = check_annotate_batch(c, "bmv_split", v, begin, cigar_offset, cigar, &columns)) return rc;
    for (uint32_t a = 0; a < n; a++)
        if (text_start[a] >> 62)
            return fail(BMV_ERR_ARG, "alignment %u: text_start %llu does not fit the signed coordinates", a, (unsigned long long)text_start[a]);
    reset_split(c, s, columns);
    if (n_groups == 0) return BMV_OK;                           // (then n = 0 too: check_groups)

    bmv::SplitRangeJob j{};
    std::vector<uint64_t> rebased;
    HIP_TRY(hipSetDevice(c->p.device));
    if (n) {
        if (const int rc = upload_annotate_batch(c, v, begin, cigar_offset, cigar, rebased, j.a)) return rc;
        HIP_TRY(need_exact_all(n, c->sp_score, c->sp_g_lo, c->sp_g_hi, c->sp_q_lo, c->sp_q_hi));
    }
    j.match = match;
    j.penalty = penalty;
    j.score = c->sp_score.p;
    j.q_lo = c->sp_q_lo.p;
    j.q_hi = c->sp_q_hi.p;
    j.g_lo = c->sp_g_lo.p;
    j.g_hi = c->sp_g_hi.p;
    if (const int rc = run_split_pick(c, s, n != 0u, [&] {
            if (n == 0u) return hipSuccess;
            hipLaunchKernelGGL(bmv::bmv_split_range_kernel<bmv::kSplitWaves>, dim3((n + bmv::kSplitWaves - 1u) / bmv::kSplitWaves),
                               dim3(64u * bmv::kSplitWaves), 0, c->stream, j);
            return hipGetLastError();
        }))
        return rc;
    if (n) {
        HIP_TRY(hipMemcpyAsync(c->h_sp_score.data(), c->sp_score.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_sp_q_lo.data(), c->sp_q_lo.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_sp_q_hi.data(), c->sp_q_hi.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_sp_g_lo.data(), c->sp_g_lo.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_sp_g_hi.data(), c->sp_g_hi.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (getenv("BMV_LOG_CLASSES"))
        fprintf(stderr, "[bmv] split: %u alignments in %u groups, range pass %.3f ms, pick %.3f ms\n", n, n_groups, c->ms_sp_range, c->ms_sp_pick);
    return BMV_OK;
}

// The pick alone (include/bmv.h): the five arrays go to the device as given, the pick kernel runs, bmv_segments reads.
int bmv_split_pick(bmv_ctx *c, const int64_t *score, const uint32_t *q_lo, const uint32_t *q_hi, const int64_t *g_lo, const int64_t *g_hi,
                   const uint8_t *text_rc, const uint32_t *contig, uint32_t n, const uint32_t *group_offset, uint32_t n_groups,
                   uint32_t min_score, uint32_t max_overlap_permille, uint32_t max_segments) {
    if (!c || !group_offset || (n && (!score || !q_lo || !q_hi || !g_lo || !g_hi || !text_rc)))
        return fail(BMV_ERR_ARG, "bmv_split_pick: null argument");
    const SplitArgs s{contig, n, group_offset, n_groups, min_score, max_overlap_permille, max_segments};
    if (const int rc = check_split_args("bmv_split_pick", s)) return rc;
    if (const int rc = check_groups("bmv_split_pick", group_offset, n_groups, n, nullptr)) return rc;
    for (uint32_t a = 0; a < n; a++) {
        if (q_lo[a] > q_hi[a]) return fail(BMV_ERR_ARG, "alignment %u: q_lo %u lies behind q_hi %u", a, q_lo[a], q_hi[a]);
        if (g_lo[a] > g_hi[a])
            return fail(BMV_ERR_ARG, "alignment %u: g_lo %lld lies behind g_hi %lld", a, (long long)g_lo[a], (long long)g_hi[a]);
    }
    reset_split(c, s, 0);
    c->h_sp_score.assign(score, score + n);
    c->h_sp_q_lo.assign(q_lo, q_lo + n);
    c->h_sp_q_hi.assign(q_hi, q_hi + n);
    c->h_sp_g_lo.assign(g_lo, g_lo + n);
    c->h_sp_g_hi.assign(g_hi, g_hi + n);
    if (n_groups == 0) return BMV_OK;
    HIP_TRY(hipSetDevice(c->p.device));
    if (n) {
        HIP_TRY(need_exact_all(n, c->sp_score, c->sp_g_lo, c->sp_g_hi, c->sp_q_lo, c->sp_q_hi, c->text_rc));
        HIP_TRY(hipMemcpyAsync(c->sp_score.p, score, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->sp_q_lo.p, q_lo, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->sp_q_hi.p, q_hi, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->sp_g_lo.p, g_lo, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->sp_g_hi.p, g_hi, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->text_rc.p, text_rc, (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    return run_split_pick(c, s, false, [] { return hipSuccess; });
}

int bmv_segments(bmv_ctx *c, int64_t *out_score, uint32_t *out_q_lo, uint32_t *out_q_hi, int64_t *out_g_lo, int64_t *out_g_hi,
                 uint32_t *out_n_seg, uint32_t *out_seg, int64_t *out_s2) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_segments: null context");
    copy_out(out_score, c->h_sp_score);
    copy_out(out_q_lo, c->h_sp_q_lo);
    copy_out(out_q_hi, c->h_sp_q_hi);
    copy_out(out_g_lo, c->h_sp_g_lo);
    copy_out(out_g_hi, c->h_sp_g_hi);
    copy_out(out_n_seg, c->h_sp_n_seg);
    copy_out(out_seg, c->h_sp_seg);
    copy_out(out_s2, c->h_sp_s2);
    return BMV_OK;
}

int bmv_last_split_stats(bmv_ctx *c, float *ms_range, float *ms_pick, uint64_t *n_columns, uint64_t *n_segments) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_split_stats: null context");
    if (ms_range) *ms_range = c->ms_sp_range;
    if (ms_pick) *ms_pick = c->ms_sp_pick;
    if (n_columns) *n_columns = c->sp_columns;
    if (n_segments) *n_segments = c->sp_segments;
    return BMV_OK;
}

// The realignment pass (include/bmv.h, bmv_realign.hip.h): bmv_annotate's checks and upload; the plan -- which alignments
// are passed through, the score bound, every realigned alignment's place in the scratch -- is made on the host from the
// entries it has just validated; the batch is taken in pieces whose direction codes and reversed entries fit the scratch:
// forward kernel, traceback, a 64-bit exclusive sum of the entry counts, the gather, the piece's entries to the host.
int bmv_realign(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint32_t match, uint32_t mismatch, uint32_t gap_open,
                uint32_t gap_extend, uint32_t band, uint64_t *total_cigar) {
    if (!c || !total_cigar) return fail(BMV_ERR_ARG, "bmv_realign: null argument");
    for (const uint32_t s : {match, mismatch, gap_open, gap_extend})
        if (s < 1u || s > 1024u)
            return fail(BMV_ERR_ARG, "bmv_realign: match, mismatch, gap_open and gap_extend must be in 1..1024 (got %u, %u, %u and %u)", match,
                        mismatch, gap_open, gap_extend);
    if (band < 1u || band > 31u) return fail(BMV_ERR_ARG, "bmv_realign: band must be in 1..31 (got %u)", band);
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    if (const int rc = check_view_args(c, "bmv_realign", v, true, begin && cigar_offset)) return rc;
    uint64_t columns = 0;
    if (const int rc = check_annotate_batch(c, "bmv_realign", v, begin, cigar_offset, cigar, &columns)) return rc;
    // the plan: pass-through, the 32-bit bound, the scratch of every realigned alignment
    const uint64_t widest = std::max(match, std::max(mismatch, gap_extend)), in_m = std::max(match, mismatch), cap = 63u - 2u * band;
    const uint64_t budget = c->scratch_bytes;
    std::vector<uint8_t> pass(n, 0);
    std::vector<uint64_t> need(n, 0);                           // bytes of scratch
    uint64_t cells = 0;
    uint32_t n_passed = 0;
    for (uint32_t a = 0; a < n; a++) {
        const uint64_t c0 = cigar_offset[a], c1 = cigar_offset[a + 1];
        if (c0 == c1) {
            pass[a] = 1;
            n_passed++;
            continue;
        }
        const uint64_t m = query_len[a];
        uint64_t path = 0;                                      // what the given path can cost at most
        for (uint64_t x = c0; x < c1; x++) {
            const uint64_t len = cigar[x] >> 4;
            if ((cigar[x] & 15u) == BMV_OP_M) {
                path += len * in_m;
            } else {
                path += gap_open + len * gap_extend;
                if ((cigar[x] & 15u) == BMV_OP_D && len > cap) pass[a] = 1;
            }
        }
        const uint64_t both = m + text_len[a];
        if (both * widest + gap_open >= (1ull << 30) || path + gap_open + both * gap_extend >= (1ull << 30))
            return fail(BMV_ERR_UNSUPPORTED, "alignment %u: a query of %u bases against %u text bases (%llu CIGAR entries) under these scores does not fit 32-bit arithmetic",
                        a, query_len[a], text_len[a], (unsigned long long)(c1 - c0));
        if (pass[a]) {
            n_passed++;
            continue;
        }
        need[a] = m * 64u + (2u * m + 2u) * 4u;
        cells += 64u * m;
        if (need[a] > budget)
            return fail(BMV_ERR_UNSUPPORTED, "alignment %u: a query of %u bases needs %llu bytes of direction codes; the scratch holds %llu (BMV_SCRATCH_MB)",
                        a, query_len[a], (unsigned long long)need[a], (unsigned long long)budget);
    }
    c->h_ra_score.assign(n, 0);
    c->h_ra_begin.assign(n, 0);
    c->h_ra_realigned.assign(n, 0);
    c->h_ra_offset.assign((size_t)n + 1, 0);
    c->h_ra_cigar.clear();
    c->ms_realign = 0.f;
    c->ra_cells = cells;
    c->ra_passed = n_passed;
    *total_cigar = 0;
    if (n == 0) return BMV_OK;

    // pieces that fit the scratch; a realigned alignment's rows and reversed entries counted from its piece's first
    std::vector<uint32_t> piece_at{0};
    std::vector<uint64_t> row_at(n, 0), ops_at(n, 0);
    uint64_t max_rows = 0, max_ops = 0;
    {
        uint64_t bytes = 0, rows = 0, ops = 0;
        for (uint32_t a = 0; a < n; a++) {
            if (bytes + need[a] > budget) {
                piece_at.push_back(a);
                bytes = rows = ops = 0;
            }
            row_at[a] = rows;
            ops_at[a] = ops;
            if (!pass[a]) {
                rows += query_len[a];
                ops += 2u * (uint64_t)query_len[a] + 2u;
            }
            bytes += need[a];
            max_rows = std::max(max_rows, rows);
            max_ops = std::max(max_ops, ops);
        }
        piece_at.push_back(n);
    }
    bmv::AnnotateJob in{};
    std::vector<uint64_t> rebased;
    if (const int rc = upload_annotate_batch(c, v, begin, cigar_offset, cigar, rebased, in)) return rc;
    HIP_TRY(need_exact_all(n, c->ra_pass, c->ra_row_at, c->ra_ops_at, c->ra_score, c->ra_begin, c->ra_end_lane, c->ra_nops));
    HIP_TRY(c->ra_offset.need_exact((size_t)n + 1u));
    HIP_TRY(c->ra_codes.need_exact(with_headroom((size_t)max_rows * 64u, c->ra_codes.cap)));
    HIP_TRY(c->ra_ops_rev.need_exact(with_headroom((size_t)max_ops, c->ra_ops_rev.cap)));
    HIP_TRY(hipMemcpyAsync(c->ra_pass.p, pass.data(), n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ra_row_at.p, row_at.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ra_ops_at.p, ops_at.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    bmv::RealignJob j{};
    j.genome = in.genome;
    j.reads = in.reads;
    j.text_start = in.text_start;
    j.text_len = in.text_len;
    j.text_rc = in.text_rc;
    j.query_start = in.query_start;
    j.query_len = in.query_len;
    j.begin = in.begin;
    j.cigar_offset = in.cigar_offset;
    j.cigar = in.cigar;
    j.pass = c->ra_pass.p;
    j.row_at = c->ra_row_at.p;
    j.ops_at = c->ra_ops_at.p;
    j.match = (int32_t)match;
    j.mismatch = (int32_t)mismatch;
    j.open = (int32_t)gap_open;
    j.ext = (int32_t)gap_extend;
    j.band = band;
    j.codes = c->ra_codes.p;
    j.ops_rev = c->ra_ops_rev.p;
    j.score = c->ra_score.p;
    j.out_begin = c->ra_begin.p;
    j.end_lane = c->ra_end_lane.p;
    j.nops = c->ra_nops.p;
    j.out_offset = c->ra_offset.p;
    uint64_t *scan_tmp = reinterpret_cast<uint64_t *>(c->scan_tmp.p);
    float ms_forward = 0.f, ms_trace = 0.f, ms_gather = 0.f;
    std::vector<uint64_t> off;
    for (size_t p = 0; p + 1 < piece_at.size(); p++) {
        const uint32_t a0 = piece_at[p], cnt = piece_at[p + 1] - a0;
        if (cnt == 0) continue;
        j.first = a0;
        j.count = cnt;
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
        hipLaunchKernelGGL(bmv::bmv_realign_forward_kernel, dim3(cnt), dim3(64), 0, c->stream, j);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_forward += ms;
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
        hipLaunchKernelGGL(bmv::bmv_realign_trace_kernel, dim3(cnt), dim3(64), 0, c->stream, j);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        HIP_TRY(bmscan::exclusive_sum<uint64_t>(c->ra_nops.p + a0, c->ra_offset.p, cnt, scan_tmp, c->stream));
        off.resize((size_t)cnt + 1);
        HIP_TRY(hipMemcpyAsync(off.data(), c->ra_offset.p, ((size_t)cnt + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_trace += ms;
        const uint64_t n_entries = off[cnt], had = c->h_ra_cigar.size();
        HIP_TRY(c->ra_cigar.need_exact(with_headroom((size_t)n_entries, c->ra_cigar.cap)));
        j.out_cigar = c->ra_cigar.p;
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
        hipLaunchKernelGGL(bmv::bmv_realign_gather_kernel, dim3((cnt + 31u) / 32u), dim3(256), 0, c->stream, j);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        c->h_ra_cigar.resize((size_t)(had + n_entries));
        if (n_entries)
            HIP_TRY(hipMemcpyAsync(c->h_ra_cigar.data() + had, c->ra_cigar.p, (size_t)n_entries * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_gather += ms;
        for (uint32_t s = 0; s <= cnt; s++) c->h_ra_offset[(size_t)a0 + s] = had + off[s];
    }
    HIP_TRY(hipMemcpyAsync(c->h_ra_score.data(), c->ra_score.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_ra_begin.data(), c->ra_begin.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t a = 0; a < n; a++) c->h_ra_realigned[a] = pass[a] ? 0 : 1;
    c->ms_realign = ms_forward + ms_trace + ms_gather;
    if (getenv("BMV_LOG_CLASSES"))
        fprintf(stderr, "[bmv] realign: %u alignments (%u passed through) in %zu pieces, forward %.3f ms, traceback %.3f ms, scan and gather %.3f ms\n",
                n, n_passed, piece_at.size() - 1, ms_forward, ms_trace, ms_gather);
    *total_cigar = c->h_ra_cigar.size();
    return BMV_OK;
}

int bmv_realigned(bmv_ctx *c, int32_t *out_score, uint32_t *out_begin, uint8_t *out_realigned, uint64_t *out_cigar_offset,
                  uint32_t *out_cigar) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_realigned: null context");
    copy_out(out_score, c->h_ra_score);
    copy_out(out_begin, c->h_ra_begin);
    copy_out(out_realigned, c->h_ra_realigned);
    copy_out(out_cigar_offset, c->h_ra_offset);
    copy_out(out_cigar, c->h_ra_cigar);
    return BMV_OK;
}

int bmv_last_realign_stats(bmv_ctx *c, float *ms_kernels, uint64_t *n_cells, uint32_t *n_passed_through) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_realign_stats: null context");
    if (ms_kernels) *ms_kernels = c->ms_realign;
    if (n_cells) *n_cells = c->ra_cells;
    if (n_passed_through) *n_passed_through = c->ra_passed;
    return BMV_OK;
}

// The normalisation pass (include/bmv.h, bmv_leftalign.hip.h): bmv_annotate's checks and upload; every alignment gets a stack
// slot of E + (gap entries) words in the scratch, the batch is taken in pieces whose slots fit it: the walk, a 64-bit
// exclusive sum of the entry counts, the gather, the piece's entries to the host.
int bmv_leftalign(bmv_ctx *c, const uint8_t *reads, uint64_t n_read_bytes, const uint64_t *text_start, const uint32_t *text_len,
                  const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                  const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, uint64_t *total_cigar) {
    const Views v{reads, n_read_bytes, text_start, text_len, text_rc, query_start, query_len, n};
    if (const int rc = check_view_args(c, "bmv_leftalign", v, total_cigar != nullptr, begin && cigar_offset)) return rc;
    uint64_t columns = 0;
    if (const int rc = check_annotate_batch(c, "bmv_leftalign", v, begin, cigar_offset, cigar, &columns)) return rc;
    // merged entries must fit 28 bits; the slot of every alignment
    const uint64_t budget = c->scratch_bytes;
    std::vector<uint64_t> need(n, 0);                           // words of scratch
    for (uint32_t a = 0; a < n; a++) {
        uint64_t by_op[3] = {0, 0, 0}, gaps = 0;
        for (uint64_t x = cigar_offset[a]; x < cigar_offset[a + 1]; x++) {
            by_op[cigar[x] & 15u] += cigar[x] >> 4;
            if ((cigar[x] & 15u) != BMV_OP_M) gaps++;
        }
        for (uint32_t op = 0; op < 3u; op++)
            if (by_op[op] >= (1ull << 28))
                return fail(BMV_ERR_UNSUPPORTED, "alignment %u: its %c entries sum to %llu columns; a merged entry holds fewer than 2^28", a,
                            "MID"[op], (unsigned long long)by_op[op]);
        need[a] = cigar_offset[a + 1] - cigar_offset[a] + gaps;
        if (need[a] * 4u > budget)
            return fail(BMV_ERR_UNSUPPORTED, "alignment %u: %llu CIGAR entries need a stack of %llu bytes; the scratch holds %llu (BMV_SCRATCH_MB)", a,
                        (unsigned long long)(cigar_offset[a + 1] - cigar_offset[a]), (unsigned long long)(need[a] * 4u),
                        (unsigned long long)budget);
    }
    c->h_la_begin.assign(n, 0);
    c->h_la_dropped.assign(n, 0);
    c->h_la_changed.assign(n, 0);
    c->h_la_offset.assign((size_t)n + 1, 0);
    c->h_la_cigar.clear();
    c->ms_leftalign = 0.f;
    c->la_n_compared = c->la_n_merges = c->la_n_dropped = 0;
    c->la_n_changed = 0;
    *total_cigar = 0;
    if (n == 0) return BMV_OK;

    std::vector<uint32_t> piece_at{0};
    std::vector<uint64_t> slot_at(n, 0);
    uint64_t max_words = 0;
    {
        uint64_t words = 0;
        for (uint32_t a = 0; a < n; a++) {
            if ((words + need[a]) * 4u > budget) {
                piece_at.push_back(a);
                words = 0;
            }
            slot_at[a] = words;
            words += need[a];
            max_words = std::max(max_words, words);
        }
        piece_at.push_back(n);
    }
    bmv::AnnotateJob in{};
    std::vector<uint64_t> rebased;
    if (const int rc = upload_annotate_batch(c, v, begin, cigar_offset, cigar, rebased, in)) return rc;
    HIP_TRY(need_exact_all(n, c->la_slot_at, c->la_compared, c->la_begin, c->la_nops, c->la_dropped, c->la_merges, c->la_changed));
    HIP_TRY(c->la_offset.need_exact((size_t)n + 1u));
    HIP_TRY(c->la_stack.need_exact(with_headroom((size_t)std::max<uint64_t>(max_words, 1u), c->la_stack.cap)));
    HIP_TRY(hipMemcpyAsync(c->la_slot_at.p, slot_at.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    bmv::LeftAlignJob j{};
    j.genome = in.genome;
    j.reads = in.reads;
    j.text_start = in.text_start;
    j.text_len = in.text_len;
    j.text_rc = in.text_rc;
    j.query_start = in.query_start;
    j.query_len = in.query_len;
    j.begin = in.begin;
    j.cigar_offset = in.cigar_offset;
    j.cigar = in.cigar;
    j.slot_at = c->la_slot_at.p;
    j.stack = c->la_stack.p;
    j.out_begin = c->la_begin.p;
    j.nops = c->la_nops.p;
    j.dropped = c->la_dropped.p;
    j.merges = c->la_merges.p;
    j.compared = c->la_compared.p;
    j.changed = c->la_changed.p;
    j.out_offset = c->la_offset.p;
    uint64_t *scan_tmp = reinterpret_cast<uint64_t *>(c->scan_tmp.p);
    float ms_walk = 0.f, ms_gather = 0.f;
    std::vector<uint64_t> off;
    for (size_t p = 0; p + 1 < piece_at.size(); p++) {
        const uint32_t a0 = piece_at[p], cnt = piece_at[p + 1] - a0;
        if (cnt == 0) continue;
        j.first = a0;
        j.count = cnt;
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
        hipLaunchKernelGGL(bmv::bmv_leftalign_kernel, dim3((cnt + bmv::kLeftAlignWaves - 1u) / bmv::kLeftAlignWaves),
                           dim3(64u * bmv::kLeftAlignWaves), 0, c->stream, j);
        HIP_TRY(hipGetLastError());
        HIP_TRY(bmscan::exclusive_sum<uint64_t>(c->la_nops.p + a0, c->la_offset.p, cnt, scan_tmp, c->stream));
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        off.resize((size_t)cnt + 1);
        HIP_TRY(hipMemcpyAsync(off.data(), c->la_offset.p, ((size_t)cnt + 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_walk += ms;
        const uint64_t n_entries = off[cnt], had = c->h_la_cigar.size();
        HIP_TRY(c->la_cigar.need_exact(with_headroom((size_t)std::max<uint64_t>(n_entries, 1u), c->la_cigar.cap)));
        j.out_cigar = c->la_cigar.p;
        HIP_TRY(hipEventRecord(c->ev0, c->stream));
        hipLaunchKernelGGL(bmv::bmv_leftalign_gather_kernel, dim3((cnt + 31u) / 32u), dim3(256), 0, c->stream, j);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev1, c->stream));
        c->h_la_cigar.resize((size_t)(had + n_entries));
        if (n_entries)
            HIP_TRY(hipMemcpyAsync(c->h_la_cigar.data() + had, c->la_cigar.p, (size_t)n_entries * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        ms_gather += ms;
        for (uint32_t s = 0; s <= cnt; s++) c->h_la_offset[(size_t)a0 + s] = had + off[s];
    }
    std::vector<uint64_t> compared(n);
    std::vector<uint32_t> merges(n);
    HIP_TRY(hipMemcpyAsync(c->h_la_begin.data(), c->la_begin.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_la_dropped.data(), c->la_dropped.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_la_changed.data(), c->la_changed.p, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(compared.data(), c->la_compared.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(merges.data(), c->la_merges.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t a = 0; a < n; a++) {
        c->la_n_compared += compared[a];
        c->la_n_merges += merges[a];
        c->la_n_dropped += c->h_la_dropped[a];
        c->la_n_changed += c->h_la_changed[a] ? 1u : 0u;
    }
    c->ms_leftalign = ms_walk + ms_gather;
    if (getenv("BMV_LOG_CLASSES"))
        fprintf(stderr, "[bmv] leftalign: %u alignments (%u changed) in %zu pieces, walk and scan %.3f ms, gather %.3f ms\n", n,
                c->la_n_changed, piece_at.size() - 1, ms_walk, ms_gather);
    *total_cigar = c->h_la_cigar.size();
    return BMV_OK;
}

int bmv_leftaligned(bmv_ctx *c, uint32_t *out_begin, uint64_t *out_cigar_offset, uint32_t *out_cigar, uint8_t *out_changed,
                    uint32_t *out_dropped) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_leftaligned: null context");
    copy_out(out_begin, c->h_la_begin);
    copy_out(out_cigar_offset, c->h_la_offset);
    copy_out(out_cigar, c->h_la_cigar);
    copy_out(out_changed, c->h_la_changed);
    copy_out(out_dropped, c->h_la_dropped);
    return BMV_OK;
}

int bmv_last_leftalign_stats(bmv_ctx *c, float *ms_kernels, uint64_t *n_compared, uint32_t *n_changed, uint64_t *n_merges,
                             uint64_t *n_dropped) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_leftalign_stats: null context");
    if (ms_kernels) *ms_kernels = c->ms_leftalign;
    if (n_compared) *n_compared = c->la_n_compared;
    if (n_changed) *n_changed = c->la_n_changed;
    if (n_merges) *n_merges = c->la_n_merges;
    if (n_dropped) *n_dropped = c->la_n_dropped;
    return BMV_OK;
}

int bmv_results(bmv_ctx *c, int32_t *out_score, uint32_t *out_begin, uint64_t *out_cigar_offset, uint32_t *out_cigar) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_results: null context");
    copy_out(out_score, c->h_score);
    copy_out(out_begin, c->h_begin);
    copy_out(out_cigar_offset, c->h_offset);
    copy_out(out_cigar, c->h_cigar);
    return BMV_OK;
}

int bmv_last_stats(bmv_ctx *c, float *ms_kernels, uint64_t *n_cells) {
    if (!c) return fail(BMV_ERR_ARG, "bmv_last_stats: null context");
    if (ms_kernels) *ms_kernels = c->ms_kernels;
    if (n_cells) *n_cells = c->n_cells;
    return BMV_OK;
}

}  // extern "C"
