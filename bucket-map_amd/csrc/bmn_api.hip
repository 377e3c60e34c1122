// bmn_api.hip -- host side of the indel caller (include/bmn.h): the argument checks, buffers, the launches of
// bmn_kernels.hip.h and the downloads.  A bmn_ctx owns a bms_ctx, as bmd_ctx does: its stream is the context's stream, and
// the two sorts of bmn_finish are the sorter's radix passes (bms_radix_sort, bms_ctx.hip.h) over the sorter's key and index
// buffers.  The stream of records is uploaded per bmn_add into a buffer of its own; the events stay on the device.
#include "../../include/bmn.h"

#include "bm_scan.hip.h"
#include "bmn_kernels.hip.h"
#include "bms_ctx.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMN_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMN_OK == BMS_OK && BMN_ERR_ARG == BMS_ERR_ARG && BMN_ERR_HIP == BMS_ERR_HIP, "bmn.h and bms.h must share their status codes");
static_assert(BMN_EVENT_WORDS == bmn::kEventWords && BMN_ALLELE_WORDS == bmn::kAlleleWords && BMN_CALL_WORDS == bmn::kCallWords &&
                  BMN_N_STATS == bmn::kStats && BMN_MAX_INS == bmn::kMaxIns && BMN_GENOTYPED == bmn::kGenotyped && BMN_VARIANT == bmn::kVariant,
              "bmn.h and bmn_kernels.hip.h disagree");

struct bmn_ctx {
    bms_ctx *s = nullptr;                   // owns the device, the stream and the radix buffers
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool begun = false, finished = false;
    std::vector<uint32_t> ref_len;
    std::vector<uint64_t> ref_base;         // n_ref + 1: reference r has the slots ref_base[r] .. ref_base[r + 1] - 1
    std::vector<uint64_t> add_first;        // the first event of every bmn_add with records, and the total behind them
    bmn::params pr{0, 2, 200000, 30, 4000};
    uint64_t n_slots = 0, n_events = 0, n_alleles = 0, n_calls = 0;
    DevBuf<uint8_t> in, skip;
    DevBuf<uint64_t> rec_offset, d_ref_base, rec_first, scan_tmp64;
    DevBuf<unsigned long long> stats;
    DevBuf<uint32_t> d_ref_len, cover, rec_events, rec_end, head, rank, start, a_head, a_rank, a_start, flag, c_rank, scan_tmp32;
    DevBuf<uint4> events, alleles, calls;
    float ms_add = 0.f, ms_finish = 0.f;
    uint32_t n_passes = 0;
};

namespace {

constexpr uint64_t kMaxBases = (uint64_t{1} << 32) - (uint64_t{1} << 20);   // bmp_begin's
constexpr uint64_t kMaxEvents = uint64_t{1} << 31;

#define BMN_NEED(call, bytes, what)                                                                                            \
    do {                                                                                                                       \
        if ((call) != hipSuccess) {                                                                                            \
            (void)hipGetLastError();                                                                                           \
            size_t free_b = 0, total_b = 0;                                                                                    \
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = 0;                                          \
            return fail(BMN_ERR_HIP,                                                                                           \
                        "cannot allocate %llu bytes for %s (%llu positions of %zu references at 4 bytes each, %llu events at 16 bytes each, " \
                        "%llu records, %llu stream bytes; %llu of %llu bytes of device memory are free)",                     \
                        (unsigned long long)(bytes), what, (unsigned long long)c->n_slots, c->ref_len.size(), (unsigned long long)n_events, \
                        (unsigned long long)n_records, (unsigned long long)n_bytes, (unsigned long long)free_b, (unsigned long long)total_b); \
        }                                                                                                                      \
    } while (0)

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + bmn::kThreads - 1) / bmn::kThreads); }

// what bmn_add checks of the records beyond bms_check_stream, without a context: bmp_add's checks
int check_records(const uint8_t *in, const uint64_t *rec_offset, uint64_t n_records) {
    for (uint64_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        const uint64_t length = rec_offset[i + 1] - rec_offset[i];
        uint16_t n_cigar;
        uint32_t l_seq;
        std::memcpy(&n_cigar, r + 16, 2);
        std::memcpy(&l_seq, r + 20, 4);
        const uint64_t need = 36ull + r[12] + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + l_seq;
        if (need > length)
            return fail(BMN_ERR_ARG, "bmn_add: the fields of record %llu take %llu bytes and do not fit its %llu", (unsigned long long)i,
                        (unsigned long long)need, (unsigned long long)length);
        uint64_t query = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            uint32_t c;
            std::memcpy(&c, r + 36 + r[12] + 4ull * k, 4);
            const uint32_t op = c & 15u;
            if (op > 8) return fail(BMN_ERR_ARG, "bmn_add: op %u of record %llu has the code %u, a CIGAR op is 0 .. 8", k, (unsigned long long)i, op);
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
        }
        if (n_cigar && l_seq && query != l_seq)
            return fail(BMN_ERR_ARG, "bmn_add: the CIGAR of record %llu takes %llu query bases, its l_seq is %u", (unsigned long long)i,
                        (unsigned long long)query, l_seq);
    }
    return BMN_OK;
}

// room for `want` events: a larger buffer takes over the events that are there
int grow_events(bmn_ctx *c, uint64_t want, uint64_t n_records, uint64_t n_bytes) {
    if (want <= c->events.cap && c->events.p) return BMN_OK;
    const uint64_t n_events = want;
    DevBuf<uint4> larger;
    BMN_NEED(larger.need((size_t)std::max<uint64_t>(want, 2 * c->n_events)), want * 16, "the events");
    hipStream_t s = c->s->z->stream;
    if (c->n_events) HIP_TRY(hipMemcpyAsync(larger.p, c->events.p, (size_t)c->n_events * 16, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->events = std::move(larger);
    return BMN_OK;
}

// rank[0 .. n] = the exclusive scan of head[0, n); start[k] = the place of the k-th head and start[*total] = n
int runs_of(bmn_ctx *c, const uint32_t *head, uint32_t n, DevBuf<uint32_t> &rank, DevBuf<uint32_t> &start, uint64_t *total) {
    hipStream_t s = c->s->z->stream;
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(head, rank.p, n, c->scan_tmp32.p, s));
    hipLaunchKernelGGL(bmn::starts_kernel, dim3(blocks_of(n)), dim3(bmn::kThreads), 0, s, head, rank.p, n, start.p);
    HIP_TRY(hipGetLastError());
    uint32_t heads = 0;
    HIP_TRY(hipMemcpyAsync(&heads, rank.p + n, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *total = heads;
    return BMN_OK;
}

}  // namespace

extern "C" {

const char *bmn_last_error(void) { return g_err; }

int bmn_create(int32_t device, bmn_ctx **out) {
    if (!out) return fail(BMN_ERR_ARG, "bmn_create: null argument");
    *out = nullptr;
    bms_ctx *s = nullptr;
    const int rc = bms_create(device, &s);
    if (rc != BMS_OK) return fail(rc, "bmn_create: %s", bms_last_error());
    bmn_ctx *c = new bmn_ctx();
    c->s = s;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        bmn_destroy(c);
        return fail(BMN_ERR_HIP, "bmn_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMN_OK;
}

void bmn_destroy(bmn_ctx *c) {
    if (!c) return;
    if (c->s && c->s->z) {
        (void)hipSetDevice(c->s->z->device);
        if (c->s->z->stream) (void)hipStreamSynchronize(c->s->z->stream);
    }
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->in.release(), c->skip.release(), c->stats.release();
    for (DevBuf<uint64_t> *b : {&c->rec_offset, &c->d_ref_base, &c->rec_first, &c->scan_tmp64}) b->release();
    for (DevBuf<uint32_t> *b : {&c->d_ref_len, &c->cover, &c->rec_events, &c->rec_end, &c->head, &c->rank, &c->start, &c->a_head, &c->a_rank, &c->a_start,
                                &c->flag, &c->c_rank, &c->scan_tmp32})
        b->release();
    for (DevBuf<uint4> *b : {&c->events, &c->alleles, &c->calls}) b->release();
    bms_destroy(c->s);
    delete c;
}

int bmn_begin(bmn_ctx *c, const uint32_t *ref_len, uint32_t n_ref, const uint32_t *params) {
    if (!ref_len || !params) return fail(BMN_ERR_ARG, "bmn_begin: null argument");
    if (n_ref == 0) return fail(BMN_ERR_ARG, "bmn_begin: no reference (n_ref is 0)");
    uint64_t bases = 0;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (ref_len[r] == 0) return fail(BMN_ERR_ARG, "bmn_begin: reference %u has the length 0", r);
        bases += ref_len[r];
    }
    if (bases > kMaxBases || bases + n_ref > 0xFFFFFFFEull)
        return fail(BMN_ERR_ARG, "bmn_begin: %llu bases in %u references, at most 2^32 - 2^20 bases (and 2^32 - 2 with one more per reference) in one context",
                    (unsigned long long)bases, n_ref);
    if (params[BMN_MIN_ALT] == 0) return fail(BMN_ERR_ARG, "bmn_begin: min_alt is 0, a site needs at least 1 read");
    if (params[BMN_MIN_FRAC_PPM] > 1000000u) return fail(BMN_ERR_ARG, "bmn_begin: min_frac_ppm is %u, at most 1 000 000", params[BMN_MIN_FRAC_PPM]);
    if (params[BMN_Q_INDEL] == 0 || params[BMN_Q_INDEL] > 93)
        return fail(BMN_ERR_ARG, "bmn_begin: q_indel is %u, the quality of an indel observation is 1 .. 93", params[BMN_Q_INDEL]);
    if (!c) return fail(BMN_ERR_ARG, "bmn_begin: null context");
    c->begun = c->finished = false;
    c->ms_add = c->ms_finish = 0.f;
    c->n_passes = 0;
    c->pr = bmn::params{params[BMN_MIN_MAPQ], params[BMN_MIN_ALT], params[BMN_MIN_FRAC_PPM], params[BMN_Q_INDEL], params[BMN_PRIOR]};
    c->ref_len.assign(ref_len, ref_len + n_ref);
    c->ref_base.assign((size_t)n_ref + 1, 0);
    for (uint32_t r = 0; r < n_ref; r++) c->ref_base[r + 1] = c->ref_base[r] + ref_len[r];
    c->n_slots = c->ref_base[n_ref];
    c->n_events = c->n_alleles = c->n_calls = 0;
    c->add_first.assign(1, 0);
    const uint64_t n_slots = c->n_slots, n_records = 0, n_bytes = 0, n_events = 0;
    HIP_TRY(hipSetDevice(c->s->z->device));
    hipStream_t s = c->s->z->stream;
    BMN_NEED(c->cover.need_exact((size_t)n_slots), n_slots * 4, "the cover");
    BMN_NEED(c->stats.need((size_t)n_ref * bmn::kStats), (uint64_t)n_ref * bmn::kStats * 8, "the sums");
    BMN_NEED(c->d_ref_len.need(n_ref), (uint64_t)n_ref * 4, "the reference lengths");
    BMN_NEED(c->d_ref_base.need((size_t)n_ref + 1), ((uint64_t)n_ref + 1) * 8, "the reference starts");
    BMN_NEED(c->scan_tmp32.need(bmscan::tmp_elems(n_slots)), bmscan::tmp_elems(n_slots) * 4, "the scan of the cover");
    HIP_TRY(hipMemcpyAsync(c->d_ref_len.p, c->ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_ref_base.p, c->ref_base.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(c->cover.p, 0, (size_t)n_slots * 4, s));
    HIP_TRY(hipMemsetAsync(c->stats.p, 0, (size_t)n_ref * bmn::kStats * 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    c->begun = true;
    return BMN_OK;
}

int bmn_add(bmn_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip) {
    if (!rec_offset || (n_bytes && !in)) return fail(BMN_ERR_ARG, "bmn_add: null argument");
    if (const int rc = bms_check_stream("bmn_add", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_records(in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMN_ERR_ARG, "bmn_add: null context");
    if (!c->begun) return fail(BMN_ERR_ARG, "bmn_add: no bmn_begin before it");
    if (c->finished) return fail(BMN_ERR_ARG, "bmn_add: bmn_finish has run; bmn_begin starts over");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    for (uint64_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        int32_t ref;
        std::memcpy(&ref, r + 4, 4);
        if (ref >= 0 && (uint32_t)ref >= n_ref && !(r[18] & 4u))
            return fail(BMN_ERR_ARG, "bmn_add: record %llu names reference %d, bmn_begin was given %u", (unsigned long long)i, ref, n_ref);
    }
    if (n_records == 0) return BMN_OK;
    const uint32_t n = (uint32_t)n_records;
    const uint64_t n_events = c->n_events;
    HIP_TRY(hipSetDevice(c->s->z->device));
    BMN_NEED(c->in.need((size_t)n_bytes + 16), n_bytes + 16, "the stream");
    BMN_NEED(c->rec_offset.need((size_t)n + 1), ((uint64_t)n + 1) * 8, "the record offsets");
    BMN_NEED(c->rec_events.need(n), (uint64_t)n * 4, "the event counts");
    BMN_NEED(c->rec_end.need(n), (uint64_t)n * 4, "the ends");
    BMN_NEED(c->rec_first.need((size_t)n + 1), ((uint64_t)n + 1) * 8, "the event offsets");
    BMN_NEED(c->scan_tmp64.need(bmscan::tmp_elems(n)), bmscan::tmp_elems(n) * 8, "the scan of the event counts");
    if (skip) BMN_NEED(c->skip.need(n), (uint64_t)n, "the skip bytes");
    hipStream_t s = c->s->z->stream;
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_offset.p, rec_offset, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    if (skip) HIP_TRY(hipMemcpyAsync(c->skip.p, skip, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmn::count_kernel, dim3(blocks_of(n)), dim3(bmn::kThreads), 0, s, c->in.p, c->rec_offset.p, n, skip ? c->skip.p : nullptr,
                       c->d_ref_len.p, c->d_ref_base.p, n_ref, c->pr.min_mapq, c->cover.p, c->stats.p, c->rec_events.p, c->rec_end.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(bmscan::exclusive_sum<uint64_t>(c->rec_events.p, c->rec_first.p, n, c->scan_tmp64.p, s));
    uint64_t found = 0;
    HIP_TRY(hipMemcpyAsync(&found, c->rec_first.p + n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // the cover and the sums of this add are in; without room for its events the context cannot go on
    if (c->n_events + found >= kMaxEvents) {
        c->begun = false;
        return fail(BMN_ERR_HIP, "bmn_add: %llu events and %llu more, fewer than 2^31 fit one context; bmn_begin starts over",
                    (unsigned long long)c->n_events, (unsigned long long)found);
    }
    if (found) {
        if (const int rc = grow_events(c, c->n_events + found, n_records, n_bytes)) {
            c->begun = false;
            return rc;
        }
        hipLaunchKernelGGL(bmn::emit_kernel, dim3(blocks_of(n)), dim3(bmn::kThreads), 0, s, c->in.p, c->rec_offset.p, n, c->d_ref_len.p, c->d_ref_base.p,
                           c->rec_events.p, c->rec_end.p, c->rec_first.p, c->n_events, c->events.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->ms_add += ms;
    c->n_events += found;
    c->add_first.push_back(c->n_events);
    return BMN_OK;
}

int bmn_finish(bmn_ctx *c, uint64_t *out_n_events, uint64_t *out_n_alleles, uint64_t *out_n_calls, uint64_t *out_ref_stats) {
    if (!out_n_events || !out_n_alleles || !out_n_calls || !out_ref_stats) return fail(BMN_ERR_ARG, "bmn_finish: null argument");
    if (!c) return fail(BMN_ERR_ARG, "bmn_finish: null context");
    if (!c->begun) return fail(BMN_ERR_ARG, "bmn_finish: no bmn_begin before it");
    if (c->finished) return fail(BMN_ERR_ARG, "bmn_finish: called twice; bmn_begin starts over");
    const uint32_t n_ref = (uint32_t)c->ref_len.size(), n = (uint32_t)c->n_events;
    const uint64_t n_events = c->n_events, n_records = 0, n_bytes = 0;
    HIP_TRY(hipSetDevice(c->s->z->device));
    bms_ctx *b = c->s;
    hipStream_t s = b->z->stream;
    c->begun = false;                                    // a failure below leaves no half-finished state behind
    const size_t n_tmp = std::max(bmscan::tmp_elems(c->n_slots), bmscan::tmp_elems((uint64_t)n + 1));
    BMN_NEED(c->scan_tmp32.need(n_tmp), (uint64_t)n_tmp * 4, "the scans");
    HIP_TRY(hipEventRecord(c->ev[0], s));
    // the cover: block sums, their scan, the inclusive scan in place
    {
        const uint64_t n_blocks = (c->n_slots + bmscan::kTile - 1) / bmscan::kTile;
        hipLaunchKernelGGL(bmscan::block_sums_kernel<uint32_t>, dim3((unsigned)n_blocks), dim3(bmscan::kThreads), 0, s, c->cover.p, c->n_slots, c->scan_tmp32.p);
        hipLaunchKernelGGL(bmscan::scan_sums_kernel<uint32_t>, dim3(1), dim3(bmscan::kThreads), 0, s, c->scan_tmp32.p, n_blocks);
        hipLaunchKernelGGL(bmn::cover_scan_kernel, dim3((unsigned)n_blocks), dim3(bmscan::kThreads), 0, s, c->cover.p, c->n_slots, c->scan_tmp32.p);
        HIP_TRY(hipGetLastError());
    }
    c->n_alleles = c->n_calls = 0;
    if (n) {
        if (bms_need_radix(b, n, 0)) return fail(BMN_ERR_HIP, "%s", bms_last_error());
        BMN_NEED(c->head.need(n), (uint64_t)n * 4, "the run heads");
        BMN_NEED(c->rank.need((size_t)n + 1), ((uint64_t)n + 1) * 4, "the run ranks");
        BMN_NEED(c->start.need((size_t)n + 1), ((uint64_t)n + 1) * 4, "the run starts");
        // two stable sorts give the order of the 128-bit key: seq first, then slot << 32 | w1
        int side = 0;
        hipLaunchKernelGGL(bmn::seq_keys_kernel, dim3(blocks_of(n)), dim3(bmn::kThreads), 0, s, c->events.p, n, b->key[0].p, b->index[0].p);
        HIP_TRY(hipGetLastError());
        if (const int rc = bms_radix_sort(b, n, &side, &c->n_passes)) return fail(rc, "%s", bms_last_error());
        hipLaunchKernelGGL(bmn::slot_keys_kernel, dim3(blocks_of(n)), dim3(bmn::kThreads), 0, s, c->events.p, b->index[side].p, n, b->key[side].p);
        HIP_TRY(hipGetLastError());
        if (const int rc = bms_radix_sort(b, n, &side, &c->n_passes)) return fail(rc, "%s", bms_last_error());
        // the runs of equal events are the alleles
        hipLaunchKernelGGL(bmn::run_heads_kernel, dim3(blocks_of(n)), dim3(bmn::kThreads), 0, s, c->events.p, b->index[side].p, n, c->head.p);
        HIP_TRY(hipGetLastError());
        if (const int rc = runs_of(c, c->head.p, n, c->rank, c->start, &c->n_alleles)) return rc;
        const uint32_t na = (uint32_t)c->n_alleles;
        BMN_NEED(c->alleles.need((size_t)na * 2), (uint64_t)na * 32, "the alleles");
        BMN_NEED(c->a_head.need(na), (uint64_t)na * 4, "the anchor heads");
        BMN_NEED(c->a_rank.need((size_t)na + 1), ((uint64_t)na + 1) * 4, "the anchor ranks");
        BMN_NEED(c->a_start.need((size_t)na + 1), ((uint64_t)na + 1) * 4, "the anchor starts");
        hipLaunchKernelGGL(bmn::alleles_kernel, dim3(blocks_of(na)), dim3(bmn::kThreads), 0, s, c->events.p, b->index[side].p, c->start.p, na,
                           c->d_ref_base.p, n_ref, c->alleles.p);
        HIP_TRY(hipGetLastError());
        // the runs of alleles on one anchor; a site flag per anchor, its scan, the calls at their ranks
        const uint32_t *words = reinterpret_cast<const uint32_t *>(c->alleles.p);
        hipLaunchKernelGGL(bmn::anchor_heads_kernel, dim3(blocks_of(na)), dim3(bmn::kThreads), 0, s, words, na, c->a_head.p);
        HIP_TRY(hipGetLastError());
        uint64_t n_anchors = 0;
        if (const int rc = runs_of(c, c->a_head.p, na, c->a_rank, c->a_start, &n_anchors)) return rc;
        const uint32_t nk = (uint32_t)n_anchors;
        BMN_NEED(c->flag.need(nk), (uint64_t)nk * 4, "the site flags");
        BMN_NEED(c->c_rank.need((size_t)nk + 1), ((uint64_t)nk + 1) * 4, "the call ranks");
        hipLaunchKernelGGL(bmn::calls_kernel<false>, dim3(blocks_of(nk)), dim3(bmn::kThreads), 0, s, words, c->a_start.p, nk, c->cover.p, c->d_ref_base.p,
                           c->pr, c->flag.p, nullptr, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->flag.p, c->c_rank.p, nk, c->scan_tmp32.p, s));
        uint32_t n_calls = 0;
        HIP_TRY(hipMemcpyAsync(&n_calls, c->c_rank.p + nk, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        c->n_calls = n_calls;
        if (n_calls) {
            BMN_NEED(c->calls.need((size_t)n_calls * 4), (uint64_t)n_calls * 64, "the calls");
            hipLaunchKernelGGL(bmn::calls_kernel<true>, dim3(blocks_of(nk)), dim3(bmn::kThreads), 0, s, words, c->a_start.p, nk, c->cover.p, c->d_ref_base.p,
                               c->pr, c->flag.p, c->c_rank.p, c->calls.p);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipMemcpyAsync(out_ref_stats, c->stats.p, (size_t)n_ref * bmn::kStats * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&c->ms_finish, c->ev[0], c->ev[1]));
    *out_n_events = c->n_events, *out_n_alleles = c->n_alleles, *out_n_calls = c->n_calls;
    c->begun = c->finished = true;
    return BMN_OK;
}

int bmn_alleles(bmn_ctx *c, uint64_t first, uint64_t count, uint32_t *out) {
    if (count && !out) return fail(BMN_ERR_ARG, "bmn_alleles: null argument");
    if (!c) return fail(BMN_ERR_ARG, "bmn_alleles: null context");
    if (!c->finished) return fail(BMN_ERR_ARG, "bmn_alleles: no bmn_finish before it");
    if (first > c->n_alleles || count > c->n_alleles - first)
        return fail(BMN_ERR_ARG, "bmn_alleles: alleles %llu .. + %llu asked for, there are %llu", (unsigned long long)first, (unsigned long long)count,
                    (unsigned long long)c->n_alleles);
    if (count == 0) return BMN_OK;
    HIP_TRY(hipSetDevice(c->s->z->device));
    HIP_TRY(hipMemcpyAsync(out, c->alleles.p + 2 * first, (size_t)count * 32, hipMemcpyDeviceToHost, c->s->z->stream));
    HIP_TRY(hipStreamSynchronize(c->s->z->stream));
    return BMN_OK;
}

int bmn_calls(bmn_ctx *c, uint64_t first, uint64_t count, uint32_t *out) {
    if (count && !out) return fail(BMN_ERR_ARG, "bmn_calls: null argument");
    if (!c) return fail(BMN_ERR_ARG, "bmn_calls: null context");
    if (!c->finished) return fail(BMN_ERR_ARG, "bmn_calls: no bmn_finish before it");
    if (first > c->n_calls || count > c->n_calls - first)
        return fail(BMN_ERR_ARG, "bmn_calls: calls %llu .. + %llu asked for, there are %llu", (unsigned long long)first, (unsigned long long)count,
                    (unsigned long long)c->n_calls);
    if (count == 0) return BMN_OK;
    HIP_TRY(hipSetDevice(c->s->z->device));
    HIP_TRY(hipMemcpyAsync(out, c->calls.p + 4 * first, (size_t)count * 64, hipMemcpyDeviceToHost, c->s->z->stream));
    HIP_TRY(hipStreamSynchronize(c->s->z->stream));
    return BMN_OK;
}

int bmn_events_of(bmn_ctx *c, uint64_t add, uint64_t *out_n_adds, uint64_t *out_n_events, uint32_t *out_events) {
    if (!out_n_adds || (out_events && !out_n_events)) return fail(BMN_ERR_ARG, "bmn_events_of: null argument");
    if (!c) return fail(BMN_ERR_ARG, "bmn_events_of: null context");
    if (!c->begun) return fail(BMN_ERR_ARG, "bmn_events_of: no bmn_begin before it");
    const uint64_t n_adds = c->add_first.size() - 1;
    *out_n_adds = n_adds;
    if (!out_n_events) return BMN_OK;
    if (add >= n_adds) return fail(BMN_ERR_ARG, "bmn_events_of: add %llu asked for, %llu have run", (unsigned long long)add, (unsigned long long)n_adds);
    const uint64_t first = c->add_first[add], count = c->add_first[add + 1] - first;
    *out_n_events = count;
    if (!out_events || count == 0) return BMN_OK;
    HIP_TRY(hipSetDevice(c->s->z->device));
    HIP_TRY(hipMemcpyAsync(out_events, c->events.p + first, (size_t)count * 16, hipMemcpyDeviceToHost, c->s->z->stream));
    HIP_TRY(hipStreamSynchronize(c->s->z->stream));
    return BMN_OK;
}

int bmn_cover_at(bmn_ctx *c, uint32_t ref, uint32_t start, uint32_t count, uint32_t *out) {
    if (count && !out) return fail(BMN_ERR_ARG, "bmn_cover_at: null argument");
    if (!c) return fail(BMN_ERR_ARG, "bmn_cover_at: null context");
    if (!c->finished) return fail(BMN_ERR_ARG, "bmn_cover_at: no bmn_finish before it");
    if (ref >= c->ref_len.size()) return fail(BMN_ERR_ARG, "bmn_cover_at: reference %u of %zu", ref, c->ref_len.size());
    if ((uint64_t)start + count > c->ref_len[ref])
        return fail(BMN_ERR_ARG, "bmn_cover_at: bases %u .. %u + %u asked for, reference %u has %u", start, start, count, ref, c->ref_len[ref]);
    if (count == 0) return BMN_OK;
    HIP_TRY(hipSetDevice(c->s->z->device));
    HIP_TRY(hipMemcpyAsync(out, c->cover.p + c->ref_base[ref] + start, (size_t)count * 4, hipMemcpyDeviceToHost, c->s->z->stream));
    HIP_TRY(hipStreamSynchronize(c->s->z->stream));
    return BMN_OK;
}

int bmn_last_stats(bmn_ctx *c, float *ms_add, float *ms_finish) {
    if (!c) return fail(BMN_ERR_ARG, "bmn_last_stats: null argument");
    if (ms_add) *ms_add = c->ms_add;
    if (ms_finish) *ms_finish = c->ms_finish;
    return BMN_OK;
}

}  // extern "C"
