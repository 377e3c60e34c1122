// bmp_api.hip -- host side of the pileup counter (include/bmp.h): the argument checks, buffers, the launches of
// bmp_kernels.hip.h and the downloads.  A bmp_ctx owns its stream and every buffer; the stream of records is uploaded per
// bmp_add into a buffer of its own, as bmc_api.hip does (the sorter's copy belongs to another context).
#include "../../include/bmp.h"

#include "bm_hip_util.h"
#include "bm_scan.hip.h"
#include "bmp_kernels.hip.h"
#include "bms_ctx.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMP_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMP_OK == BMS_OK && BMP_ERR_ARG == BMS_ERR_ARG && BMP_ERR_HIP == BMS_ERR_HIP, "bmp.h and bms.h must share their status codes");
static_assert(BMP_N_STATS == bmp::kStats && BMP_N_COUNTERS == bmp::kCounters && BMP_SITE_WORDS == bmp::kSiteWords && BMP_DEL == bmp::kDel &&
                  BMP_INS == bmp::kIns && BMP_LOWQ == bmp::kLowq,
              "bmp.h and bmp_kernels.hip.h disagree");

struct bmp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    enum { kIdle, kBegun, kFinished } state = kIdle;
    std::vector<uint32_t> ref_len;
    std::vector<uint64_t> ref_base;         // n_ref + 1: reference r has the slots ref_base[r] .. ref_base[r + 1] - 1
    bmp::thresholds th{0, 0, 1, 0};
    uint64_t n_slots = 0, n_sites = 0;
    DevBuf<uint8_t> in, skip, ref;
    DevBuf<uint64_t> rec_offset, d_ref_base;
    DevBuf<uint32_t> d_ref_len, cnt, scan_tmp, tile_count, tile_rank, sites;
    DevBuf<unsigned long long> stats;
    float ms_add = 0.f, ms_finish = 0.f;
};

namespace {

constexpr uint64_t kMaxBases = (uint64_t{1} << 32) - (uint64_t{1} << 20);

#define BMP_NEED(call, bytes, what)                                                                                            \
    do {                                                                                                                       \
        if ((call) != hipSuccess) {                                                                                            \
            (void)hipGetLastError();                                                                                           \
            size_t free_b = 0, total_b = 0;                                                                                    \
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = 0;                                          \
            return fail(BMP_ERR_HIP,                                                                                           \
                        "cannot allocate %llu bytes for %s (%llu positions of %zu references at 33 bytes each, %llu records, %llu stream bytes, " \
                        "%llu sites; %llu of %llu bytes of device memory are free)",                                           \
                        (unsigned long long)(bytes), what, (unsigned long long)c->n_slots, c->ref_len.size(), (unsigned long long)n_records, \
                        (unsigned long long)n_bytes, (unsigned long long)c->n_sites, (unsigned long long)free_b, (unsigned long long)total_b); \
        }                                                                                                                      \
    } while (0)

// what bmp_add checks of the records beyond bms_check_stream, without a context: bmc_add's checks
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
            return fail(BMP_ERR_ARG, "bmp_add: the fields of record %llu take %llu bytes and do not fit its %llu", (unsigned long long)i,
                        (unsigned long long)need, (unsigned long long)length);
        uint64_t query = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            uint32_t c;
            std::memcpy(&c, r + 36 + r[12] + 4ull * k, 4);
            const uint32_t op = c & 15u;
            if (op > 8) return fail(BMP_ERR_ARG, "bmp_add: op %u of record %llu has the code %u, a CIGAR op is 0 .. 8", k, (unsigned long long)i, op);
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
        }
        if (n_cigar && l_seq && query != l_seq)
            return fail(BMP_ERR_ARG, "bmp_add: the CIGAR of record %llu takes %llu query bases, its l_seq is %u", (unsigned long long)i,
                        (unsigned long long)query, l_seq);
    }
    return BMP_OK;
}

}  // namespace

extern "C" {

const char *bmp_last_error(void) { return g_err; }

int bmp_create(int32_t device, bmp_ctx **out) {
    if (!out) return fail(BMP_ERR_ARG, "bmp_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMP_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    bmp_ctx *c = new bmp_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        bmp_destroy(c);
        return fail(BMP_ERR_HIP, "bmp_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMP_OK;
}

void bmp_destroy(bmp_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->in.release(), c->skip.release(), c->ref.release(), c->rec_offset.release(), c->d_ref_base.release(), c->stats.release();
    for (DevBuf<uint32_t> *b : {&c->d_ref_len, &c->cnt, &c->scan_tmp, &c->tile_count, &c->tile_rank, &c->sites}) b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmp_begin(bmp_ctx *c, const uint32_t *ref_len, uint32_t n_ref, const uint8_t *const *ref_bases, const uint32_t *thresholds) {
    if (!ref_len || !ref_bases || !thresholds) return fail(BMP_ERR_ARG, "bmp_begin: null argument");
    if (n_ref == 0) return fail(BMP_ERR_ARG, "bmp_begin: no reference (n_ref is 0)");
    uint64_t bases = 0;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (ref_len[r] == 0) return fail(BMP_ERR_ARG, "bmp_begin: reference %u has the length 0", r);
        bases += ref_len[r];
    }
    if (bases > kMaxBases || bases + n_ref > 0xFFFFFFFEull)
        return fail(BMP_ERR_ARG, "bmp_begin: %llu bases in %u references, at most 2^32 - 2^20 bases (and 2^32 - 2 with one more per reference) in one context",
                    (unsigned long long)bases, n_ref);
    if (thresholds[BMP_MIN_ALT] == 0) return fail(BMP_ERR_ARG, "bmp_begin: min_alt is 0, a site needs at least 1 differing read");
    if (thresholds[BMP_MIN_FRAC_PPM] > 1000000u)
        return fail(BMP_ERR_ARG, "bmp_begin: min_frac_ppm is %u, a fraction is 0 .. 1000000 ppm", thresholds[BMP_MIN_FRAC_PPM]);
    for (uint32_t r = 0; r < n_ref; r++)
        if (!ref_bases[r]) return fail(BMP_ERR_ARG, "bmp_begin: reference %u has no bases (a null ref_bases entry)", r);
    if (!c) return fail(BMP_ERR_ARG, "bmp_begin: null context");
    c->state = bmp_ctx::kIdle;
    c->ms_add = c->ms_finish = 0.f;
    c->n_sites = 0;
    c->th = bmp::thresholds{thresholds[BMP_MIN_MAPQ], thresholds[BMP_MIN_BQ], thresholds[BMP_MIN_ALT], thresholds[BMP_MIN_FRAC_PPM]};
    c->ref_len.assign(ref_len, ref_len + n_ref);
    c->ref_base.assign((size_t)n_ref + 1, 0);
    for (uint32_t r = 0; r < n_ref; r++) c->ref_base[r + 1] = c->ref_base[r] + ref_len[r];
    c->n_slots = c->ref_base[n_ref];
    const uint64_t n_slots = c->n_slots, n_tiles = (n_slots + bmp::kTile - 1) / bmp::kTile, n_records = 0, n_bytes = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMP_NEED(c->cnt.need_exact((size_t)n_slots * bmp::kCounters), n_slots * bmp::kCounters * 4, "the counters");
    BMP_NEED(c->ref.need_exact((size_t)n_slots + bmp::kRefPad), n_slots + bmp::kRefPad, "the reference bases");
    BMP_NEED(c->scan_tmp.need(bmscan::tmp_elems(n_tiles)), bmscan::tmp_elems(n_tiles) * 4, "the scan of the tiles' site counts");
    BMP_NEED(c->tile_count.need(n_tiles), n_tiles * 4, "the tiles' site counts");
    BMP_NEED(c->tile_rank.need(n_tiles + 1), (n_tiles + 1) * 4, "the tiles' site ranks");
    BMP_NEED(c->d_ref_len.need(n_ref), (uint64_t)n_ref * 4, "the reference lengths");
    BMP_NEED(c->d_ref_base.need((size_t)n_ref + 1), ((uint64_t)n_ref + 1) * 8, "the reference starts");
    BMP_NEED(c->stats.need((size_t)n_ref * bmp::kStats), (uint64_t)n_ref * bmp::kStats * 8, "the reference sums");
    HIP_TRY(hipMemcpyAsync(c->d_ref_len.p, c->ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_ref_base.p, c->ref_base.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->cnt.p, 0, (size_t)n_slots * bmp::kCounters * 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->ref.p + n_slots, 0, bmp::kRefPad, c->stream));
    HIP_TRY(hipMemsetAsync(c->stats.p, 0, (size_t)n_ref * bmp::kStats * 8, c->stream));
    std::vector<uint64_t> lens(ref_len, ref_len + n_ref);
    HIP_TRY(bmhip::upload_pageable_records(c->ref.p, ref_bases, lens.data(), n_ref));   // on a stream of its own; waits for it
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->state = bmp_ctx::kBegun;
    return BMP_OK;
}

int bmp_add(bmp_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip) {
    if (!rec_offset || (n_bytes && !in)) return fail(BMP_ERR_ARG, "bmp_add: null argument");
    if (const int rc = bms_check_stream("bmp_add", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_records(in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMP_ERR_ARG, "bmp_add: null context");
    if (c->state != bmp_ctx::kBegun) return fail(BMP_ERR_ARG, "bmp_add: no bmp_begin before it, or a bmp_finish since");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    for (uint64_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        int32_t ref;
        std::memcpy(&ref, r + 4, 4);
        if (ref >= 0 && (uint32_t)ref >= n_ref && !(r[18] & 4u))
            return fail(BMP_ERR_ARG, "bmp_add: record %llu names reference %d, bmp_begin was given %u", (unsigned long long)i, ref, n_ref);
    }
    if (n_records == 0) return BMP_OK;
    const uint32_t n = (uint32_t)n_records;
    HIP_TRY(hipSetDevice(c->device));
    BMP_NEED(c->in.need((size_t)n_bytes + 16), n_bytes + 16, "the stream");   // bases_shared reads whole aligned words
    BMP_NEED(c->rec_offset.need((size_t)n + 1), ((uint64_t)n + 1) * 8, "the record offsets");
    if (skip) BMP_NEED(c->skip.need(n), (uint64_t)n, "the skip bytes");
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_offset.p, rec_offset, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    if (skip) HIP_TRY(hipMemcpyAsync(c->skip.p, skip, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmp::add_kernel, dim3((n + bmp::kThreads - 1) / bmp::kThreads), dim3(bmp::kThreads), 0, s, c->in.p, c->rec_offset.p, n,
                       skip ? c->skip.p : nullptr, c->d_ref_len.p, c->d_ref_base.p, n_ref, c->th, c->cnt.p, c->stats.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->ms_add += ms;
    return BMP_OK;
}

int bmp_finish(bmp_ctx *c, uint64_t *out_n_sites, uint64_t *out_ref_stats) {
    if (!out_n_sites || !out_ref_stats) return fail(BMP_ERR_ARG, "bmp_finish: null argument");
    if (!c) return fail(BMP_ERR_ARG, "bmp_finish: null context");
    if (c->state != bmp_ctx::kBegun) return fail(BMP_ERR_ARG, "bmp_finish: no bmp_begin before it, or a second bmp_finish");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    const uint64_t n_slots = c->n_slots, n_tiles = (n_slots + bmp::kTile - 1) / bmp::kTile, n_records = 0, n_bytes = 0;
    hipStream_t s = c->stream;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmp::sites_count_kernel, dim3((uint32_t)n_tiles), dim3(bmp::kThreads), 0, s, c->cnt.p, c->ref.p, n_slots, c->d_ref_base.p, n_ref,
                       c->th, c->tile_count.p, c->stats.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->tile_count.p, c->tile_rank.p, n_tiles, c->scan_tmp.p, s));
    uint32_t n_sites = 0;
    HIP_TRY(hipMemcpyAsync(&n_sites, c->tile_rank.p + n_tiles, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_sites > n_slots) return fail(BMP_ERR_HIP, "bmp_finish: %u sites counted over %llu positions", n_sites, (unsigned long long)n_slots);
    c->n_sites = n_sites;                                // for the message of a list that does not fit
    c->state = bmp_ctx::kIdle;                           // this pass's sums are in the stats: a failure from here on ends the counting
    BMP_NEED(c->sites.need((size_t)n_sites * bmp::kSiteWords), (uint64_t)n_sites * bmp::kSiteWords * 4, "the sites");
    c->n_sites = 0;
    if (n_sites) {
        hipLaunchKernelGGL(bmp::sites_emit_kernel, dim3((uint32_t)n_tiles), dim3(bmp::kThreads), 0, s, c->cnt.p, c->ref.p, n_slots, c->d_ref_base.p, n_ref,
                           c->th, c->tile_rank.p, n_sites, c->sites.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipMemcpyAsync(out_ref_stats, c->stats.p, (size_t)n_ref * bmp::kStats * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&c->ms_finish, c->ev[0], c->ev[1]));
    c->n_sites = n_sites;
    *out_n_sites = n_sites;
    c->state = bmp_ctx::kFinished;
    return BMP_OK;
}

int bmp_sites(bmp_ctx *c, uint64_t first, uint64_t count, uint32_t *out) {
    if (count && !out) return fail(BMP_ERR_ARG, "bmp_sites: null argument");
    if (!c) return fail(BMP_ERR_ARG, "bmp_sites: null context");
    if (c->state != bmp_ctx::kFinished) return fail(BMP_ERR_ARG, "bmp_sites: no bmp_finish before it");
    if (first > c->n_sites || count > c->n_sites - first)
        return fail(BMP_ERR_ARG, "bmp_sites: sites %llu .. %llu + %llu asked for, there are %llu", (unsigned long long)first, (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)c->n_sites);
    if (count == 0) return BMP_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->sites.p + bmp::kSiteWords * first, (size_t)count * bmp::kSiteWords * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMP_OK;
}

int bmp_counts_at(bmp_ctx *c, uint32_t ref, uint32_t start, uint32_t count, uint32_t *out) {
    if (count && !out) return fail(BMP_ERR_ARG, "bmp_counts_at: null argument");
    if (!c) return fail(BMP_ERR_ARG, "bmp_counts_at: null context");
    if (c->state != bmp_ctx::kFinished) return fail(BMP_ERR_ARG, "bmp_counts_at: no bmp_finish before it");
    if (ref >= c->ref_len.size()) return fail(BMP_ERR_ARG, "bmp_counts_at: reference %u of %zu", ref, c->ref_len.size());
    if ((uint64_t)start + count > c->ref_len[ref])
        return fail(BMP_ERR_ARG, "bmp_counts_at: bases %u .. %u + %u asked for, reference %u has %u", start, start, count, ref, c->ref_len[ref]);
    if (count == 0) return BMP_OK;
    HIP_TRY(hipSetDevice(c->device));
    // counter-major: the eight counters of a position lie together, a stretch of positions is one plain copy
    HIP_TRY(hipMemcpyAsync(out, c->cnt.p + (c->ref_base[ref] + start) * bmp::kCounters, (size_t)count * bmp::kCounters * 4, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMP_OK;
}

int bmp_last_stats(bmp_ctx *c, float *ms_add, float *ms_finish) {
    if (!c) return fail(BMP_ERR_ARG, "bmp_last_stats: null argument");
    if (ms_add) *ms_add = c->ms_add;
    if (ms_finish) *ms_finish = c->ms_finish;
    return BMP_OK;
}

}  // extern "C"
