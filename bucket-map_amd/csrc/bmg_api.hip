// bmg_api.hip -- host side of the genotype caller (include/bmg.h): the argument checks, buffers, the launches of
// bmg_kernels.hip.h and the downloads.  A bmg_ctx owns its stream and every buffer; the stream of records is uploaded per
// bmg_add into a buffer of its own, as bmp_api.hip does, and the sites of a bmg_call per call.
#include "../../include/bmg.h"

#include "bm_hip_util.h"
#include "bmg_ctx.hip.h"
#include "bmg_kernels.hip.h"
#include "bms_ctx.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMG_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMG_OK == BMS_OK && BMG_ERR_ARG == BMS_ERR_ARG && BMG_ERR_HIP == BMS_ERR_HIP, "bmg.h and bms.h must share their status codes");
static_assert(BMG_N_CELLS == bmg::kCells && BMG_N_GENOTYPES == bmg::kGenotypes && BMG_SITE_WORDS == bmg::kSiteWords && BMG_CALL_WORDS == bmg::kCallWords &&
                  BMG_GENOTYPED == bmg::kGenotyped && BMG_VARIANT == bmg::kVariant,
              "bmg.h and bmg_kernels.hip.h disagree");

namespace {

constexpr uint64_t kMaxBases = (uint64_t{1} << 32) - (uint64_t{1} << 20);   // bmp_begin's
constexpr uint64_t kMaxSites = uint64_t{1} << 31;

#define BMG_NEED(call, bytes, what)                                                                                            \
    do {                                                                                                                       \
        if ((call) != hipSuccess) {                                                                                            \
            (void)hipGetLastError();                                                                                           \
            size_t free_b = 0, total_b = 0;                                                                                    \
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = 0;                                          \
            return fail(BMG_ERR_HIP,                                                                                           \
                        "cannot allocate %llu bytes for %s (%llu positions of %zu references at 32 bytes each, %llu records, %llu stream bytes, " \
                        "%llu sites; %llu of %llu bytes of device memory are free)",                                           \
                        (unsigned long long)(bytes), what, (unsigned long long)c->n_slots, c->ref_len.size(), (unsigned long long)n_records, \
                        (unsigned long long)n_bytes, (unsigned long long)n_sites, (unsigned long long)free_b, (unsigned long long)total_b); \
        }                                                                                                                      \
    } while (0)

// what bmg_add checks of the records beyond bms_check_stream, without a context: bmp_add's checks
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
            return fail(BMG_ERR_ARG, "bmg_add: the fields of record %llu take %llu bytes and do not fit its %llu", (unsigned long long)i,
                        (unsigned long long)need, (unsigned long long)length);
        uint64_t query = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            uint32_t c;
            std::memcpy(&c, r + 36 + r[12] + 4ull * k, 4);
            const uint32_t op = c & 15u;
            if (op > 8) return fail(BMG_ERR_ARG, "bmg_add: op %u of record %llu has the code %u, a CIGAR op is 0 .. 8", k, (unsigned long long)i, op);
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
        }
        if (n_cigar && l_seq && query != l_seq)
            return fail(BMG_ERR_ARG, "bmg_add: the CIGAR of record %llu takes %llu query bases, its l_seq is %u", (unsigned long long)i,
                        (unsigned long long)query, l_seq);
    }
    return BMG_OK;
}

}  // namespace

extern "C" {

const char *bmg_last_error(void) { return g_err; }

int bmg_create(int32_t device, bmg_ctx **out) {
    if (!out) return fail(BMG_ERR_ARG, "bmg_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMG_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    bmg_ctx *c = new bmg_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        bmg_destroy(c);
        return fail(BMG_ERR_HIP, "bmg_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMG_OK;
}

void bmg_destroy(bmg_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->in.release(), c->skip.release(), c->rec_offset.release(), c->d_ref_base.release(), c->cell.release();
    for (DevBuf<uint32_t> *b : {&c->d_ref_len, &c->sites, &c->calls}) b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmg_begin(bmg_ctx *c, const uint32_t *ref_len, uint32_t n_ref, const uint32_t *params) {
    if (!ref_len || !params) return fail(BMG_ERR_ARG, "bmg_begin: null argument");
    if (n_ref == 0) return fail(BMG_ERR_ARG, "bmg_begin: no reference (n_ref is 0)");
    uint64_t bases = 0;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (ref_len[r] == 0) return fail(BMG_ERR_ARG, "bmg_begin: reference %u has the length 0", r);
        bases += ref_len[r];
    }
    if (bases > kMaxBases || bases + n_ref > 0xFFFFFFFEull)
        return fail(BMG_ERR_ARG, "bmg_begin: %llu bases in %u references, at most 2^32 - 2^20 bases (and 2^32 - 2 with one more per reference) in one context",
                    (unsigned long long)bases, n_ref);
    if (params[BMG_Q_CAP] == 0 || params[BMG_Q_CAP] > 93)
        return fail(BMG_ERR_ARG, "bmg_begin: q_cap is %u, the most a base quality counts for is 1 .. 93", params[BMG_Q_CAP]);
    if (params[BMG_Q_ABSENT] > params[BMG_Q_CAP])
        return fail(BMG_ERR_ARG, "bmg_begin: q_absent is %u, above q_cap %u", params[BMG_Q_ABSENT], params[BMG_Q_CAP]);
    if (!c) return fail(BMG_ERR_ARG, "bmg_begin: null context");
    c->begun = false;
    c->ms_add = c->ms_call = 0.f;
    c->pr = bmg::params{params[BMG_MIN_MAPQ], params[BMG_MIN_BQ], params[BMG_Q_ABSENT], params[BMG_Q_CAP], params[BMG_PRIOR]};
    c->ref_len.assign(ref_len, ref_len + n_ref);
    c->ref_base.assign((size_t)n_ref + 1, 0);
    for (uint32_t r = 0; r < n_ref; r++) c->ref_base[r + 1] = c->ref_base[r] + ref_len[r];
    c->n_slots = c->ref_base[n_ref];
    const uint64_t n_slots = c->n_slots, n_records = 0, n_bytes = 0, n_sites = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMG_NEED(c->cell.need_exact((size_t)n_slots * bmg::kCells), n_slots * bmg::kCells * 8, "the cells");
    BMG_NEED(c->d_ref_len.need(n_ref), (uint64_t)n_ref * 4, "the reference lengths");
    BMG_NEED(c->d_ref_base.need((size_t)n_ref + 1), ((uint64_t)n_ref + 1) * 8, "the reference starts");
    HIP_TRY(hipMemcpyAsync(c->d_ref_len.p, c->ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_ref_base.p, c->ref_base.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->cell.p, 0, (size_t)n_slots * bmg::kCells * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->begun = true;
    return BMG_OK;
}

int bmg_add(bmg_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip) {
    if (!rec_offset || (n_bytes && !in)) return fail(BMG_ERR_ARG, "bmg_add: null argument");
    if (const int rc = bms_check_stream("bmg_add", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_records(in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMG_ERR_ARG, "bmg_add: null context");
    if (!c->begun) return fail(BMG_ERR_ARG, "bmg_add: no bmg_begin before it");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    for (uint64_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        int32_t ref;
        std::memcpy(&ref, r + 4, 4);
        if (ref >= 0 && (uint32_t)ref >= n_ref && !(r[18] & 4u))
            return fail(BMG_ERR_ARG, "bmg_add: record %llu names reference %d, bmg_begin was given %u", (unsigned long long)i, ref, n_ref);
    }
    if (n_records == 0) return BMG_OK;
    const uint32_t n = (uint32_t)n_records;
    const uint64_t n_sites = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMG_NEED(c->in.need((size_t)n_bytes + 16), n_bytes + 16, "the stream");   // bases_shared reads whole aligned words
    BMG_NEED(c->rec_offset.need((size_t)n + 1), ((uint64_t)n + 1) * 8, "the record offsets");
    if (skip) BMG_NEED(c->skip.need(n), (uint64_t)n, "the skip bytes");
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_offset.p, rec_offset, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    if (skip) HIP_TRY(hipMemcpyAsync(c->skip.p, skip, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmg::add_kernel, dim3((n + bmg::kThreads - 1) / bmg::kThreads), dim3(bmg::kThreads), 0, s, c->in.p, c->rec_offset.p, n,
                       skip ? c->skip.p : nullptr, c->d_ref_len.p, c->d_ref_base.p, n_ref, c->pr, c->cell.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->ms_add += ms;
    return BMG_OK;
}

int bmg_call(bmg_ctx *c, const uint32_t *sites, uint64_t n_sites, uint32_t *out) {
    if (n_sites && (!sites || !out)) return fail(BMG_ERR_ARG, "bmg_call: null argument");
    if (n_sites >= kMaxSites) return fail(BMG_ERR_ARG, "bmg_call: %llu sites, fewer than 2^31 are called in one go", (unsigned long long)n_sites);
    if (!c) return fail(BMG_ERR_ARG, "bmg_call: null context");
    if (!c->begun) return fail(BMG_ERR_ARG, "bmg_call: no bmg_begin before it");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    for (uint64_t i = 0; i < n_sites; i++) {
        const uint32_t ref = sites[bmg::kSiteWords * i], pos = sites[bmg::kSiteWords * i + 1];
        if (ref >= n_ref) return fail(BMG_ERR_ARG, "bmg_call: site %llu names reference %u, bmg_begin was given %u", (unsigned long long)i, ref, n_ref);
        if (pos >= c->ref_len[ref])
            return fail(BMG_ERR_ARG, "bmg_call: site %llu lies at base %u of reference %u, which has %u", (unsigned long long)i, pos, ref, c->ref_len[ref]);
    }
    c->ms_call = 0.f;
    if (n_sites == 0) return BMG_OK;
    const uint64_t n_records = 0, n_bytes = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMG_NEED(c->sites.need((size_t)n_sites * bmg::kSiteWords), n_sites * bmg::kSiteWords * 4, "the sites");
    BMG_NEED(c->calls.need((size_t)n_sites * bmg::kCallWords), n_sites * bmg::kCallWords * 4, "the calls");
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->sites.p, sites, (size_t)n_sites * bmg::kSiteWords * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmg::call_kernel, dim3((uint32_t)((n_sites + bmg::kThreads - 1) / bmg::kThreads)), dim3(bmg::kThreads), 0, s, c->sites.p, n_sites,
                       c->cell.p, c->d_ref_len.p, c->d_ref_base.p, n_ref, c->pr.prior, c->calls.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipMemcpyAsync(out, c->calls.p, (size_t)n_sites * bmg::kCallWords * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&c->ms_call, c->ev[0], c->ev[1]));
    return BMG_OK;
}

int bmg_cells_at(bmg_ctx *c, uint32_t ref, uint32_t start, uint32_t count, uint64_t *out) {
    if (count && !out) return fail(BMG_ERR_ARG, "bmg_cells_at: null argument");
    if (!c) return fail(BMG_ERR_ARG, "bmg_cells_at: null context");
    if (!c->begun) return fail(BMG_ERR_ARG, "bmg_cells_at: no bmg_begin before it");
    if (ref >= c->ref_len.size()) return fail(BMG_ERR_ARG, "bmg_cells_at: reference %u of %zu", ref, c->ref_len.size());
    if ((uint64_t)start + count > c->ref_len[ref])
        return fail(BMG_ERR_ARG, "bmg_cells_at: bases %u .. %u + %u asked for, reference %u has %u", start, start, count, ref, c->ref_len[ref]);
    if (count == 0) return BMG_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->cell.p + (c->ref_base[ref] + start) * bmg::kCells, (size_t)count * bmg::kCells * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMG_OK;
}

int bmg_last_stats(bmg_ctx *c, float *ms_add, float *ms_call) {
    if (!c) return fail(BMG_ERR_ARG, "bmg_last_stats: null argument");
    if (ms_add) *ms_add = c->ms_add;
    if (ms_call) *ms_call = c->ms_call;
    return BMG_OK;
}

}  // extern "C"
