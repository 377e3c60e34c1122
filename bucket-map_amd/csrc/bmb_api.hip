// bmb_api.hip -- host side of the strand-bias and mapping-quality annotator (include/bmb.h): the two tables, the argument
// checks, buffers, the launches of bmb_kernels.hip.h and the downloads.  A bmb_ctx owns its stream and every buffer; the
// stream of records is uploaded per bmb_add into a buffer of its own, as bmg_api.hip does, and the calls of a bmb_annotate per
// call.
#include "../../include/bmb.h"

#include <math.h>

#include "bm_hip_util.h"
#include "bmb_kernels.hip.h"
#include "bms_ctx.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMB_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMB_OK == BMS_OK && BMB_ERR_ARG == BMS_ERR_ARG && BMB_ERR_HIP == BMS_ERR_HIP, "bmb.h and bms.h must share their status codes");
static_assert(BMB_N_STRAND_CELLS == bmb::kStrandCells && BMB_CALL_WORDS == bmb::kCallWords && BMB_OUT_WORDS == bmb::kOutWords && BMB_N_LF == bmb::kNLf &&
                  BMB_N_E == bmb::kNE && BMB_FS_CAP == bmb::kFsCap && BMB_FS_MAX_N == bmb::kFsMaxN && BMB_ANNOTATED == bmb::kAnnotated &&
                  BMB_NO_FS == bmb::kNoFs,
              "bmb.h and bmb_kernels.hip.h disagree");

struct bmb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool begun = false;
    std::vector<uint32_t> ref_len;
    std::vector<uint64_t> ref_base;         // n_ref + 1: reference r has the slots ref_base[r] .. ref_base[r + 1] - 1
    bmb::params pr{0, 13};
    uint64_t n_slots = 0;
    DevBuf<uint8_t> in, skip;
    DevBuf<uint64_t> rec_offset, d_ref_base;
    DevBuf<uint32_t> d_ref_len, calls, out, lf;
    DevBuf<unsigned long long> strand, mapq, e;
    float ms_add = 0.f, ms_annotate = 0.f;
};

namespace {

constexpr uint64_t kMaxBases = (uint64_t{1} << 32) - (uint64_t{1} << 20);   // bmp_begin's
constexpr uint64_t kMaxCalls = uint64_t{1} << 31;

#define BMB_NEED(call, bytes, what)                                                                                            \
    do {                                                                                                                       \
        if ((call) != hipSuccess) {                                                                                            \
            (void)hipGetLastError();                                                                                           \
            size_t free_b = 0, total_b = 0;                                                                                    \
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = 0;                                          \
            return fail(BMB_ERR_HIP,                                                                                           \
                        "cannot allocate %llu bytes for %s (%llu positions of %zu references at 40 bytes each, %llu records, %llu stream bytes, " \
                        "%llu calls; %llu of %llu bytes of device memory are free)",                                           \
                        (unsigned long long)(bytes), what, (unsigned long long)c->n_slots, c->ref_len.size(), (unsigned long long)n_records, \
                        (unsigned long long)n_bytes, (unsigned long long)n_calls, (unsigned long long)free_b, (unsigned long long)total_b); \
        }                                                                                                                      \
    } while (0)

// what bmb_add checks of the records beyond bms_check_stream, without a context: bmp_add's checks
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
            return fail(BMB_ERR_ARG, "bmb_add: the fields of record %llu take %llu bytes and do not fit its %llu", (unsigned long long)i,
                        (unsigned long long)need, (unsigned long long)length);
        uint64_t query = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            uint32_t c;
            std::memcpy(&c, r + 36 + r[12] + 4ull * k, 4);
            const uint32_t op = c & 15u;
            if (op > 8) return fail(BMB_ERR_ARG, "bmb_add: op %u of record %llu has the code %u, a CIGAR op is 0 .. 8", k, (unsigned long long)i, op);
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
        }
        if (n_cigar && l_seq && query != l_seq)
            return fail(BMB_ERR_ARG, "bmb_add: the CIGAR of record %llu takes %llu query bases, its l_seq is %u", (unsigned long long)i,
                        (unsigned long long)query, l_seq);
    }
    return BMB_OK;
}

}  // namespace

extern "C" {

const char *bmb_last_error(void) { return g_err; }

int bmb_tables(uint32_t *lf, uint64_t *e) {
    if (!lf || !e) return fail(BMB_ERR_ARG, "bmb_tables: null argument");
    long double acc = 0.0L;                              // log10(n!)
    lf[0] = 0;
    for (uint32_t n = 1; n < bmb::kNLf; n++) {
        acc += log10l((long double)n);
        lf[n] = (uint32_t)llroundl(1000.0L * acc);
    }
    for (uint32_t k = 0; k < bmb::kNE; k++) e[k] = (uint64_t)llroundl(1099511627776.0L * powl(10.0L, -(long double)k / 1000.0L));
    return BMB_OK;
}

int bmb_create(int32_t device, bmb_ctx **out) {
    if (!out) return fail(BMB_ERR_ARG, "bmb_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMB_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    bmb_ctx *c = new bmb_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    std::vector<uint32_t> lf(bmb::kNLf);
    std::vector<uint64_t> et(bmb::kNE);
    (void)bmb_tables(lf.data(), et.data());
    if (e == hipSuccess) e = c->lf.need_exact(bmb::kNLf);
    if (e == hipSuccess) e = c->e.need_exact(bmb::kNE);
    if (e == hipSuccess) e = hipMemcpyAsync(c->lf.p, lf.data(), (size_t)bmb::kNLf * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->e.p, et.data(), (size_t)bmb::kNE * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // lf and et leave the scope
    if (e != hipSuccess) {
        (void)hipGetLastError();
        bmb_destroy(c);
        return fail(BMB_ERR_HIP, "bmb_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMB_OK;
}

void bmb_destroy(bmb_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->in.release(), c->skip.release(), c->rec_offset.release(), c->d_ref_base.release();
    for (DevBuf<uint32_t> *b : {&c->d_ref_len, &c->calls, &c->out, &c->lf}) b->release();
    for (DevBuf<unsigned long long> *b : {&c->strand, &c->mapq, &c->e}) b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmb_begin(bmb_ctx *c, const uint32_t *ref_len, uint32_t n_ref, const uint32_t *params) {
    if (!ref_len || !params) return fail(BMB_ERR_ARG, "bmb_begin: null argument");
    if (n_ref == 0) return fail(BMB_ERR_ARG, "bmb_begin: no reference (n_ref is 0)");
    uint64_t bases = 0;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (ref_len[r] == 0) return fail(BMB_ERR_ARG, "bmb_begin: reference %u has the length 0", r);
        bases += ref_len[r];
    }
    if (bases > kMaxBases || bases + n_ref > 0xFFFFFFFEull)
        return fail(BMB_ERR_ARG, "bmb_begin: %llu bases in %u references, at most 2^32 - 2^20 bases (and 2^32 - 2 with one more per reference) in one context",
                    (unsigned long long)bases, n_ref);
    if (!c) return fail(BMB_ERR_ARG, "bmb_begin: null context");
    c->begun = false;
    c->ms_add = c->ms_annotate = 0.f;
    c->pr = bmb::params{params[BMB_MIN_MAPQ], params[BMB_MIN_BQ]};
    c->ref_len.assign(ref_len, ref_len + n_ref);
    c->ref_base.assign((size_t)n_ref + 1, 0);
    for (uint32_t r = 0; r < n_ref; r++) c->ref_base[r + 1] = c->ref_base[r] + ref_len[r];
    c->n_slots = c->ref_base[n_ref];
    const uint64_t n_slots = c->n_slots, n_records = 0, n_bytes = 0, n_calls = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMB_NEED(c->strand.need_exact((size_t)n_slots * bmb::kStrandCells), n_slots * bmb::kStrandCells * 8, "the strand cells");
    BMB_NEED(c->mapq.need_exact((size_t)n_slots), n_slots * 8, "the mapq cells");
    BMB_NEED(c->d_ref_len.need(n_ref), (uint64_t)n_ref * 4, "the reference lengths");
    BMB_NEED(c->d_ref_base.need((size_t)n_ref + 1), ((uint64_t)n_ref + 1) * 8, "the reference starts");
    HIP_TRY(hipMemcpyAsync(c->d_ref_len.p, c->ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_ref_base.p, c->ref_base.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->strand.p, 0, (size_t)n_slots * bmb::kStrandCells * 8, c->stream));
    HIP_TRY(hipMemsetAsync(c->mapq.p, 0, (size_t)n_slots * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->begun = true;
    return BMB_OK;
}

int bmb_add(bmb_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip) {
    if (!rec_offset || (n_bytes && !in)) return fail(BMB_ERR_ARG, "bmb_add: null argument");
    if (const int rc = bms_check_stream("bmb_add", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_records(in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMB_ERR_ARG, "bmb_add: null context");
    if (!c->begun) return fail(BMB_ERR_ARG, "bmb_add: no bmb_begin before it");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    for (uint64_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        int32_t ref;
        std::memcpy(&ref, r + 4, 4);
        if (ref >= 0 && (uint32_t)ref >= n_ref && !(r[18] & 4u))
            return fail(BMB_ERR_ARG, "bmb_add: record %llu names reference %d, bmb_begin was given %u", (unsigned long long)i, ref, n_ref);
    }
    if (n_records == 0) return BMB_OK;
    const uint32_t n = (uint32_t)n_records;
    const uint64_t n_calls = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMB_NEED(c->in.need((size_t)n_bytes + 16), n_bytes + 16, "the stream");   // bases_shared reads whole aligned words
    BMB_NEED(c->rec_offset.need((size_t)n + 1), ((uint64_t)n + 1) * 8, "the record offsets");
    if (skip) BMB_NEED(c->skip.need(n), (uint64_t)n, "the skip bytes");
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_offset.p, rec_offset, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    if (skip) HIP_TRY(hipMemcpyAsync(c->skip.p, skip, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmb::add_kernel, dim3((n + bmb::kThreads - 1) / bmb::kThreads), dim3(bmb::kThreads), 0, s, c->in.p, c->rec_offset.p, n,
                       skip ? c->skip.p : nullptr, c->d_ref_len.p, c->d_ref_base.p, n_ref, c->pr, c->strand.p, c->mapq.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->ms_add += ms;
    return BMB_OK;
}

int bmb_annotate(bmb_ctx *c, const uint32_t *calls, uint64_t n_calls, uint32_t *out) {
    if (n_calls && (!calls || !out)) return fail(BMB_ERR_ARG, "bmb_annotate: null argument");
    if (n_calls >= kMaxCalls) return fail(BMB_ERR_ARG, "bmb_annotate: %llu calls, fewer than 2^31 are annotated in one go", (unsigned long long)n_calls);
    if (!c) return fail(BMB_ERR_ARG, "bmb_annotate: null context");
    if (!c->begun) return fail(BMB_ERR_ARG, "bmb_annotate: no bmb_begin before it");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    for (uint64_t i = 0; i < n_calls; i++) {
        const uint32_t *w = calls + bmb::kCallWords * i;
        if (!(w[3] & bmb::kVariant)) continue;
        if (w[0] >= n_ref) return fail(BMB_ERR_ARG, "bmb_annotate: call %llu names reference %u, bmb_begin was given %u", (unsigned long long)i, w[0], n_ref);
        if (w[1] >= c->ref_len[w[0]])
            return fail(BMB_ERR_ARG, "bmb_annotate: call %llu lies at base %u of reference %u, which has %u", (unsigned long long)i, w[1], w[0], c->ref_len[w[0]]);
        if (w[2] > 3 || w[4] > 3 || w[5] > 3)
            return fail(BMB_ERR_ARG, "bmb_annotate: call %llu has the reference allele %u and the letters %u and %u, each is 0 .. 3", (unsigned long long)i, w[2],
                        w[4], w[5]);
    }
    c->ms_annotate = 0.f;
    if (n_calls == 0) return BMB_OK;
    const uint64_t n_records = 0, n_bytes = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMB_NEED(c->calls.need((size_t)n_calls * bmb::kCallWords), n_calls * bmb::kCallWords * 4, "the calls");
    BMB_NEED(c->out.need((size_t)n_calls * bmb::kOutWords), n_calls * bmb::kOutWords * 4, "the annotations");
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->calls.p, calls, (size_t)n_calls * bmb::kCallWords * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmb::annotate_kernel, dim3((uint32_t)((n_calls + bmb::kWaves - 1) / bmb::kWaves)), dim3(bmb::kThreads), 0, s, c->calls.p, n_calls,
                       c->strand.p, c->mapq.p, c->d_ref_len.p, c->d_ref_base.p, n_ref, c->lf.p, c->e.p, c->out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipMemcpyAsync(out, c->out.p, (size_t)n_calls * bmb::kOutWords * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&c->ms_annotate, c->ev[0], c->ev[1]));
    return BMB_OK;
}

int bmb_cells_at(bmb_ctx *c, uint32_t ref, uint32_t start, uint32_t count, uint64_t *strand, uint64_t *mapq) {
    if (count && !strand && !mapq) return fail(BMB_ERR_ARG, "bmb_cells_at: null argument");
    if (!c) return fail(BMB_ERR_ARG, "bmb_cells_at: null context");
    if (!c->begun) return fail(BMB_ERR_ARG, "bmb_cells_at: no bmb_begin before it");
    if (ref >= c->ref_len.size()) return fail(BMB_ERR_ARG, "bmb_cells_at: reference %u of %zu", ref, c->ref_len.size());
    if ((uint64_t)start + count > c->ref_len[ref])
        return fail(BMB_ERR_ARG, "bmb_cells_at: bases %u .. %u + %u asked for, reference %u has %u", start, start, count, ref, c->ref_len[ref]);
    if (count == 0) return BMB_OK;
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t first = c->ref_base[ref] + start;
    if (strand) HIP_TRY(hipMemcpyAsync(strand, c->strand.p + first * bmb::kStrandCells, (size_t)count * bmb::kStrandCells * 8, hipMemcpyDeviceToHost, c->stream));
    if (mapq) HIP_TRY(hipMemcpyAsync(mapq, c->mapq.p + first, (size_t)count * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMB_OK;
}

int bmb_last_stats(bmb_ctx *c, float *ms_add, float *ms_annotate) {
    if (!c) return fail(BMB_ERR_ARG, "bmb_last_stats: null argument");
    if (ms_add) *ms_add = c->ms_add;
    if (ms_annotate) *ms_annotate = c->ms_annotate;
    return BMB_OK;
}

}  // extern "C"
