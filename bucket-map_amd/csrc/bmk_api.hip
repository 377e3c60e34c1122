// bmk_api.hip -- host side of the read-backed phaser (include/bmk.h): the argument checks, the choice of the phase sites among
// the calls, buffers, the launches of bmk_kernels.hip.h and the downloads.  A bmk_ctx owns its stream and every buffer; the
// stream of records is uploaded per bmk_add into a buffer of its own, as bmb_api.hip does.
#include "../../include/bmk.h"

#include "bm_hip_util.h"
#include "bmk_kernels.hip.h"
#include "bms_ctx.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMK_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMK_OK == BMS_OK && BMK_ERR_ARG == BMS_ERR_ARG && BMK_ERR_HIP == BMS_ERR_HIP, "bmk.h and bms.h must share their status codes");
static_assert(BMK_CALL_WORDS == bmk::kCallWords && BMK_OUT_WORDS == bmk::kOutWords && BMK_N_STATS == bmk::kStats && BMK_MAX_REACH == bmk::kMaxReach &&
                  BMK_PHASED == bmk::kPhased && BMK_ROOT == bmk::kRoot,
              "bmk.h and bmk_kernels.hip.h disagree");

struct bmk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool begun = false, finished = false;
    std::vector<uint32_t> ref_len;
    std::vector<uint64_t> ref_base;         // n_ref + 1: reference r has the slots ref_base[r] .. ref_base[r + 1] - 1
    bmk::params pr{0, 13, 2, 800000, 4};
    uint64_t n_sites = 0;                   // H
    DevBuf<uint8_t> in, skip;
    DevBuf<uint64_t> rec_offset, d_ref_base;
    DevBuf<uint32_t> d_ref_len, slot, link, up[2], has_child, out;
    DevBuf<uint4> meta, chosen;
    DevBuf<unsigned long long> stats;       // BMK_N_STATS; [3] is what the adds count
    float ms_add = 0.f, ms_finish = 0.f;
};

namespace {

constexpr uint64_t kMaxBases = (uint64_t{1} << 32) - (uint64_t{1} << 20);   // bmp_begin's
constexpr uint64_t kMaxSites = uint64_t{1} << 31;

#define BMK_NEED(call, bytes, what)                                                                                            \
    do {                                                                                                                       \
        if ((call) != hipSuccess) {                                                                                            \
            (void)hipGetLastError();                                                                                           \
            size_t free_b = 0, total_b = 0;                                                                                    \
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = 0;                                          \
            return fail(BMK_ERR_HIP, "cannot allocate %llu bytes for %s (%llu phase sites with %u x 4 counters each, %llu records, %llu stream bytes; " \
                        "%llu of %llu bytes of device memory are free)",                                                       \
                        (unsigned long long)(bytes), what, (unsigned long long)n_sites, c->pr.reach, (unsigned long long)n_records, \
                        (unsigned long long)n_bytes, (unsigned long long)free_b, (unsigned long long)total_b);                 \
        }                                                                                                                      \
    } while (0)

// what bmk_add checks of the records beyond bms_check_stream, without a context: bmp_add's checks
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
            return fail(BMK_ERR_ARG, "bmk_add: the fields of record %llu take %llu bytes and do not fit its %llu", (unsigned long long)i,
                        (unsigned long long)need, (unsigned long long)length);
        uint64_t query = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            uint32_t c;
            std::memcpy(&c, r + 36 + r[12] + 4ull * k, 4);
            const uint32_t op = c & 15u;
            if (op > 8) return fail(BMK_ERR_ARG, "bmk_add: op %u of record %llu has the code %u, a CIGAR op is 0 .. 8", k, (unsigned long long)i, op);
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
        }
        if (n_cigar && l_seq && query != l_seq)
            return fail(BMK_ERR_ARG, "bmk_add: the CIGAR of record %llu takes %llu query bases, its l_seq is %u", (unsigned long long)i,
                        (unsigned long long)query, l_seq);
    }
    return BMK_OK;
}

uint32_t grid_of(uint64_t n) { return (uint32_t)((n + bmk::kThreads - 1) / bmk::kThreads); }

}  // namespace

extern "C" {

const char *bmk_last_error(void) { return g_err; }

int bmk_create(int32_t device, bmk_ctx **out) {
    if (!out) return fail(BMK_ERR_ARG, "bmk_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMK_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    bmk_ctx *c = new bmk_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        bmk_destroy(c);
        return fail(BMK_ERR_HIP, "bmk_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMK_OK;
}

void bmk_destroy(bmk_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->in.release(), c->skip.release(), c->rec_offset.release(), c->d_ref_base.release(), c->meta.release(), c->chosen.release(), c->stats.release();
    for (DevBuf<uint32_t> *b : {&c->d_ref_len, &c->slot, &c->link, &c->up[0], &c->up[1], &c->has_child, &c->out}) b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmk_begin(bmk_ctx *c, const uint32_t *ref_len, uint32_t n_ref, const uint32_t *params, const uint32_t *calls, uint64_t n_calls, uint64_t *out_n_sites) {
    if (!ref_len || !params || (n_calls && !calls)) return fail(BMK_ERR_ARG, "bmk_begin: null argument");
    if (n_ref == 0) return fail(BMK_ERR_ARG, "bmk_begin: no reference (n_ref is 0)");
    uint64_t bases = 0;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (ref_len[r] == 0) return fail(BMK_ERR_ARG, "bmk_begin: reference %u has the length 0", r);
        bases += ref_len[r];
    }
    if (bases > kMaxBases || bases + n_ref > 0xFFFFFFFEull)
        return fail(BMK_ERR_ARG, "bmk_begin: %llu bases in %u references, at most 2^32 - 2^20 bases (and 2^32 - 2 with one more per reference) in one context",
                    (unsigned long long)bases, n_ref);
    const bmk::params pr{params[BMK_MIN_MAPQ], params[BMK_MIN_BQ], params[BMK_MIN_LINKS], params[BMK_MIN_FRAC_PPM], params[BMK_REACH]};
    if (pr.reach < 1 || pr.reach > BMK_MAX_REACH) return fail(BMK_ERR_ARG, "bmk_begin: reach is %u, it is 1 .. 8", pr.reach);
    if (pr.min_links == 0) return fail(BMK_ERR_ARG, "bmk_begin: min_links is 0, it is at least 1");
    if (pr.min_frac_ppm < 500001 || pr.min_frac_ppm > 1000000)
        return fail(BMK_ERR_ARG, "bmk_begin: min_frac_ppm is %u, it is 500001 .. 1000000", pr.min_frac_ppm);
    std::vector<uint64_t> ref_base((size_t)n_ref + 1, 0);
    for (uint32_t r = 0; r < n_ref; r++) ref_base[r + 1] = ref_base[r] + ref_len[r];
    std::vector<uint32_t> slot;
    std::vector<uint4> meta;
    for (uint64_t i = 0; i < n_calls; i++) {
        const uint32_t *w = calls + bmk::kCallWords * i;
        if (!(w[3] & bmk::kVariant) || w[4] == w[5]) continue;
        if (w[0] >= n_ref) return fail(BMK_ERR_ARG, "bmk_begin: call %llu names reference %u, there are %u", (unsigned long long)i, w[0], n_ref);
        if (w[1] >= ref_len[w[0]])
            return fail(BMK_ERR_ARG, "bmk_begin: call %llu lies at base %u of reference %u, which has %u", (unsigned long long)i, w[1], w[0], ref_len[w[0]]);
        if (w[4] > 3 || w[5] > 3) return fail(BMK_ERR_ARG, "bmk_begin: call %llu has the letters %u and %u, each is 0 .. 3", (unsigned long long)i, w[4], w[5]);
        const uint32_t at = (uint32_t)(ref_base[w[0]] + w[1]);   // below 2^32: the bases are
        if (!slot.empty() && at <= slot.back())
            return fail(BMK_ERR_ARG, "bmk_begin: call %llu (reference %u, base %u) does not lie behind the phase site before it: the calls ascend", (unsigned long long)i,
                        w[0], w[1]);
        if (slot.size() == kMaxSites - 1) return fail(BMK_ERR_ARG, "bmk_begin: 2^31 phase sites or more");   // this one would be the 2^31st: H is at most 2^31 - 1
        if (i > 0xFFFFFFFFull) return fail(BMK_ERR_ARG, "bmk_begin: the phase site at call %llu, a call's index is below 2^32", (unsigned long long)i);
        slot.push_back(at);
        meta.push_back(make_uint4(w[0], w[1], (uint32_t)i, w[4] | w[5] << 4));
    }
    if (!c) return fail(BMK_ERR_ARG, "bmk_begin: null context");
    c->begun = c->finished = false;
    c->ms_add = c->ms_finish = 0.f;
    c->pr = pr;
    c->ref_len.assign(ref_len, ref_len + n_ref);
    c->ref_base = ref_base;
    c->n_sites = slot.size();
    if (out_n_sites) *out_n_sites = c->n_sites;
    const uint64_t n_sites = c->n_sites, n_records = 0, n_bytes = 0;
    if (n_sites) {
        const size_t H = (size_t)n_sites, n_link = H * pr.reach * 4;
        HIP_TRY(hipSetDevice(c->device));
        BMK_NEED(c->slot.need(H), n_sites * 4, "the site slots");
        BMK_NEED(c->meta.need(H), n_sites * 16, "the site data");
        BMK_NEED(c->link.need(n_link), (uint64_t)n_link * 4, "the link counters");
        BMK_NEED(c->stats.need(bmk::kStats), bmk::kStats * 8ull, "the sums");
        BMK_NEED(c->d_ref_len.need(n_ref), (uint64_t)n_ref * 4, "the reference lengths");
        BMK_NEED(c->d_ref_base.need((size_t)n_ref + 1), ((uint64_t)n_ref + 1) * 8, "the reference starts");
        HIP_TRY(hipMemcpyAsync(c->slot.p, slot.data(), H * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->meta.p, meta.data(), H * 16, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_ref_len.p, c->ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_ref_base.p, c->ref_base.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(c->link.p, 0, n_link * 4, c->stream));
        HIP_TRY(hipMemsetAsync(c->stats.p, 0, bmk::kStats * 8, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));        // slot and meta leave the scope
    }
    c->begun = true;
    return BMK_OK;
}

int bmk_add(bmk_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip) {
    if (!rec_offset || (n_bytes && !in)) return fail(BMK_ERR_ARG, "bmk_add: null argument");
    if (const int rc = bms_check_stream("bmk_add", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_records(in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMK_ERR_ARG, "bmk_add: null context");
    if (!c->begun) return fail(BMK_ERR_ARG, "bmk_add: no bmk_begin before it");
    if (c->finished) return fail(BMK_ERR_ARG, "bmk_add: bmk_finish has run, the next is bmk_begin");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    for (uint64_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        int32_t ref;
        std::memcpy(&ref, r + 4, 4);
        if (ref >= 0 && (uint32_t)ref >= n_ref && !(r[18] & 4u))
            return fail(BMK_ERR_ARG, "bmk_add: record %llu names reference %d, bmk_begin was given %u", (unsigned long long)i, ref, n_ref);
    }
    if (n_records == 0 || c->n_sites == 0) return BMK_OK;
    const uint32_t n = (uint32_t)n_records;
    const uint64_t n_sites = c->n_sites;
    HIP_TRY(hipSetDevice(c->device));
    BMK_NEED(c->in.need((size_t)n_bytes + 16), n_bytes + 16, "the stream");   // the room bmp_add documents
    BMK_NEED(c->rec_offset.need((size_t)n + 1), ((uint64_t)n + 1) * 8, "the record offsets");
    if (skip) BMK_NEED(c->skip.need(n), (uint64_t)n, "the skip bytes");
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_offset.p, rec_offset, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    if (skip) HIP_TRY(hipMemcpyAsync(c->skip.p, skip, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmk::add_kernel, dim3(grid_of(n)), dim3(bmk::kThreads), 0, s, c->in.p, c->rec_offset.p, n, skip ? c->skip.p : nullptr, c->d_ref_len.p,
                       c->d_ref_base.p, n_ref, c->pr, c->slot.p, c->meta.p, (uint32_t)n_sites, c->link.p, c->stats.p + BMK_S_OBSERVATIONS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->ms_add += ms;
    return BMK_OK;
}

int bmk_finish(bmk_ctx *c, uint64_t *out_stats) {
    if (!c) return fail(BMK_ERR_ARG, "bmk_finish: null context");
    if (!c->begun) return fail(BMK_ERR_ARG, "bmk_finish: no bmk_begin before it");
    if (c->finished) return fail(BMK_ERR_ARG, "bmk_finish: it has run already, the next is bmk_begin");
    c->ms_finish = 0.f;
    uint64_t stats[BMK_N_STATS] = {c->n_sites, 0, 0, 0};
    if (c->n_sites) {
        const uint64_t n_sites = c->n_sites, n_records = 0, n_bytes = 0;
        const uint32_t H = (uint32_t)n_sites, grid = grid_of(H);
        HIP_TRY(hipSetDevice(c->device));
        BMK_NEED(c->up[0].need(H), n_sites * 4, "the parents");
        BMK_NEED(c->up[1].need(H), n_sites * 4, "the parents");
        BMK_NEED(c->chosen.need(H), n_sites * 16, "the parent links");
        BMK_NEED(c->has_child.need(H), n_sites * 4, "the root marks");
        BMK_NEED(c->out.need((size_t)H * bmk::kOutWords), n_sites * bmk::kOutWords * 4, "the output");
        hipStream_t s = c->stream;
        HIP_TRY(hipMemsetAsync(c->has_child.p, 0, (size_t)H * 4, s));
        HIP_TRY(hipEventRecord(c->ev[0], s));
        hipLaunchKernelGGL(bmk::pick_kernel, dim3(grid), dim3(bmk::kThreads), 0, s, c->meta.p, c->link.p, H, c->pr, c->up[0].p, c->chosen.p);
        uint32_t rounds = 1;                             // the smallest with 2^rounds >= max(H, 2): it depends on H alone
        while ((uint64_t{1} << rounds) < n_sites) rounds++;
        int at = 0;
        for (uint32_t k = 0; k < rounds; k++, at ^= 1)
            hipLaunchKernelGGL(bmk::jump_kernel, dim3(grid), dim3(bmk::kThreads), 0, s, c->up[at].p, c->up[at ^ 1].p, H);
        hipLaunchKernelGGL(bmk::mark_kernel, dim3(grid), dim3(bmk::kThreads), 0, s, c->up[at].p, H, c->has_child.p);
        hipLaunchKernelGGL(bmk::out_kernel, dim3(grid), dim3(bmk::kThreads), 0, s, c->meta.p, c->up[at].p, c->chosen.p, c->has_child.p, H, c->out.p, c->stats.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev[1], s));
        unsigned long long got[BMK_N_STATS];
        HIP_TRY(hipMemcpyAsync(got, c->stats.p, sizeof got, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipEventElapsedTime(&c->ms_finish, c->ev[0], c->ev[1]));
        stats[BMK_S_PHASED] = got[BMK_S_PHASED], stats[BMK_S_BLOCKS] = got[BMK_S_BLOCKS], stats[BMK_S_OBSERVATIONS] = got[BMK_S_OBSERVATIONS];
    }
    c->finished = true;
    if (out_stats) std::memcpy(out_stats, stats, sizeof stats);
    return BMK_OK;
}

int bmk_phase(bmk_ctx *c, uint64_t first, uint64_t count, uint32_t *out) {
    if (count && !out) return fail(BMK_ERR_ARG, "bmk_phase: null argument");
    if (!c) return fail(BMK_ERR_ARG, "bmk_phase: null context");
    if (!c->begun || !c->finished) return fail(BMK_ERR_ARG, "bmk_phase: no bmk_finish before it");
    if (first > c->n_sites || count > c->n_sites - first)
        return fail(BMK_ERR_ARG, "bmk_phase: sites %llu .. %llu + %llu asked for, there are %llu", (unsigned long long)first, (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)c->n_sites);
    if (count == 0) return BMK_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->out.p + first * bmk::kOutWords, (size_t)count * bmk::kOutWords * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMK_OK;
}

int bmk_links(bmk_ctx *c, uint64_t first, uint64_t count, uint32_t *out) {
    if (count && !out) return fail(BMK_ERR_ARG, "bmk_links: null argument");
    if (!c) return fail(BMK_ERR_ARG, "bmk_links: null context");
    if (!c->begun) return fail(BMK_ERR_ARG, "bmk_links: no bmk_begin before it");
    if (first > c->n_sites || count > c->n_sites - first)
        return fail(BMK_ERR_ARG, "bmk_links: sites %llu .. %llu + %llu asked for, there are %llu", (unsigned long long)first, (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)c->n_sites);
    if (count == 0) return BMK_OK;
    const size_t per = (size_t)c->pr.reach * 4;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->link.p + first * per, (size_t)count * per * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMK_OK;
}

int bmk_last_stats(bmk_ctx *c, float *ms_add, float *ms_finish) {
    if (!c) return fail(BMK_ERR_ARG, "bmk_last_stats: null argument");
    if (ms_add) *ms_add = c->ms_add;
    if (ms_finish) *ms_finish = c->ms_finish;
    return BMK_OK;
}

}  // extern "C"
