// bmc_api.hip -- host side of the coverage counter (include/bmc.h): the argument checks, buffers, the launches of
// bmc_kernels.hip.h and the downloads.  A bmc_ctx owns its stream and every buffer; the stream of records is uploaded per
// bmc_add into a buffer of its own (the sorter's copy belongs to another context and is gone when the file is written).
#include "../../include/bmc.h"

#include "bm_hip_util.h"
#include "bm_scan.hip.h"
#include "bmc_kernels.hip.h"
#include "bms_ctx.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMC_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMC_OK == BMS_OK && BMC_ERR_ARG == BMS_ERR_ARG && BMC_ERR_HIP == BMS_ERR_HIP, "bmc.h and bms.h must share their status codes");
static_assert(BMC_N_STATS == bmc::kStats, "bmc.h and bmc_kernels.hip.h disagree");

struct bmc_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    enum { kIdle, kBegun, kFinished } state = kIdle;
    std::vector<uint32_t> ref_len;
    std::vector<uint64_t> ref_base;         // n_ref + 1: reference r has the slots ref_base[r] .. ref_base[r + 1] - 1
    uint64_t n_slots = 0, n_runs = 0;
    DevBuf<uint8_t> in, skip;
    DevBuf<uint64_t> rec_offset, d_ref_base;
    DevBuf<uint32_t> d_ref_len, diff, depth, scan_tmp, tile_count, tile_rank, runs;
    DevBuf<unsigned long long> stats;
    float ms_add = 0.f, ms_finish = 0.f;
};

namespace {

constexpr uint64_t kMaxBases = (uint64_t{1} << 32) - (uint64_t{1} << 20);

#define BMC_NEED(call, bytes, what)                                                                                            \
    do {                                                                                                                       \
        if ((call) != hipSuccess) {                                                                                            \
            (void)hipGetLastError();                                                                                           \
            return fail(BMC_ERR_HIP, "cannot allocate %llu bytes for %s (%llu slots of %zu references, %llu records, %llu stream bytes)", \
                        (unsigned long long)(bytes), what, (unsigned long long)c->n_slots, c->ref_len.size(), (unsigned long long)n_records, \
                        (unsigned long long)n_bytes);                                                                          \
        }                                                                                                                      \
    } while (0)

// what bmc_add checks of the records beyond bms_check_stream, without a context
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
            return fail(BMC_ERR_ARG, "bmc_add: the fields of record %llu take %llu bytes and do not fit its %llu", (unsigned long long)i,
                        (unsigned long long)need, (unsigned long long)length);
        uint64_t query = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            uint32_t c;
            std::memcpy(&c, r + 36 + r[12] + 4ull * k, 4);
            const uint32_t op = c & 15u;
            if (op > 8) return fail(BMC_ERR_ARG, "bmc_add: op %u of record %llu has the code %u, a CIGAR op is 0 .. 8", k, (unsigned long long)i, op);
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
        }
        if (n_cigar && l_seq && query != l_seq)
            return fail(BMC_ERR_ARG, "bmc_add: the CIGAR of record %llu takes %llu query bases, its l_seq is %u", (unsigned long long)i,
                        (unsigned long long)query, l_seq);
    }
    return BMC_OK;
}

}  // namespace

extern "C" {

const char *bmc_last_error(void) { return g_err; }

int bmc_create(int32_t device, bmc_ctx **out) {
    if (!out) return fail(BMC_ERR_ARG, "bmc_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMC_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    bmc_ctx *c = new bmc_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        bmc_destroy(c);
        return fail(BMC_ERR_HIP, "bmc_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMC_OK;
}

void bmc_destroy(bmc_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->in.release(), c->skip.release(), c->rec_offset.release(), c->d_ref_base.release(), c->stats.release();
    for (DevBuf<uint32_t> *b : {&c->d_ref_len, &c->diff, &c->depth, &c->scan_tmp, &c->tile_count, &c->tile_rank, &c->runs}) b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmc_begin(bmc_ctx *c, const uint32_t *ref_len, uint32_t n_ref) {
    if (!ref_len) return fail(BMC_ERR_ARG, "bmc_begin: null argument");
    if (n_ref == 0) return fail(BMC_ERR_ARG, "bmc_begin: no reference (n_ref is 0)");
    uint64_t bases = 0;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (ref_len[r] == 0) return fail(BMC_ERR_ARG, "bmc_begin: reference %u has the length 0", r);
        bases += ref_len[r];
    }
    if (bases > kMaxBases || bases + n_ref > 0xFFFFFFFEull)
        return fail(BMC_ERR_ARG, "bmc_begin: %llu bases in %u references, at most 2^32 - 2^20 bases (and 2^32 - 2 slots) in one context",
                    (unsigned long long)bases, n_ref);
    if (!c) return fail(BMC_ERR_ARG, "bmc_begin: null context");
    c->state = bmc_ctx::kIdle;
    c->ms_add = c->ms_finish = 0.f;
    c->n_runs = 0;
    c->ref_len.assign(ref_len, ref_len + n_ref);
    c->ref_base.assign((size_t)n_ref + 1, 0);
    for (uint32_t r = 0; r < n_ref; r++) c->ref_base[r + 1] = c->ref_base[r] + ref_len[r] + 1;
    c->n_slots = c->ref_base[n_ref];
    const uint64_t n_slots = c->n_slots, n_tiles = (n_slots + bmc::kTile - 1) / bmc::kTile, n_records = 0, n_bytes = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMC_NEED(c->diff.need_exact(n_slots), n_slots * 4, "the differences");
    BMC_NEED(c->depth.need_exact(n_slots + 1), (n_slots + 1) * 4, "the depths");
    BMC_NEED(c->scan_tmp.need(bmscan::tmp_elems(n_slots)), bmscan::tmp_elems(n_slots) * 4, "the scan of the differences");
    BMC_NEED(c->tile_count.need(n_tiles), n_tiles * 4, "the tiles' run counts");
    BMC_NEED(c->tile_rank.need(n_tiles + 1), (n_tiles + 1) * 4, "the tiles' run ranks");
    BMC_NEED(c->d_ref_len.need(n_ref), (uint64_t)n_ref * 4, "the reference lengths");
    BMC_NEED(c->d_ref_base.need((size_t)n_ref + 1), ((uint64_t)n_ref + 1) * 8, "the reference bases");
    BMC_NEED(c->stats.need((size_t)n_ref * bmc::kStats), (uint64_t)n_ref * bmc::kStats * 8, "the reference sums");
    HIP_TRY(hipMemcpyAsync(c->d_ref_len.p, c->ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_ref_base.p, c->ref_base.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->diff.p, 0, (size_t)n_slots * 4, c->stream));
    HIP_TRY(hipMemsetAsync(c->stats.p, 0, (size_t)n_ref * bmc::kStats * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->state = bmc_ctx::kBegun;
    return BMC_OK;
}

int bmc_add(bmc_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip) {
    if (!rec_offset || (n_bytes && !in)) return fail(BMC_ERR_ARG, "bmc_add: null argument");
    if (const int rc = bms_check_stream("bmc_add", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_records(in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMC_ERR_ARG, "bmc_add: null context");
    if (c->state != bmc_ctx::kBegun) return fail(BMC_ERR_ARG, "bmc_add: no bmc_begin before it, or a bmc_finish since");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    for (uint64_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        int32_t ref;
        std::memcpy(&ref, r + 4, 4);
        if (ref >= 0 && (uint32_t)ref >= n_ref && !(r[18] & 4u))
            return fail(BMC_ERR_ARG, "bmc_add: record %llu names reference %d, bmc_begin was given %u", (unsigned long long)i, ref, n_ref);
    }
    if (n_records == 0) return BMC_OK;
    const uint32_t n = (uint32_t)n_records;
    HIP_TRY(hipSetDevice(c->device));
    BMC_NEED(c->in.need((size_t)n_bytes + 16), n_bytes + 16, "the stream");   // span_sum reads whole aligned words
    BMC_NEED(c->rec_offset.need((size_t)n + 1), ((uint64_t)n + 1) * 8, "the record offsets");
    if (skip) BMC_NEED(c->skip.need(n), (uint64_t)n, "the skip bytes");
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_offset.p, rec_offset, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    if (skip) HIP_TRY(hipMemcpyAsync(c->skip.p, skip, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmc::blocks_kernel, dim3((n + bmc::kThreads - 1) / bmc::kThreads), dim3(bmc::kThreads), 0, s, c->in.p, c->rec_offset.p, n,
                       skip ? c->skip.p : nullptr, c->d_ref_len.p, c->d_ref_base.p, n_ref, c->diff.p, c->stats.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->ms_add += ms;
    return BMC_OK;
}

int bmc_finish(bmc_ctx *c, uint64_t *out_n_runs, uint64_t *out_ref_stats) {
    if (!out_n_runs || !out_ref_stats) return fail(BMC_ERR_ARG, "bmc_finish: null argument");
    if (!c) return fail(BMC_ERR_ARG, "bmc_finish: null context");
    if (c->state != bmc_ctx::kBegun) return fail(BMC_ERR_ARG, "bmc_finish: no bmc_begin before it, or a second bmc_finish");
    const uint32_t n_ref = (uint32_t)c->ref_len.size();
    const uint64_t n_slots = c->n_slots, n_tiles = (n_slots + bmc::kTile - 1) / bmc::kTile, n_records = 0, n_bytes = 0;
    hipStream_t s = c->stream;
    HIP_TRY(hipSetDevice(c->device));
    BMC_NEED(c->scan_tmp.need(bmscan::tmp_elems(n_slots)), bmscan::tmp_elems(n_slots) * 4, "the scan of the differences");
    HIP_TRY(hipEventRecord(c->ev[0], s));
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->diff.p, c->depth.p, n_slots, c->scan_tmp.p, s));
    hipLaunchKernelGGL(bmc::runs_count_kernel, dim3((uint32_t)n_tiles), dim3(bmc::kThreads), 0, s, c->depth.p, n_slots, c->d_ref_base.p, n_ref,
                       c->tile_count.p, c->stats.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->tile_count.p, c->tile_rank.p, n_tiles, c->scan_tmp.p, s));
    uint32_t n_runs = 0;
    HIP_TRY(hipMemcpyAsync(&n_runs, c->tile_rank.p + n_tiles, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_runs > n_slots) return fail(BMC_ERR_HIP, "bmc_finish: %u runs counted over %llu slots", n_runs, (unsigned long long)n_slots);
    BMC_NEED(c->runs.need((size_t)n_runs * 4), (uint64_t)n_runs * 16, "the runs");
    if (n_runs) {
        hipLaunchKernelGGL(bmc::runs_emit_kernel, dim3((uint32_t)n_tiles), dim3(bmc::kThreads), 0, s, c->depth.p, n_slots, c->d_ref_base.p, n_ref,
                           c->tile_rank.p, n_runs, c->runs.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipMemcpyAsync(out_ref_stats, c->stats.p, (size_t)n_ref * bmc::kStats * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&c->ms_finish, c->ev[0], c->ev[1]));
    c->n_runs = n_runs;
    *out_n_runs = n_runs;
    c->state = bmc_ctx::kFinished;
    return BMC_OK;
}

int bmc_runs(bmc_ctx *c, uint64_t first, uint64_t count, uint32_t *out) {
    if (count && !out) return fail(BMC_ERR_ARG, "bmc_runs: null argument");
    if (!c) return fail(BMC_ERR_ARG, "bmc_runs: null context");
    if (c->state != bmc_ctx::kFinished) return fail(BMC_ERR_ARG, "bmc_runs: no bmc_finish before it");
    if (first > c->n_runs || count > c->n_runs - first)
        return fail(BMC_ERR_ARG, "bmc_runs: runs %llu .. %llu + %llu asked for, there are %llu", (unsigned long long)first, (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)c->n_runs);
    if (count == 0) return BMC_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->runs.p + 4 * first, (size_t)count * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMC_OK;
}

int bmc_depth_at(bmc_ctx *c, uint32_t ref, uint32_t start, uint32_t count, uint32_t *out) {
    if (count && !out) return fail(BMC_ERR_ARG, "bmc_depth_at: null argument");
    if (!c) return fail(BMC_ERR_ARG, "bmc_depth_at: null context");
    if (c->state != bmc_ctx::kFinished) return fail(BMC_ERR_ARG, "bmc_depth_at: no bmc_finish before it");
    if (ref >= c->ref_len.size()) return fail(BMC_ERR_ARG, "bmc_depth_at: reference %u of %zu", ref, c->ref_len.size());
    if ((uint64_t)start + count > c->ref_len[ref])
        return fail(BMC_ERR_ARG, "bmc_depth_at: bases %u .. %u + %u asked for, reference %u has %u", start, start, count, ref, c->ref_len[ref]);
    if (count == 0) return BMC_OK;
    HIP_TRY(hipSetDevice(c->device));
    // depth[i + 1] is the depth of slot i
    HIP_TRY(hipMemcpyAsync(out, c->depth.p + c->ref_base[ref] + start + 1, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMC_OK;
}

int bmc_last_stats(bmc_ctx *c, float *ms_add, float *ms_finish) {
    if (!c) return fail(BMC_ERR_ARG, "bmc_last_stats: null argument");
    if (ms_add) *ms_add = c->ms_add;
    if (ms_finish) *ms_finish = c->ms_finish;
    return BMC_OK;
}

}  // extern "C"
