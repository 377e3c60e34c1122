// bmq_api.hip -- host side of the mapping statistics (include/bmq.h): the argument checks, the tables' buffer, the launches of
// bmq_kernels.hip.h and the downloads.  A bmq_ctx owns its stream and every buffer; the stream of records is uploaded per
// bmq_add into a buffer of its own, as bmk_api.hip does.
#include "../../include/bmq.h"

#include "bm_hip_util.h"
#include "bmq_kernels.hip.h"
#include "bms_ctx.hip.h"

#include <cstdlib>

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMQ_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMQ_OK == BMS_OK && BMQ_ERR_ARG == BMS_ERR_ARG && BMQ_ERR_HIP == BMS_ERR_HIP, "bmq.h and bms.h must share their status codes");
static_assert(BMQ_N_TALLIES == bmq::kTallies && BMQ_MAX_LDS_CYCLES == bmq::kMaxLdsCycles, "bmq.h and bmq_kernels.hip.h disagree");

namespace {

constexpr uint32_t kDefaultLdsCycles = 256;              // 79 KB of LDS, two workgroups of 16 waves per CU
constexpr uint64_t kWidth[BMQ_N_TABLES] = {1, 1, 3, 1, 2, 5, 64, 6};

}  // namespace

struct bmq_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool begun = false, finished = false;
    uint32_t n_cu = 1, lds_cycles = kDefaultLdsCycles;   // the window asked for; the one used is min(lds_cycles, C)
    uint32_t C = 0, I = 0;
    uint64_t rows[BMQ_N_TABLES] = {}, at[BMQ_N_TABLES + 1] = {};   // table t: cells[at[t] .. at[t + 1]) behind the tallies
    DevBuf<uint8_t> in, skip;
    DevBuf<uint64_t> rec_offset;
    DevBuf<unsigned long long> cells;                    // the tallies, then the eight tables
    float ms_add = 0.f, ms_finish = 0.f;
};

namespace {

#define BMQ_NEED(call, bytes, what)                                                                                            \
    do {                                                                                                                       \
        if ((call) != hipSuccess) {                                                                                            \
            (void)hipGetLastError();                                                                                           \
            size_t free_b = 0, total_b = 0;                                                                                    \
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = 0;                                          \
            return fail(BMQ_ERR_HIP, "cannot allocate %llu bytes for %s (%u cycles, %u insert sizes, %llu records, %llu stream bytes; " \
                        "%llu of %llu bytes of device memory are free)",                                                       \
                        (unsigned long long)(bytes), what, c->C, c->I, (unsigned long long)n_records, (unsigned long long)n_bytes, \
                        (unsigned long long)free_b, (unsigned long long)total_b);                                              \
        }                                                                                                                      \
    } while (0)

// what bmq_add checks of the records beyond bms_check_stream, without a context: bmp_add's checks
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
            return fail(BMQ_ERR_ARG, "bmq_add: the fields of record %llu take %llu bytes and do not fit its %llu", (unsigned long long)i,
                        (unsigned long long)need, (unsigned long long)length);
        uint64_t query = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            uint32_t c;
            std::memcpy(&c, r + 36 + r[12] + 4ull * k, 4);
            const uint32_t op = c & 15u;
            if (op > 8) return fail(BMQ_ERR_ARG, "bmq_add: op %u of record %llu has the code %u, a CIGAR op is 0 .. 8", k, (unsigned long long)i, op);
            if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
        }
        if (n_cigar && l_seq && query != l_seq)
            return fail(BMQ_ERR_ARG, "bmq_add: the CIGAR of record %llu takes %llu query bases, its l_seq is %u", (unsigned long long)i,
                        (unsigned long long)query, l_seq);
    }
    return BMQ_OK;
}

bmq::state state_of(const bmq_ctx *c) {
    unsigned long long *t = c->cells.p + BMQ_N_TALLIES;
    bmq::state st;
    st.tally = c->cells.p;
    st.mapq = t + c->at[BMQ_T_MAPQ], st.rl = t + c->at[BMQ_T_RL], st.is = t + c->at[BMQ_T_IS], st.gc = t + c->at[BMQ_T_GC], st.id = t + c->at[BMQ_T_ID];
    st.bc = t + c->at[BMQ_T_BC], st.qc = t + c->at[BMQ_T_QC], st.mc = t + c->at[BMQ_T_MC];
    st.C = c->C, st.I = c->I, st.Cw = c->lds_cycles < c->C ? c->lds_cycles : c->C;
    return st;
}

}  // namespace

extern "C" {

const char *bmq_last_error(void) { return g_err; }

int bmq_create(int32_t device, bmq_ctx **out) {
    if (!out) return fail(BMQ_ERR_ARG, "bmq_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMQ_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    int n_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    bmq_ctx *c = new bmq_ctx();
    c->device = device;
    c->n_cu = n_cu > 0 ? (uint32_t)n_cu : 1u;
    if (const char *e = std::getenv("BMQ_LDS_CYCLES")) {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (end != e && *end == 0) c->lds_cycles = v > BMQ_MAX_LDS_CYCLES ? (uint32_t)BMQ_MAX_LDS_CYCLES : (uint32_t)v;
    }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e == hipSuccess)                                 // more than the 64 KB a kernel gets unasked
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(bmq::bases_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(bmq::lds_words(BMQ_MAX_LDS_CYCLES) * 4));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        bmq_destroy(c);
        return fail(BMQ_ERR_HIP, "bmq_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMQ_OK;
}

void bmq_destroy(bmq_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->in.release(), c->skip.release(), c->rec_offset.release(), c->cells.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmq_begin(bmq_ctx *c, const uint32_t *params) {
    if (!params) return fail(BMQ_ERR_ARG, "bmq_begin: null argument");
    const uint32_t C = params[BMQ_MAX_CYCLE], I = params[BMQ_MAX_INSERT];
    if (C < 1 || C > 65535) return fail(BMQ_ERR_ARG, "bmq_begin: max_cycle is %u, it is 1 .. 65535", C);
    if (I < 1 || I > 65535) return fail(BMQ_ERR_ARG, "bmq_begin: max_insert is %u, it is 1 .. 65535", I);
    if (!c) return fail(BMQ_ERR_ARG, "bmq_begin: null context");
    c->begun = c->finished = false;
    c->ms_add = c->ms_finish = 0.f;
    c->C = C, c->I = I;
    const uint64_t rows[BMQ_N_TABLES] = {256, (uint64_t)C + 1, (uint64_t)I + 1, 101, 256, C, C, C};
    for (int t = 0; t < BMQ_N_TABLES; t++) c->rows[t] = rows[t], c->at[t + 1] = c->at[t] + rows[t] * kWidth[t];
    const uint64_t n_cells = BMQ_N_TALLIES + c->at[BMQ_N_TABLES], n_records = 0, n_bytes = 0;
    HIP_TRY(hipSetDevice(c->device));
    BMQ_NEED(c->cells.need((size_t)n_cells), n_cells * 8, "the tallies and tables");
    HIP_TRY(hipMemsetAsync(c->cells.p, 0, (size_t)n_cells * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->begun = true;
    return BMQ_OK;
}

int bmq_add(bmq_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, const uint8_t *skip) {
    if (!rec_offset || (n_bytes && !in)) return fail(BMQ_ERR_ARG, "bmq_add: null argument");
    if (const int rc = bms_check_stream("bmq_add", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_records(in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMQ_ERR_ARG, "bmq_add: null context");
    if (!c->begun) return fail(BMQ_ERR_ARG, "bmq_add: no bmq_begin before it");
    if (c->finished) return fail(BMQ_ERR_ARG, "bmq_add: bmq_finish has run, the next is bmq_begin");
    if (n_records == 0) return BMQ_OK;
    const uint32_t n = (uint32_t)n_records;              // below 2^31: bms_check_stream
    HIP_TRY(hipSetDevice(c->device));
    BMQ_NEED(c->in.need((size_t)n_bytes + 16), n_bytes + 16, "the stream");   // the room bmp_add documents: the kernels read whole words
    BMQ_NEED(c->rec_offset.need((size_t)n + 1), ((uint64_t)n + 1) * 8, "the record offsets");
    if (skip) BMQ_NEED(c->skip.need(n), (uint64_t)n, "the skip bytes");
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_offset.p, rec_offset, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    if (skip) HIP_TRY(hipMemcpyAsync(c->skip.p, skip, (size_t)n, hipMemcpyHostToDevice, s));
    const bmq::state st = state_of(c);
    const size_t lds_bytes = bmq::lds_words(st.Cw) * 4;
    // two workgroups of `bases` per CU at the default window; a wave takes at most kWaveRecords records in one launch, which
    // keeps every u32 cell of a workgroup's LDS below 2^32 (bmq_kernels.hip.h)
    const uint32_t max_base_grid = 2 * c->n_cu, max_rec_grid = 8 * c->n_cu;
    const uint64_t per_launch = (uint64_t)max_base_grid * bmq::kBaseWaves * bmq::kWaveRecords;
    HIP_TRY(hipEventRecord(c->ev[0], s));
    const uint32_t rec_grid = (uint32_t)std::min<uint64_t>(((uint64_t)n + bmq::kRecThreads - 1) / bmq::kRecThreads, max_rec_grid);
    hipLaunchKernelGGL(bmq::records_kernel, dim3(rec_grid), dim3(bmq::kRecThreads), 0, s, c->in.p, c->rec_offset.p, n, skip ? c->skip.p : nullptr, st);
    for (uint64_t first = 0; first < n; first += per_launch) {
        const uint32_t part = (uint32_t)std::min<uint64_t>(per_launch, n - first);
        const uint32_t grid = (uint32_t)std::min<uint64_t>(((uint64_t)part + bmq::kBaseWaves - 1) / bmq::kBaseWaves, max_base_grid);
        hipLaunchKernelGGL(bmq::bases_kernel, dim3(grid), dim3(bmq::kBaseThreads), lds_bytes, s, c->in.p, c->rec_offset.p + first, part,
                           skip ? c->skip.p + first : nullptr, st);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->ms_add += ms;
    return BMQ_OK;
}

int bmq_finish(bmq_ctx *c, uint64_t *out_tallies) {
    if (!c) return fail(BMQ_ERR_ARG, "bmq_finish: null context");
    if (!c->begun) return fail(BMQ_ERR_ARG, "bmq_finish: no bmq_begin before it");
    if (c->finished) return fail(BMQ_ERR_ARG, "bmq_finish: it has run already, the next is bmq_begin");
    // every bmq_add has flushed its workgroups' counters into the u64 tables: nothing is partial here
    unsigned long long got[BMQ_N_TALLIES];
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(hipMemcpyAsync(got, c->cells.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->ms_finish, c->ev[0], c->ev[1]));
    c->finished = true;
    if (out_tallies)
        for (int k = 0; k < BMQ_N_TALLIES; k++) out_tallies[k] = got[k];
    return BMQ_OK;
}

int bmq_table(bmq_ctx *c, uint32_t which, uint64_t first, uint64_t count, uint64_t *out) {
    if (count && !out) return fail(BMQ_ERR_ARG, "bmq_table: null argument");
    if (!c) return fail(BMQ_ERR_ARG, "bmq_table: null context");
    if (!c->begun || !c->finished) return fail(BMQ_ERR_ARG, "bmq_table: no bmq_finish before it");
    if (which >= BMQ_N_TABLES) return fail(BMQ_ERR_ARG, "bmq_table: table %u asked for, the tables are 0 .. %d", which, BMQ_N_TABLES - 1);
    if (first > c->rows[which] || count > c->rows[which] - first)
        return fail(BMQ_ERR_ARG, "bmq_table: rows %llu .. %llu + %llu of table %u asked for, it has %llu", (unsigned long long)first, (unsigned long long)first,
                    (unsigned long long)count, which, (unsigned long long)c->rows[which]);
    if (count == 0) return BMQ_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->cells.p + BMQ_N_TALLIES + c->at[which] + first * kWidth[which], (size_t)(count * kWidth[which]) * 8, hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMQ_OK;
}

int bmq_last_stats(bmq_ctx *c, float *ms_add, float *ms_finish) {
    if (!c) return fail(BMQ_ERR_ARG, "bmq_last_stats: null argument");
    if (ms_add) *ms_add = c->ms_add;
    if (ms_finish) *ms_finish = c->ms_finish;
    return BMQ_OK;
}

}  // extern "C"
