// bmr_api.hip -- host side of the reference-block pass (include/bmr.h): the argument checks, buffers, the launches of
// bmr_kernels.hip.h and the downloads.  A bmr_ctx owns its stream and every buffer; it reads the cells, the reference table
// and the parameters of a bmg_ctx through bmg_ctx.hip.h and keeps no pointer to it between calls.
#include "../../include/bmr.h"

#include "bm_hip_util.h"
#include "bm_scan.hip.h"
#include "bmg_ctx.hip.h"
#include "bmr_kernels.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMR_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMR_OK == BMG_OK && BMR_ERR_ARG == BMG_ERR_ARG && BMR_ERR_HIP == BMG_ERR_HIP, "bmr.h and bmg.h must share their status codes");
static_assert(BMR_MAX_BANDS == bmr::kMaxBands && BMR_BLOCK_WORDS == bmr::kBlockWords && BMR_IN == bmr::kIn && BMR_EXCLUDED == bmr::kExcluded &&
                  BMR_NO_ALLELE == bmr::kNoAllele && BMR_CONF_WORDS == 2 && BMR_EXCLUDE_WORDS == 3,
              "bmr.h and bmr_kernels.hip.h disagree");

struct bmr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool ran = false;
    std::vector<uint32_t> ref_len;          // of the last bmr_run
    std::vector<uint64_t> ref_base;
    uint64_t n = 0, n_blocks = 0;
    DevBuf<uint8_t> base;
    DevBuf<uint32_t> st, dp, flag, rank, tmp, blk;
    DevBuf<uint64_t> d_ref_base, first, before;
    std::vector<uint64_t> h_first, h_before;
    std::vector<uint32_t> h_conf;
    float ms_kernels = 0.f;
    uint64_t bytes_state() const {
        return base.cap + 4ull * (st.cap + dp.cap + flag.cap + rank.cap + tmp.cap + blk.cap) + 8ull * (d_ref_base.cap + first.cap + before.cap);
    }
};

namespace {

#define BMR_NEED(call, bytes, what)                                                                                            \
    do {                                                                                                                       \
        if ((call) != hipSuccess) {                                                                                            \
            (void)hipGetLastError();                                                                                           \
            size_t free_b = 0, total_b = 0;                                                                                    \
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = 0;                                          \
            return fail(BMR_ERR_HIP,                                                                                           \
                        "cannot allocate %llu bytes for %s (%llu positions of %u references at 17 bytes each, %llu blocks at 32 bytes each, " \
                        "%llu excluded intervals; %llu of %llu bytes of device memory are free)",                              \
                        (unsigned long long)(bytes), what, (unsigned long long)n, n_ref, (unsigned long long)n_blocks,        \
                        (unsigned long long)n_exclude, (unsigned long long)free_b, (unsigned long long)total_b);               \
        }                                                                                                                      \
    } while (0)

inline unsigned grid_of(uint64_t items, uint64_t per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

extern "C" {

const char *bmr_last_error(void) { return g_err; }

int bmr_create(int32_t device, bmr_ctx **out) {
    if (!out) return fail(BMR_ERR_ARG, "bmr_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMR_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    bmr_ctx *c = new bmr_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        bmr_destroy(c);
        return fail(BMR_ERR_HIP, "bmr_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMR_OK;
}

void bmr_destroy(bmr_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->base.release();
    for (DevBuf<uint32_t> *b : {&c->st, &c->dp, &c->flag, &c->rank, &c->tmp, &c->blk}) b->release();
    for (DevBuf<uint64_t> *b : {&c->d_ref_base, &c->first, &c->before}) b->release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmr_run(bmr_ctx *c, bmg_ctx *g, const uint8_t *const *ref_bases, const uint32_t *bands, uint32_t n_bands, const uint32_t *exclude,
            uint64_t n_exclude, uint64_t *out_n_blocks) {
    if (!c || !g || !ref_bases || !out_n_blocks || (n_bands && !bands) || (n_exclude && !exclude)) return fail(BMR_ERR_ARG, "bmr_run: null argument");
    if (!g->begun) return fail(BMR_ERR_ARG, "bmr_run: no bmg_begin on the cells context before it");
    if (c->device != g->device) return fail(BMR_ERR_ARG, "bmr_run: the context is on device %d, the cells on device %d", c->device, g->device);
    const uint32_t n_ref = (uint32_t)g->ref_len.size();
    for (uint32_t r = 0; r < n_ref; r++)
        if (!ref_bases[r]) return fail(BMR_ERR_ARG, "bmr_run: no bases for reference %u (null pointer)", r);
    if (n_bands > BMR_MAX_BANDS) return fail(BMR_ERR_ARG, "bmr_run: %u band bounds, at most %d", n_bands, (int)BMR_MAX_BANDS);
    for (uint32_t k = 0; k < n_bands; k++) {
        if (bands[k] == 0 || bands[k] > 99) return fail(BMR_ERR_ARG, "bmr_run: band bound %u is %u, a bound is 1 .. 99", k, bands[k]);
        if (k && bands[k] <= bands[k - 1]) return fail(BMR_ERR_ARG, "bmr_run: band bound %u is %u, not above its predecessor %u", k, bands[k], bands[k - 1]);
    }
    for (uint64_t i = 0; i < n_exclude; i++) {
        const uint32_t ref = exclude[3 * i], start = exclude[3 * i + 1], end = exclude[3 * i + 2];
        if (ref >= n_ref) return fail(BMR_ERR_ARG, "bmr_run: interval %llu names reference %u, bmg_begin was given %u", (unsigned long long)i, ref, n_ref);
        if (start >= end) return fail(BMR_ERR_ARG, "bmr_run: interval %llu is %u .. %u, empty or backwards", (unsigned long long)i, start, end);
        if (end > g->ref_len[ref])
            return fail(BMR_ERR_ARG, "bmr_run: interval %llu ends at base %u of reference %u, which has %u", (unsigned long long)i, end, ref, g->ref_len[ref]);
    }
    // the checks are done: from here on the run before this one is gone
    c->ran = false;
    c->ms_kernels = 0.f;
    c->ref_len = g->ref_len;
    c->ref_base = g->ref_base;
    const uint64_t n = c->n = g->n_slots;
    uint64_t n_blocks = c->n_blocks = 0;
    c->h_first.resize((size_t)n_exclude);
    c->h_before.assign((size_t)n_exclude + 1, 0);
    for (uint64_t i = 0; i < n_exclude; i++) {
        c->h_first[i] = g->ref_base[exclude[3 * i]] + exclude[3 * i + 1];
        c->h_before[i + 1] = c->h_before[i] + (exclude[3 * i + 2] - exclude[3 * i + 1]);
    }
    const uint64_t total_excluded = c->h_before[n_exclude];
    bmr::bounds bd;
    for (uint32_t k = 0; k < bmr::kMaxBands; k++) bd.b[k] = k < n_bands ? bands[k] : bmr::kNone;

    HIP_TRY(hipSetDevice(c->device));
    const size_t padded = (size_t)((n + bmr::kQuad - 1) / bmr::kQuad * bmr::kQuad);   // conf and heads move whole quads
    BMR_NEED(c->base.need_exact(padded), padded, "the reference bases");
    BMR_NEED(c->st.need_exact(padded), padded * 4, "the states");
    BMR_NEED(c->dp.need_exact(padded), padded * 4, "the depths");
    BMR_NEED(c->flag.need_exact(padded), padded * 4, "the head flags");
    BMR_NEED(c->rank.need_exact((size_t)n + 1), (n + 1) * 4, "the ranks");
    BMR_NEED(c->tmp.need(bmscan::tmp_elems(n)), bmscan::tmp_elems(n) * 4, "the scan's block sums");
    BMR_NEED(c->d_ref_base.need((size_t)n_ref + 1), ((uint64_t)n_ref + 1) * 8, "the reference starts");
    if (n_exclude) {
        BMR_NEED(c->first.need((size_t)n_exclude), n_exclude * 8, "the intervals' starts");
        BMR_NEED(c->before.need((size_t)n_exclude + 1), (n_exclude + 1) * 8, "the intervals' prefix sums");
    }
    hipStream_t s = c->stream;
    for (uint32_t r = 0; r < n_ref; r++)
        HIP_TRY(hipMemcpyAsync(c->base.p + g->ref_base[r], ref_bases[r], g->ref_len[r], hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->d_ref_base.p, c->ref_base.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_exclude) {
        HIP_TRY(hipMemcpyAsync(c->first.p, c->h_first.data(), (size_t)n_exclude * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(c->before.p, c->h_before.data(), ((size_t)n_exclude + 1) * 8, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(g->stream));            // nothing of the cells context is in flight (its calls return finished)
    const unsigned quads = grid_of(n, (uint64_t)bmr::kThreads * bmr::kQuad);
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bmr::conf_kernel, dim3(quads), dim3(bmr::kThreads), 0, s, g->cell.p, c->base.p, n, bd, c->st.p, c->dp.p);
    if (total_excluded)
        hipLaunchKernelGGL(bmr::exclude_kernel, dim3(grid_of(total_excluded, bmr::kThreads)), dim3(bmr::kThreads), 0, s, c->first.p, c->before.p, n_exclude,
                           total_excluded, n, c->st.p);
    hipLaunchKernelGGL(bmr::heads_kernel, dim3(quads), dim3(bmr::kThreads), 0, s, c->st.p, n, c->flag.p);
    hipLaunchKernelGGL(bmr::ref_heads_kernel, dim3(grid_of(n_ref, bmr::kThreads)), dim3(bmr::kThreads), 0, s, c->d_ref_base.p, n_ref, c->st.p, c->flag.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->flag.p, c->rank.p, n, c->tmp.p, s));
    HIP_TRY(hipEventRecord(c->ev[1], s));
    uint32_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, c->rank.p + n, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    n_blocks = count;
    BMR_NEED(c->blk.need((size_t)n_blocks * bmr::kBlockWords), n_blocks * bmr::kBlockWords * 4, "the blocks");
    HIP_TRY(hipEventRecord(c->ev[2], s));
    if (n_blocks) {
        hipLaunchKernelGGL(bmr::fill_kernel, dim3(grid_of(n_blocks, bmr::kThreads)), dim3(bmr::kThreads), 0, s, c->blk.p, n_blocks);
        hipLaunchKernelGGL(bmr::blocks_kernel, dim3(grid_of(n, 64ull * bmr::kPerLane * (bmr::kThreads / 64))), dim3(bmr::kThreads), 0, s, c->st.p, c->dp.p,
                           c->flag.p, c->rank.p, n, c->d_ref_base.p, n_ref, c->blk.p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms_a = 0.f, ms_b = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_a, c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms_b, c->ev[2], c->ev[3]));
    c->ms_kernels = ms_a + ms_b;
    c->n_blocks = n_blocks;
    c->ran = true;
    *out_n_blocks = n_blocks;
    return BMR_OK;
}

int bmr_blocks(bmr_ctx *c, uint64_t first, uint64_t count, uint32_t *out) {
    if (count && !out) return fail(BMR_ERR_ARG, "bmr_blocks: null argument");
    if (!c) return fail(BMR_ERR_ARG, "bmr_blocks: null context");
    if (!c->ran) return fail(BMR_ERR_ARG, "bmr_blocks: no bmr_run before it");
    if (first > c->n_blocks || count > c->n_blocks - first)
        return fail(BMR_ERR_ARG, "bmr_blocks: blocks %llu .. %llu + %llu asked for, there are %llu", (unsigned long long)first, (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)c->n_blocks);
    if (count == 0) return BMR_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->blk.p + first * bmr::kBlockWords, (size_t)count * bmr::kBlockWords * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BMR_OK;
}

int bmr_conf_at(bmr_ctx *c, uint32_t ref, uint32_t start, uint32_t count, uint32_t *out) {
    if (count && !out) return fail(BMR_ERR_ARG, "bmr_conf_at: null argument");
    if (!c) return fail(BMR_ERR_ARG, "bmr_conf_at: null context");
    if (!c->ran) return fail(BMR_ERR_ARG, "bmr_conf_at: no bmr_run before it");
    if (ref >= c->ref_len.size()) return fail(BMR_ERR_ARG, "bmr_conf_at: reference %u of %zu", ref, c->ref_len.size());
    if ((uint64_t)start + count > c->ref_len[ref])
        return fail(BMR_ERR_ARG, "bmr_conf_at: bases %u .. %u + %u asked for, reference %u has %u", start, start, count, ref, c->ref_len[ref]);
    if (count == 0) return BMR_OK;
    HIP_TRY(hipSetDevice(c->device));
    c->h_conf.resize(2 * (size_t)count);
    const uint64_t at = c->ref_base[ref] + start;
    HIP_TRY(hipMemcpyAsync(c->h_conf.data(), c->st.p + at, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_conf.data() + count, c->dp.p + at, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < count; k++) out[2 * (size_t)k] = c->h_conf[k], out[2 * (size_t)k + 1] = c->h_conf[(size_t)count + k];
    return BMR_OK;
}

int bmr_last_stats(bmr_ctx *c, float *ms_kernels, uint64_t *bytes_state) {
    if (!c) return fail(BMR_ERR_ARG, "bmr_last_stats: null argument");
    if (ms_kernels) *ms_kernels = c->ms_kernels;
    if (bytes_state) *bytes_state = c->bytes_state();
    return BMR_OK;
}

}  // extern "C"
