// bms_api.hip -- host side of the BAM record sorter (include/bms.h): the argument checks, buffers, the launches of
// bms_kernels.hip.h and the downloads.  The sorted stream is deflated where it lies by the compressor's own launch sequence
// (bmz_deflate_device, bmz_ctx.hip.h), on the compressor's stream, which carries all of the sorter's work too.
#include "bms_ctx.hip.h"
#include "bms_kernels.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMS_ERR_HIP)

static_assert(BMS_MIN_RECORD == bms::kMinRecord, "bms.h and the kernels disagree");
static_assert(bms::kChunk / bms::kMinRecord + 2 <= bms::kChunkRecords, "a gather chunk's records must fit its LDS table");

#define BMS_NEED(buf, count, what)                                                                                             \
    do {                                                                                                                       \
        if ((buf).need(count) != hipSuccess) {                                                                                 \
            (void)hipGetLastError();                                                                                           \
            return fail(BMS_ERR_HIP, "cannot allocate %zu bytes for %s (%u records, %llu stream bytes)",                       \
                        (size_t)(count) * sizeof(*(buf).p), what, n, (unsigned long long)n_bytes);                             \
        }                                                                                                                      \
    } while (0)

// what every entry point that takes a stream checks of it, without a device
int bms_check_stream(const char *who, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records) {
    if (n_records > 0x7FFFFFFFull) return fail(BMS_ERR_ARG, "%s: %llu records in one call, at most 2^31 - 1", who, (unsigned long long)n_records);
    if (rec_offset[0] != 0) return fail(BMS_ERR_ARG, "%s: rec_offset[0] is %llu, not 0", who, (unsigned long long)rec_offset[0]);
    for (uint64_t i = 0; i < n_records; i++)
        if (rec_offset[i + 1] <= rec_offset[i])
            return fail(BMS_ERR_ARG, "%s: rec_offset is not strictly ascending at record %llu", who, (unsigned long long)i);
    for (uint64_t i = 0; i < n_records; i++) {
        const uint64_t at = rec_offset[i], end = rec_offset[i + 1];
        if (end > n_bytes) return fail(BMS_ERR_ARG, "%s: record %llu ends at %llu, beyond the stream's %llu bytes", who, (unsigned long long)i,
                                       (unsigned long long)end, (unsigned long long)n_bytes);
        if (end - at < BMS_MIN_RECORD || end - at > 0xFFFFFFFFull)
            return fail(BMS_ERR_ARG, "%s: record %llu has %llu bytes, a BAM record has %d .. 2^32 - 1", who, (unsigned long long)i,
                        (unsigned long long)(end - at), (int)BMS_MIN_RECORD);
        uint32_t block_size;
        std::memcpy(&block_size, in + at, 4);
        if ((uint64_t)block_size != end - at - 4)
            return fail(BMS_ERR_ARG, "%s: record %llu says block_size %u but spans %llu bytes", who, (unsigned long long)i, block_size,
                        (unsigned long long)(end - at));
    }
    if (rec_offset[n_records] != n_bytes)
        return fail(BMS_ERR_ARG, "%s: rec_offset[%llu] is %llu, the stream has %llu bytes", who, (unsigned long long)n_records,
                    (unsigned long long)rec_offset[n_records], (unsigned long long)n_bytes);
    return BMS_OK;
}

// room for a stable sort of n (key, index) pairs: key[0..1], index[0..1], the tile counts and their scan, the digit counts
int bms_need_radix(bms_ctx *c, uint32_t n, uint64_t n_bytes) {
    const uint32_t n_tiles = (n + bms::kTile - 1) / bms::kTile;
    const uint64_t n_counts = (uint64_t)n_tiles * 256;
    for (int k = 0; k < 2; k++) {
        BMS_NEED(c->key[k], n, "the keys");
        BMS_NEED(c->index[k], n, "the indices");
    }
    BMS_NEED(c->counts, (size_t)n_counts, "the tile counts");
    BMS_NEED(c->place, (size_t)n_counts + 1, "the tile places");
    BMS_NEED(c->scan_tmp32, bmscan::tmp_elems(n_counts), "the scan of the tile counts");
    BMS_NEED(c->hist, 8 * 256, "the digit counts");
    return BMS_OK;
}

// every buffer of a sort of n records in n_bytes of stream
int bms_need_sort(bms_ctx *c, uint32_t n, uint64_t n_bytes) {
    HIP_TRY(hipSetDevice(c->z->device));
    BMS_NEED(c->in, (size_t)n_bytes + 8, "the stream");
    BMS_NEED(c->sorted, (size_t)n_bytes + 16, "the sorted stream");
    BMS_NEED(c->rec_offset, (size_t)n + 1, "the record offsets");
    BMS_NEED(c->sorted_offset, (size_t)n + 1, "the sorted offsets");
    if (const int rc = bms_need_radix(c, n, n_bytes)) return rc;
    BMS_NEED(c->length, n, "the lengths");
    BMS_NEED(c->perm_length, n, "the sorted lengths");
    BMS_NEED(c->scan_tmp64, bmscan::tmp_elems(n), "the scan of the lengths");
    return BMS_OK;
}

// the stream and its offsets to c->in and c->rec_offset, enqueued (bms_need_sort has run)
int bms_upload_stream(bms_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint32_t n) {
    hipStream_t s = c->z->stream;
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->rec_offset.p, rec_offset, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
    return BMS_OK;
}

// The n keys of c->key[*side] with their companions c->index[*side], sorted stably by the whole key: the digit counts in
// one pass, read by the host (this waits for the stream), then one count / scan / scatter pass per digit on which the keys
// differ.  *side names the buffers that hold the result; *n_passes grows by the passes that ran.  The events, where given,
// are recorded after the histogram and around the passes.
int bms_radix_sort(bms_ctx *c, uint32_t n, int *side, uint32_t *n_passes, hipEvent_t ev_hist_end, hipEvent_t ev_pass_begin,
                   hipEvent_t ev_pass_end) {
    hipStream_t s = c->z->stream;
    const uint32_t n_tiles = (n + bms::kTile - 1) / bms::kTile, n_blocks = (n + bms::kThreads - 1) / bms::kThreads;
    const uint64_t n_counts = (uint64_t)n_tiles * 256;
    HIP_TRY(hipMemsetAsync(c->hist.p, 0, 8 * 256 * 4, s));
    hipLaunchKernelGGL(bms::hist_kernel, dim3(std::min(n_blocks, 4 * c->n_cu)), dim3(bms::kThreads), 0, s, c->key[*side].p, n, c->hist.p);
    HIP_TRY(hipGetLastError());
    if (ev_hist_end) HIP_TRY(hipEventRecord(ev_hist_end, s));
    uint32_t hist[8 * 256];
    HIP_TRY(hipMemcpyAsync(hist, c->hist.p, sizeof hist, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    if (ev_pass_begin) HIP_TRY(hipEventRecord(ev_pass_begin, s));
    for (uint32_t d = 0; d < 8; d++) {
        bool constant = false;                           // one bucket holds every key: the pass would move nothing
        for (uint32_t b = 0; b < 256 && !constant; b++) constant = hist[d * 256 + b] == n;
        if (constant) continue;
        hipLaunchKernelGGL(bms::count_kernel, dim3(n_tiles), dim3(bms::kThreads), 0, s, c->key[*side].p, n, 8 * d, n_tiles, c->counts.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->counts.p, c->place.p, n_counts, c->scan_tmp32.p, s));
        hipLaunchKernelGGL(bms::scatter_kernel, dim3(n_tiles), dim3(bms::kThreads), 0, s, c->key[*side].p, c->index[*side].p, n, 8 * d, n_tiles,
                           c->place.p, c->key[*side ^ 1].p, c->index[*side ^ 1].p);
        HIP_TRY(hipGetLastError());
        *side ^= 1;
        (*n_passes)++;
    }
    if (ev_pass_end) HIP_TRY(hipEventRecord(ev_pass_end, s));
    return BMS_OK;
}

// the records of c->in[0, n_bytes) (offsets in c->rec_offset) in order: c->sorted, c->index[*final_side] (perm) and
// c->sorted_offset on the device, enqueued
int bms_sort_on_device(bms_ctx *c, uint64_t n_bytes, uint32_t n, int *final_side) {
    hipStream_t s = c->z->stream;
    const uint32_t n_blocks = (n + bms::kThreads - 1) / bms::kThreads;
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(bms::keys_kernel, dim3(n_blocks), dim3(bms::kThreads), 0, s, c->in.p, c->rec_offset.p, n, c->key[0].p, c->index[0].p,
                       c->length.p);
    HIP_TRY(hipGetLastError());
    int side = 0;
    if (const int rc = bms_radix_sort(c, n, &side, &c->n_passes, c->ev[1], c->ev[2], c->ev[3])) return rc;
    HIP_TRY(hipEventRecord(c->ev[4], s));
    hipLaunchKernelGGL(bms::perm_len_kernel, dim3(n_blocks), dim3(bms::kThreads), 0, s, c->index[side].p, c->length.p, n, c->perm_length.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(bmscan::exclusive_sum<uint64_t>(c->perm_length.p, c->sorted_offset.p, n, c->scan_tmp64.p, s));
    const uint64_t n_chunks = (n_bytes + bms::kChunk - 1) / bms::kChunk;
    if (n_chunks > 0x7FFFFFFFull) return fail(BMS_ERR_ARG, "a stream of %llu bytes is beyond one call", (unsigned long long)n_bytes);
    hipLaunchKernelGGL(bms::gather_kernel, dim3((uint32_t)n_chunks), dim3(bms::kThreads), 0, s, c->in.p, c->rec_offset.p, c->index[side].p,
                       c->sorted_offset.p, n, n_bytes, c->sorted.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[5], s));
    *final_side = side;
    return BMS_OK;
}

int bms_read_times(bms_ctx *c) {
    float a = 0.f, b = 0.f;
    HIP_TRY(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&b, c->ev[2], c->ev[3]));
    c->ms_sort = a + b;
    HIP_TRY(hipEventElapsedTime(&c->ms_gather, c->ev[4], c->ev[5]));
    return BMS_OK;
}

void bms_reset_stats(bms_ctx *c) {
    c->ms_sort = c->ms_gather = c->ms_deflate = 0.f;
    c->n_passes = 0;
}


namespace {

// the upload, then the launches
int upload_and_sort(bms_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint32_t n, int *final_side) {
    if (const int rc = bms_need_sort(c, n, n_bytes)) return rc;
    if (const int rc = bms_upload_stream(c, in, n_bytes, rec_offset, n)) return rc;
    return bms_sort_on_device(c, n_bytes, n, final_side);
}

}  // namespace

extern "C" {

const char *bms_last_error(void) { return g_err; }

int bms_create(int32_t device, bms_ctx **out) {
    if (!out) return fail(BMS_ERR_ARG, "bms_create: null argument");
    *out = nullptr;
    bmz_ctx *z = nullptr;
    const int rc = bmz_create(device, &z);
    if (rc != BMZ_OK) return fail(rc == BMZ_ERR_ARG ? BMS_ERR_ARG : BMS_ERR_HIP, "bms_create: %s", bmz_last_error());
    bms_ctx *c = new bms_ctx();
    c->z = z;
    c->n_cu = z->n_cu;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 6 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        bms_destroy(c);
        return fail(BMS_ERR_HIP, "bms_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMS_OK;
}

void bms_destroy(bms_ctx *c) {
    if (!c) return;
    if (c->z) {
        (void)hipSetDevice(c->z->device);
        if (c->z->stream) (void)hipStreamSynchronize(c->z->stream);
    }
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    c->in.release(); c->sorted.release(); c->rec_offset.release(); c->sorted_offset.release(); c->scan_tmp64.release();
    for (int k = 0; k < 2; k++) c->key[k].release(), c->index[k].release();
    c->length.release(); c->perm_length.release(); c->counts.release(); c->place.release(); c->scan_tmp32.release(); c->hist.release();
    bmz_destroy(c->z);
    delete c;
}

int bms_sort(bms_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, uint8_t *out_sorted,
             uint32_t *out_perm, uint64_t *out_sorted_offset) {
    if (!rec_offset || !out_sorted_offset || (n_records && !out_perm) || (n_bytes && (!in || !out_sorted)))
        return fail(BMS_ERR_ARG, "bms_sort: null argument");
    if (const int rc = bms_check_stream("bms_sort", in, n_bytes, rec_offset, n_records)) return rc;
    if (!c) return fail(BMS_ERR_ARG, "bms_sort: null context");
    bms_reset_stats(c);
    out_sorted_offset[0] = 0;
    if (n_records == 0) return BMS_OK;
    const uint32_t n = (uint32_t)n_records;
    int side = 0;
    if (const int rc = upload_and_sort(c, in, n_bytes, rec_offset, n, &side)) return rc;
    hipStream_t s = c->z->stream;
    HIP_TRY(hipMemcpyAsync(out_sorted, c->sorted.p, (size_t)n_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_perm, c->index[side].p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_sorted_offset, c->sorted_offset.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return bms_read_times(c);
}

int bms_sort_deflate(bms_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, uint32_t block_bytes,
                     uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *out_perm, uint64_t *out_sorted_offset) {
    if (block_bytes < 1 || block_bytes > BMZ_BLOCK_MAX)
        return fail(BMS_ERR_ARG, "bms_sort_deflate: block_bytes must be in 1..%d (got %u)", (int)BMZ_BLOCK_MAX, block_bytes);
    if (!rec_offset || !out_sorted_offset || !out_bytes || (n_records && !out_perm) || (n_bytes && (!in || !out)))
        return fail(BMS_ERR_ARG, "bms_sort_deflate: null argument");
    if (out_cap < bmz_bound(n_bytes, block_bytes))
        return fail(BMS_ERR_ARG, "bms_sort_deflate: out holds %llu bytes, %llu may be needed", (unsigned long long)out_cap,
                    (unsigned long long)bmz_bound(n_bytes, block_bytes));
    if ((n_bytes + block_bytes - 1) / block_bytes > 0x7FFFFFFFull)
        return fail(BMS_ERR_ARG, "bms_sort_deflate: %llu blocks in one call", (unsigned long long)((n_bytes + block_bytes - 1) / block_bytes));
    if (const int rc = bms_check_stream("bms_sort_deflate", in, n_bytes, rec_offset, n_records)) return rc;
    if (!c) return fail(BMS_ERR_ARG, "bms_sort_deflate: null context");
    bms_reset_stats(c);
    *out_bytes = 0;
    out_sorted_offset[0] = 0;
    if (n_records == 0) return BMS_OK;
    const uint32_t n = (uint32_t)n_records;
    int side = 0;
    if (const int rc = upload_and_sort(c, in, n_bytes, rec_offset, n, &side)) return rc;
    hipStream_t s = c->z->stream;
    HIP_TRY(hipMemcpyAsync(out_perm, c->index[side].p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_sorted_offset, c->sorted_offset.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (bmz_deflate_device(c->z, c->sorted.p, n_bytes, block_bytes, out, out_cap, out_bytes) != BMZ_OK)
        return fail(BMS_ERR_HIP, "bms_sort_deflate: %s", bmz_last_error());
    c->ms_deflate = c->z->ms_kernels;
    return bms_read_times(c);
}

int bms_last_stats(bms_ctx *c, float *ms_sort, float *ms_gather, float *ms_deflate, uint32_t *n_passes) {
    if (!c) return fail(BMS_ERR_ARG, "bms_last_stats: null argument");
    if (ms_sort) *ms_sort = c->ms_sort;
    if (ms_gather) *ms_gather = c->ms_gather;
    if (ms_deflate) *ms_deflate = c->ms_deflate;
    if (n_passes) *n_passes = c->n_passes;
    return BMS_OK;
}

}  // extern "C"
