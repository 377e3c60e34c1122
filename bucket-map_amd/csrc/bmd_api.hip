// bmd_api.hip -- host side of the duplicate marker (include/bmd.h): the argument checks, buffers, the launches of
// bmd_kernels.hip.h and the downloads.  A bmd_ctx owns a bms_ctx: the stream lies in the sorter's buffers, the marker's own
// sorts are the sorter's radix passes (bms_radix_sort, bms_ctx.hip.h) over the sorter's key and index buffers, and the fused
// call goes on with the sorter's launch sequence and the deflate on the same device copy.
#include "../../include/bmd.h"

#include "bm_scan.hip.h"
#include "bmd_kernels.hip.h"
#include "bms_ctx.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMD_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMD_OK == BMS_OK && BMD_ERR_ARG == BMS_ERR_ARG && BMD_ERR_HIP == BMS_ERR_HIP, "bmd.h and bms.h must share their status codes");

struct bmd_ctx {
    bms_ctx *s = nullptr;                   // owns the device, the stream, the stream's copy and the radix buffers
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // ends | mark: begin, end
    DevBuf<uint64_t> end, score, p_lo, p_hi, p_key, a_end, a_key;
    DevBuf<uint8_t> kind, eligible, dup;
    DevBuf<uint32_t> is_pair, is_frag, pair_slot, frag_slot, pair_mark, frag_mark, mark_sum, scan_tmp;
    float ms_ends = 0.f, ms_mark = 0.f;
    uint32_t n_passes = 0;
};

namespace {

#define BMD_NEED(buf, count, what)                                                                                             \
    do {                                                                                                                       \
        if ((buf).need(count) != hipSuccess) {                                                                                 \
            (void)hipGetLastError();                                                                                           \
            return fail(BMD_ERR_HIP, "cannot allocate %zu bytes for %s (%u records, %llu stream bytes)",                       \
                        (size_t)(count) * sizeof(*(buf).p), what, n, (unsigned long long)n_bytes);                             \
        }                                                                                                                      \
    } while (0)

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + bmd::kThreads - 1) / bmd::kThreads); }

// the one check bmd adds to the sorter's: the fields of every record lie inside it
int check_fields(const char *who, const uint8_t *in, const uint64_t *rec_offset, uint64_t n_records) {
    for (uint64_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        const uint64_t length = rec_offset[i + 1] - rec_offset[i];
        uint16_t n_cigar;
        uint32_t l_seq;
        std::memcpy(&n_cigar, r + 16, 2);
        std::memcpy(&l_seq, r + 20, 4);
        const uint64_t need = 36ull + r[12] + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + l_seq;
        if (need > length)
            return fail(BMD_ERR_ARG, "%s: the fields of record %llu take %llu bytes and do not fit its %llu", who, (unsigned long long)i,
                        (unsigned long long)need, (unsigned long long)length);
    }
    return BMD_OK;
}

void reset_stats(bmd_ctx *c) {
    c->ms_ends = c->ms_mark = 0.f;
    c->n_passes = 0;
    bms_reset_stats(c->s);
}

// end, score, kind of the n records of the sorter's device copy, enqueued
int ends_on_device(bmd_ctx *c, uint64_t n_bytes, uint32_t n) {
    bms_ctx *b = c->s;
    hipStream_t s = b->z->stream;
    BMD_NEED(c->end, n, "the ends");
    BMD_NEED(c->score, n, "the scores");
    BMD_NEED(c->kind, n, "the kinds");
    BMD_NEED(c->eligible, n, "the eligibility");
    const uint64_t n_chunks = (n_bytes + bmd::kChunk - 1) / bmd::kChunk;
    if (n_chunks > 0x7FFFFFFFull) return fail(BMD_ERR_ARG, "a stream of %llu bytes is beyond one call", (unsigned long long)n_bytes);
    HIP_TRY(hipEventRecord(c->ev[0], s));
    HIP_TRY(hipMemsetAsync(c->score.p, 0, (size_t)n * 8, s));
    hipLaunchKernelGGL(bmd::qual_sum_kernel, dim3((uint32_t)n_chunks), dim3(bmd::kThreads), 0, s, b->in.p, b->rec_offset.p, n, n_bytes, c->score.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bmd::cigar_ends_kernel, dim3((n + bmd::kWaves - 1) / bmd::kWaves), dim3(bmd::kThreads), 0, s, b->in.p, b->rec_offset.p, n,
                       c->end.p, c->eligible.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bmd::kinds_kernel, dim3(blocks_of(n)), dim3(bmd::kThreads), 0, s, b->in.p, b->rec_offset.p, n, c->eligible.p, c->kind.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    return BMD_OK;
}

// one stable sort of m items by the u64 word[item], in the order the items have in index (fresh: 0, 1, ...)
int sort_by(bmd_ctx *c, const uint64_t *word, uint32_t m, bool fresh, int *side) {
    bms_ctx *b = c->s;
    hipStream_t s = b->z->stream;
    if (fresh) {
        *side = 0;
        hipLaunchKernelGGL(bmd::iota_kernel, dim3(blocks_of(m)), dim3(bmd::kThreads), 0, s, word, m, b->key[0].p, b->index[0].p);
    } else {
        hipLaunchKernelGGL(bmd::rekey_kernel, dim3(blocks_of(m)), dim3(bmd::kThreads), 0, s, word, b->index[*side].p, m, b->key[*side].p);
    }
    HIP_TRY(hipGetLastError());
    if (const int rc = bms_radix_sort(b, m, side, &c->n_passes)) return fail(rc, "%s", bms_last_error());
    return BMD_OK;
}

// dup[0, n) on the device from c->end, c->score, c->kind; stream / rec_offset non-null: the flag bytes are set too.
// counts[0..3] on the host.  Waits for the stream (the unit counts and every sort's digit counts are read by the host).
int mark_on_device(bmd_ctx *c, uint32_t n, uint64_t n_bytes, uint8_t *d_stream, const uint64_t *d_rec_offset, uint64_t *counts) {
    bms_ctx *b = c->s;
    hipStream_t s = b->z->stream;
    if (bms_need_radix(b, n, n_bytes)) return fail(BMD_ERR_HIP, "%s", bms_last_error());
    BMD_NEED(c->dup, n, "the marks");
    BMD_NEED(c->is_pair, n, "the pair flags");
    BMD_NEED(c->is_frag, n, "the fragment flags");
    BMD_NEED(c->pair_slot, (size_t)n + 1, "the pair slots");
    BMD_NEED(c->frag_slot, (size_t)n + 1, "the fragment slots");
    BMD_NEED(c->scan_tmp, bmscan::tmp_elems((uint64_t)n + 1), "the scans of the units");
    HIP_TRY(hipEventRecord(c->ev[2], s));
    hipLaunchKernelGGL(bmd::unit_flags_kernel, dim3(blocks_of(n)), dim3(bmd::kThreads), 0, s, c->kind.p, n, c->is_pair.p, c->is_frag.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->is_pair.p, c->pair_slot.p, n, c->scan_tmp.p, s));
    HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->is_frag.p, c->frag_slot.p, n, c->scan_tmp.p, s));
    uint32_t n_pairs = 0, n_frags = 0;
    HIP_TRY(hipMemcpyAsync(&n_pairs, c->pair_slot.p + n, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&n_frags, c->frag_slot.p + n, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t n_items = 2ull * n_pairs + n_frags;
    if (n_items > n) return fail(BMD_ERR_HIP, "the unit counts (%u pairs, %u fragments) exceed the %u records", n_pairs, n_frags, n);
    const uint32_t m = (uint32_t)n_items;
    BMD_NEED(c->p_lo, n_pairs, "the pair keys");
    BMD_NEED(c->p_hi, n_pairs, "the pair keys");
    BMD_NEED(c->p_key, n_pairs, "the pair scores");
    BMD_NEED(c->a_end, m, "the fragment pass' ends");
    BMD_NEED(c->a_key, m, "the fragment pass' scores");
    BMD_NEED(c->pair_mark, n_pairs, "the pair marks");
    BMD_NEED(c->frag_mark, n_frags, "the fragment marks");
    BMD_NEED(c->mark_sum, (size_t)std::max(n_pairs, n_frags) + 2, "the mark counts");
    hipLaunchKernelGGL(bmd::build_kernel, dim3(blocks_of(n)), dim3(bmd::kThreads), 0, s, c->end.p, c->score.p, c->kind.p, n, c->pair_slot.p,
                       c->frag_slot.p, n_pairs, n_frags, c->p_lo.p, c->p_hi.p, c->p_key.p, c->a_end.p, c->a_key.p);
    HIP_TRY(hipGetLastError());
    int side = 0;
    uint32_t dup_pairs = 0, dup_frags = 0;
    if (n_pairs) {                                       // by ~score, then the key's low word, then its high word
        if (const int rc = sort_by(c, c->p_key.p, n_pairs, true, &side)) return rc;
        if (const int rc = sort_by(c, c->p_lo.p, n_pairs, false, &side)) return rc;
        if (const int rc = sort_by(c, c->p_hi.p, n_pairs, false, &side)) return rc;
        hipLaunchKernelGGL(bmd::pair_heads_kernel, dim3(blocks_of(n_pairs)), dim3(bmd::kThreads), 0, s, b->index[side].p, n_pairs, c->p_lo.p,
                           c->p_hi.p, c->pair_mark.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->pair_mark.p, c->mark_sum.p, n_pairs, c->scan_tmp.p, s));
        HIP_TRY(hipMemcpyAsync(&dup_pairs, c->mark_sum.p + n_pairs, 4, hipMemcpyDeviceToHost, s));
    }
    if (n_frags) {                                       // pair ends lead (key 0), then by ~score; then by E
        if (const int rc = sort_by(c, c->a_key.p, m, true, &side)) return rc;
        if (const int rc = sort_by(c, c->a_end.p, m, false, &side)) return rc;
        hipLaunchKernelGGL(bmd::frag_heads_kernel, dim3(blocks_of(m)), dim3(bmd::kThreads), 0, s, b->index[side].p, m, c->a_end.p, 2 * n_pairs,
                           c->frag_mark.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(bmscan::exclusive_sum<uint32_t>(c->frag_mark.p, c->mark_sum.p, n_frags, c->scan_tmp.p, s));
        HIP_TRY(hipMemcpyAsync(&dup_frags, c->mark_sum.p + n_frags, 4, hipMemcpyDeviceToHost, s));
    }
    hipLaunchKernelGGL(bmd::apply_kernel, dim3(blocks_of(n)), dim3(bmd::kThreads), 0, s, c->kind.p, n, c->pair_slot.p, c->frag_slot.p,
                       c->pair_mark.p, c->frag_mark.p, c->dup.p, d_stream, d_rec_offset);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[3], s));
    HIP_TRY(hipStreamSynchronize(s));
    counts[0] = n_pairs, counts[1] = n_frags, counts[2] = 2ull * dup_pairs, counts[3] = dup_frags;
    return BMD_OK;
}

int read_times(bmd_ctx *c, bool ends, bool mark) {
    if (ends) HIP_TRY(hipEventElapsedTime(&c->ms_ends, c->ev[0], c->ev[1]));
    if (mark) HIP_TRY(hipEventElapsedTime(&c->ms_mark, c->ev[2], c->ev[3]));
    return BMD_OK;
}

}  // namespace

extern "C" {

const char *bmd_last_error(void) { return g_err; }

int bmd_create(int32_t device, bmd_ctx **out) {
    if (!out) return fail(BMD_ERR_ARG, "bmd_create: null argument");
    *out = nullptr;
    bms_ctx *s = nullptr;
    const int rc = bms_create(device, &s);
    if (rc != BMS_OK) return fail(rc, "bmd_create: %s", bms_last_error());
    bmd_ctx *c = new bmd_ctx();
    c->s = s;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        bmd_destroy(c);
        return fail(BMD_ERR_HIP, "bmd_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMD_OK;
}

void bmd_destroy(bmd_ctx *c) {
    if (!c) return;
    if (c->s && c->s->z) {
        (void)hipSetDevice(c->s->z->device);
        if (c->s->z->stream) (void)hipStreamSynchronize(c->s->z->stream);
    }
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf<uint64_t> *b : {&c->end, &c->score, &c->p_lo, &c->p_hi, &c->p_key, &c->a_end, &c->a_key}) b->release();
    for (DevBuf<uint8_t> *b : {&c->kind, &c->eligible, &c->dup}) b->release();
    for (DevBuf<uint32_t> *b : {&c->is_pair, &c->is_frag, &c->pair_slot, &c->frag_slot, &c->pair_mark, &c->frag_mark, &c->mark_sum, &c->scan_tmp})
        b->release();
    bms_destroy(c->s);
    delete c;
}

int bmd_ends(bmd_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, uint64_t *out_end,
             uint64_t *out_score, uint8_t *out_kind) {
    if (!rec_offset || (n_records && (!out_end || !out_score || !out_kind)) || (n_bytes && !in)) return fail(BMD_ERR_ARG, "bmd_ends: null argument");
    if (const int rc = bms_check_stream("bmd_ends", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_fields("bmd_ends", in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMD_ERR_ARG, "bmd_ends: null context");
    reset_stats(c);
    if (n_records == 0) return BMD_OK;
    const uint32_t n = (uint32_t)n_records;
    if (const int rc = bms_need_sort(c->s, n, n_bytes)) return fail(rc, "%s", bms_last_error());
    if (const int rc = bms_upload_stream(c->s, in, n_bytes, rec_offset, n)) return fail(rc, "%s", bms_last_error());
    if (const int rc = ends_on_device(c, n_bytes, n)) return rc;
    hipStream_t s = c->s->z->stream;
    HIP_TRY(hipMemcpyAsync(out_end, c->end.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_score, c->score.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_kind, c->kind.p, (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return read_times(c, true, false);
}

int bmd_mark(bmd_ctx *c, const uint64_t *end, const uint64_t *score, const uint8_t *kind, uint64_t n_records, uint8_t *out_dup,
             uint64_t *out_counts) {
    if (!out_counts || (n_records && (!end || !score || !kind || !out_dup))) return fail(BMD_ERR_ARG, "bmd_mark: null argument");
    if (n_records > 0x7FFFFFFFull) return fail(BMD_ERR_ARG, "bmd_mark: %llu records in one call, at most 2^31 - 1", (unsigned long long)n_records);
    for (uint64_t i = 0; i < n_records; i++) {
        if (kind[i] > 3) return fail(BMD_ERR_ARG, "bmd_mark: kind[%llu] is %u, a kind is 0 .. 3", (unsigned long long)i, (unsigned)kind[i]);
        if (kind[i] == 2 && (i + 1 == n_records || kind[i + 1] != 3))
            return fail(BMD_ERR_ARG, "bmd_mark: kind[%llu] is 2 and is not followed by a 3", (unsigned long long)i);
        if (kind[i] == 3 && (i == 0 || kind[i - 1] != 2))
            return fail(BMD_ERR_ARG, "bmd_mark: kind[%llu] is 3 and is not preceded by a 2", (unsigned long long)i);
    }
    if (!c) return fail(BMD_ERR_ARG, "bmd_mark: null context");
    reset_stats(c);
    out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (n_records == 0) return BMD_OK;
    const uint32_t n = (uint32_t)n_records;
    const uint64_t n_bytes = 0;
    hipStream_t s = c->s->z->stream;
    HIP_TRY(hipSetDevice(c->s->z->device));
    BMD_NEED(c->end, n, "the ends");
    BMD_NEED(c->score, n, "the scores");
    BMD_NEED(c->kind, n, "the kinds");
    HIP_TRY(hipMemcpyAsync(c->end.p, end, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->score.p, score, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c->kind.p, kind, (size_t)n, hipMemcpyHostToDevice, s));
    if (const int rc = mark_on_device(c, n, n_bytes, nullptr, nullptr, out_counts)) return rc;
    HIP_TRY(hipMemcpyAsync(out_dup, c->dup.p, (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return read_times(c, false, true);
}

int bmd_mark_sort_deflate(bmd_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records, uint32_t block_bytes,
                          uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *out_perm, uint64_t *out_sorted_offset, uint8_t *out_dup,
                          uint64_t *out_counts) {
    if (block_bytes < 1 || block_bytes > BMZ_BLOCK_MAX)
        return fail(BMD_ERR_ARG, "bmd_mark_sort_deflate: block_bytes must be in 1..%d (got %u)", (int)BMZ_BLOCK_MAX, block_bytes);
    if (!rec_offset || !out_sorted_offset || !out_bytes || !out_counts || (n_records && (!out_perm || !out_dup)) || (n_bytes && (!in || !out)))
        return fail(BMD_ERR_ARG, "bmd_mark_sort_deflate: null argument");
    if (out_cap < bmz_bound(n_bytes, block_bytes))
        return fail(BMD_ERR_ARG, "bmd_mark_sort_deflate: out holds %llu bytes, %llu may be needed", (unsigned long long)out_cap,
                    (unsigned long long)bmz_bound(n_bytes, block_bytes));
    if ((n_bytes + block_bytes - 1) / block_bytes > 0x7FFFFFFFull)
        return fail(BMD_ERR_ARG, "bmd_mark_sort_deflate: %llu blocks in one call", (unsigned long long)((n_bytes + block_bytes - 1) / block_bytes));
    if (const int rc = bms_check_stream("bmd_mark_sort_deflate", in, n_bytes, rec_offset, n_records)) return fail(rc, "%s", bms_last_error());
    if (const int rc = check_fields("bmd_mark_sort_deflate", in, rec_offset, n_records)) return rc;
    if (!c) return fail(BMD_ERR_ARG, "bmd_mark_sort_deflate: null context");
    reset_stats(c);
    *out_bytes = 0;
    out_sorted_offset[0] = 0;
    out_counts[0] = out_counts[1] = out_counts[2] = out_counts[3] = 0;
    if (n_records == 0) return BMD_OK;
    const uint32_t n = (uint32_t)n_records;
    bms_ctx *b = c->s;
    if (const int rc = bms_need_sort(b, n, n_bytes)) return fail(rc, "%s", bms_last_error());
    if (const int rc = bms_upload_stream(b, in, n_bytes, rec_offset, n)) return fail(rc, "%s", bms_last_error());
    if (const int rc = ends_on_device(c, n_bytes, n)) return rc;
    if (const int rc = mark_on_device(c, n, n_bytes, b->in.p, b->rec_offset.p, out_counts)) return rc;
    int side = 0;
    if (const int rc = bms_sort_on_device(b, n_bytes, n, &side)) return fail(rc, "%s", bms_last_error());
    hipStream_t s = b->z->stream;
    HIP_TRY(hipMemcpyAsync(out_perm, b->index[side].p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_sorted_offset, b->sorted_offset.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_dup, c->dup.p, (size_t)n, hipMemcpyDeviceToHost, s));
    if (bmz_deflate_device(b->z, b->sorted.p, n_bytes, block_bytes, out, out_cap, out_bytes) != BMZ_OK)
        return fail(BMD_ERR_HIP, "bmd_mark_sort_deflate: %s", bmz_last_error());
    b->ms_deflate = b->z->ms_kernels;
    if (const int rc = bms_read_times(b)) return fail(rc, "%s", bms_last_error());
    return read_times(c, true, true);
}

int bmd_last_stats(bmd_ctx *c, float *ms_ends, float *ms_mark, uint32_t *n_passes) {
    if (!c) return fail(BMD_ERR_ARG, "bmd_last_stats: null argument");
    if (ms_ends) *ms_ends = c->ms_ends;
    if (ms_mark) *ms_mark = c->ms_mark;
    if (n_passes) *n_passes = c->n_passes;
    return BMD_OK;
}

int bmd_last_sort_stats(bmd_ctx *c, float *ms_sort, float *ms_gather, float *ms_deflate, uint32_t *n_passes) {
    if (!c) return fail(BMD_ERR_ARG, "bmd_last_sort_stats: null argument");
    if (bms_last_stats(c->s, ms_sort, ms_gather, ms_deflate, n_passes) != BMS_OK) return fail(BMD_ERR_ARG, "bmd_last_sort_stats: %s", bms_last_error());
    return BMD_OK;
}

}  // extern "C"
