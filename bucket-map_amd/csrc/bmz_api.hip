// bmz_api.hip -- host side of the BGZF block compressor (include/bmz.h): buffers, the launch, the packed download.
#include "bmz_ctx.hip.h"
#include "bmz_kernels.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMZ_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMZ_BLOCK_MAX == bmz::kBlockMax && BMZ_HASH_BITS == bmz::kHashBits, "bmz.h and the kernels disagree");

// the launch sequence of a call: the deflate kernel over the blocks, the scan of their sizes, the gather of the slots, and
// the packed download (bmz_ctx.hip.h)
int bmz_deflate_device(bmz_ctx *c, const uint8_t *d_in, uint64_t n_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap,
                       uint64_t *out_bytes) {
    const uint32_t n_blocks = (uint32_t)((n_bytes + block_bytes - 1) / block_bytes);
    *out_bytes = 0;
    c->h_offsets.assign(1, 0);
    c->ms_kernels = 0.f;
    c->n_form[0] = c->n_form[1] = c->n_form[2] = 0;
    HIP_TRY(hipSetDevice(c->device));
    const uint32_t stride = bmz::slot_stride(block_bytes), grid = std::min(n_blocks, c->n_cu);
    HIP_TRY(c->stage.need((size_t)n_blocks * stride));
    HIP_TRY(c->out.need((size_t)bmz_bound(n_bytes, block_bytes)));
    HIP_TRY(c->tokens.need((size_t)grid * bmz::kBlockMax));
    HIP_TRY(c->sizes.need(n_blocks));
    HIP_TRY(c->forms.need(n_blocks));
    HIP_TRY(c->offsets.need((size_t)n_blocks + 1));
    HIP_TRY(c->scan_tmp.need(bmscan::tmp_elems(n_blocks)));

    HIP_TRY(hipMemsetAsync(c->stage.p, 0, (size_t)n_blocks * stride, c->stream));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(bmz::deflate_kernel, dim3(grid), dim3(bmz::kThreads), 0, c->stream, d_in, n_bytes, block_bytes, n_blocks,
                       c->stage.p, c->tokens.p, c->sizes.p, c->forms.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(bmscan::exclusive_sum<uint64_t>(c->sizes.p, c->offsets.p, n_blocks, c->scan_tmp.p, c->stream));
    hipLaunchKernelGGL(bmz::gather_kernel, dim3(n_blocks), dim3(bmz::kThreads), 0, c->stream, c->stage.p, stride, c->sizes.p,
                       c->offsets.p, c->out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    c->h_offsets.resize((size_t)n_blocks + 1);
    std::vector<uint8_t> forms(n_blocks);
    HIP_TRY(hipMemcpyAsync(c->h_offsets.data(), c->offsets.p, ((size_t)n_blocks + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(forms.data(), c->forms.p, n_blocks, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t total = c->h_offsets[n_blocks];
    if (total > out_cap) return fail(BMZ_ERR_HIP, "bmz_deflate: the blocks take %llu bytes, beyond the bound", (unsigned long long)total);
    HIP_TRY(hipMemcpyAsync(out, c->out.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->ms_kernels, c->ev0, c->ev1));
    for (uint8_t f : forms)
        if (f < 3) c->n_form[f]++;
    *out_bytes = total;
    return BMZ_OK;
}

extern "C" {

const char *bmz_last_error(void) { return g_err; }

int bmz_create(int32_t device, bmz_ctx **out) {
    if (!out) return fail(BMZ_ERR_ARG, "bmz_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMZ_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if ((size_t)prop.sharedMemPerBlock < sizeof(bmz::Shared))
        return fail(BMZ_ERR_HIP, "device %d offers %zu bytes of LDS per workgroup, the parse needs %zu", device,
                    (size_t)prop.sharedMemPerBlock, sizeof(bmz::Shared));
    bmz_ctx *c = new bmz_ctx();
    c->device = device;
    c->n_cu = (uint32_t)std::max(1, prop.multiProcessorCount);
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e != hipSuccess) {
        bmz_destroy(c);
        return fail(BMZ_ERR_HIP, "bmz_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMZ_OK;
}

void bmz_destroy(bmz_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    c->in.release(); c->stage.release(); c->out.release(); c->forms.release();
    c->tokens.release(); c->sizes.release(); c->offsets.release(); c->scan_tmp.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

uint64_t bmz_bound(uint64_t n_bytes, uint32_t block_bytes) {
    if (block_bytes == 0) return 0;
    return n_bytes + 31 * ((n_bytes + block_bytes - 1) / block_bytes);
}

int bmz_deflate(bmz_ctx *c, const uint8_t *in, uint64_t n_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap,
                uint64_t *out_bytes) {
    if (block_bytes < 1 || block_bytes > BMZ_BLOCK_MAX)
        return fail(BMZ_ERR_ARG, "bmz_deflate: block_bytes must be in 1..%d (got %u)", (int)BMZ_BLOCK_MAX, block_bytes);
    if (!c || !out_bytes || (n_bytes && (!in || !out))) return fail(BMZ_ERR_ARG, "bmz_deflate: null argument");
    if (out_cap < bmz_bound(n_bytes, block_bytes))
        return fail(BMZ_ERR_ARG, "bmz_deflate: out holds %llu bytes, %llu may be needed", (unsigned long long)out_cap,
                    (unsigned long long)bmz_bound(n_bytes, block_bytes));
    const uint64_t n_blocks64 = (n_bytes + block_bytes - 1) / block_bytes;
    if (n_blocks64 > 0x7FFFFFFFull) return fail(BMZ_ERR_ARG, "bmz_deflate: %llu blocks in one call", (unsigned long long)n_blocks64);
    const uint32_t n_blocks = (uint32_t)n_blocks64;
    *out_bytes = 0;
    c->h_offsets.assign(1, 0);
    c->ms_kernels = 0.f;
    c->n_form[0] = c->n_form[1] = c->n_form[2] = 0;
    if (n_blocks == 0) return BMZ_OK;

    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->in.need((size_t)n_bytes + 8));
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, c->stream));
    return bmz_deflate_device(c, c->in.p, n_bytes, block_bytes, out, out_cap, out_bytes);
}

int bmz_blocks(bmz_ctx *c, uint64_t *out_offset) {
    if (!c || !out_offset) return fail(BMZ_ERR_ARG, "bmz_blocks: null argument");
    std::copy(c->h_offsets.begin(), c->h_offsets.end(), out_offset);
    return BMZ_OK;
}

int bmz_last_stats(bmz_ctx *c, float *ms_kernels, uint32_t *n_stored, uint32_t *n_fixed, uint32_t *n_dynamic) {
    if (!c) return fail(BMZ_ERR_ARG, "bmz_last_stats: null argument");
    if (ms_kernels) *ms_kernels = c->ms_kernels;
    if (n_stored) *n_stored = c->n_form[0];
    if (n_fixed) *n_fixed = c->n_form[1];
    if (n_dynamic) *n_dynamic = c->n_form[2];
    return BMZ_OK;
}

}  // extern "C"
