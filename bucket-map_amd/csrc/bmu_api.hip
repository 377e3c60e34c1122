// bmu_api.hip -- host side of the BGZF block inflater (include/bmu.h): the layout walk, buffers, the launch, the check.
#include "../../include/bmu.h"

#include "../host/bgzf_in.h"
#include "bm_hip_util.h"
#include "bmu_kernels.hip.h"

#define HIP_TRY(expr) BM_HIP_TRY(expr, BMU_ERR_HIP)

using bmhip::DevBuf;

static_assert(BMU_REASON_TRUNCATED == bmu_rule::kTruncated && BMU_REASON_BLOCK_TYPE == bmu_rule::kBadType &&
                  BMU_REASON_STORED_LEN == bmu_rule::kStoredLen && BMU_REASON_CODE == bmu_rule::kBadCode &&
                  BMU_REASON_DISTANCE == bmu_rule::kDistance && BMU_REASON_TOO_LONG == bmu_rule::kTooLong &&
                  BMU_REASON_TOO_SHORT == bmu_rule::kTooShort && BMU_REASON_CRC == bmu_rule::kCrc,
              "bmu.h and inflate_rule.h disagree");

struct bmu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DevBuf<uint8_t> in, out;
    DevBuf<uint64_t> payload_at, out_offset;
    DevBuf<uint32_t> payload_len;
    DevBuf<bmu::Result> result;
    std::vector<bm::bgzf_member> members;
    std::vector<uint64_t> h_payload_at, h_out_offset;
    std::vector<uint32_t> h_payload_len;
    std::vector<bmu::Result> h_result;
    float ms_kernels = 0.f;
    uint64_t n_type[3] = {0, 0, 0};
    uint64_t bad_block = UINT64_MAX;
    uint32_t bad_reason = 0;
};

extern "C" {

const char *bmu_last_error(void) { return g_err; }

int bmu_layout(const uint8_t *in, uint64_t n_bytes, uint64_t *in_offset, uint64_t *out_offset, uint64_t *n_blocks, uint64_t *out_bytes) {
    if ((n_bytes && !in) || !n_blocks || !out_bytes) return fail(BMU_ERR_ARG, "bmu_layout: null argument");
    *n_blocks = 0, *out_bytes = 0;
    std::vector<bm::bgzf_member> members;
    std::string error;
    if (!bm::bgzf_layout(in, n_bytes, members, error)) return fail(BMU_ERR_FORMAT, "%s", error.c_str());
    uint64_t total = 0;
    for (size_t b = 0; b < members.size(); b++) {
        if (in_offset) in_offset[b] = members[b].at;
        if (out_offset) out_offset[b] = total;
        total += members[b].isize;
    }
    if (in_offset) in_offset[members.size()] = n_bytes;
    if (out_offset) out_offset[members.size()] = total;
    *n_blocks = members.size(), *out_bytes = total;
    return BMU_OK;
}

int bmu_create(int32_t device, bmu_ctx **out) {
    if (!out) return fail(BMU_ERR_ARG, "bmu_create: null argument");
    *out = nullptr;
    int n_dev = 0;
    HIP_TRY(hipGetDeviceCount(&n_dev));
    if (device < 0 || device >= n_dev) return fail(BMU_ERR_HIP, "device %d not available (%d HIP devices)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if ((size_t)prop.sharedMemPerBlock < sizeof(bmu::Shared))
        return fail(BMU_ERR_HIP, "device %d offers %zu bytes of LDS per workgroup, the inflater needs %zu", device,
                    (size_t)prop.sharedMemPerBlock, sizeof(bmu::Shared));
    bmu_ctx *c = new bmu_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e != hipSuccess) {
        bmu_destroy(c);
        return fail(BMU_ERR_HIP, "bmu_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return BMU_OK;
}

void bmu_destroy(bmu_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    c->in.release(); c->out.release(); c->payload_at.release(); c->out_offset.release(); c->payload_len.release(); c->result.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int bmu_inflate(bmu_ctx *c, const uint8_t *in, uint64_t n_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes) {
    if (!c || !out_bytes || (n_bytes && !in)) return fail(BMU_ERR_ARG, "bmu_inflate: null argument");
    *out_bytes = 0;
    c->ms_kernels = 0.f;
    c->n_type[0] = c->n_type[1] = c->n_type[2] = 0;
    c->bad_block = UINT64_MAX, c->bad_reason = 0;
    std::string error;
    if (!bm::bgzf_layout(in, n_bytes, c->members, error)) return fail(BMU_ERR_FORMAT, "%s", error.c_str());
    const size_t n_blocks = c->members.size();
    if (n_blocks > 0x7FFFFFFFull) return fail(BMU_ERR_ARG, "bmu_inflate: %zu blocks in one call", n_blocks);
    c->h_payload_at.resize(n_blocks);
    c->h_payload_len.resize(n_blocks);
    c->h_out_offset.assign(n_blocks + 1, 0);
    for (size_t b = 0; b < n_blocks; b++) {
        c->h_payload_at[b] = c->members[b].payload;
        c->h_payload_len[b] = c->members[b].payload_len;
        c->h_out_offset[b + 1] = c->h_out_offset[b] + c->members[b].isize;
    }
    const uint64_t total = c->h_out_offset[n_blocks];
    if (out_cap < total)
        return fail(BMU_ERR_ARG, "bmu_inflate: out holds %llu bytes, the blocks inflate to %llu", (unsigned long long)out_cap,
                    (unsigned long long)total);
    if (total && !out) return fail(BMU_ERR_ARG, "bmu_inflate: null argument");
    if (n_blocks == 0) return BMU_OK;

    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->in.need((size_t)n_bytes));
    HIP_TRY(c->out.need((size_t)total));
    HIP_TRY(c->payload_at.need(n_blocks));
    HIP_TRY(c->payload_len.need(n_blocks));
    HIP_TRY(c->out_offset.need(n_blocks + 1));
    HIP_TRY(c->result.need(n_blocks));
    HIP_TRY(hipMemcpyAsync(c->in.p, in, (size_t)n_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->payload_at.p, c->h_payload_at.data(), n_blocks * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->payload_len.p, c->h_payload_len.data(), n_blocks * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->out_offset.p, c->h_out_offset.data(), (n_blocks + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    hipLaunchKernelGGL(bmu::inflate_kernel, dim3((uint32_t)n_blocks), dim3(bmu::kThreads), 0, c->stream, c->in.p, c->payload_at.p,
                       c->payload_len.p, c->out_offset.p, c->out.p, c->result.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    c->h_result.resize(n_blocks);
    HIP_TRY(hipMemcpyAsync(c->h_result.data(), c->result.p, n_blocks * sizeof(bmu::Result), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&c->ms_kernels, c->ev0, c->ev1));
    for (size_t b = 0; b < n_blocks; b++) {
        const bmu::Result &r = c->h_result[b];
        if (r.reason && c->bad_block == UINT64_MAX) c->bad_block = b, c->bad_reason = r.reason;
        for (int k = 0; k < 3; k++) c->n_type[k] += r.n_type[k];
    }
    if (c->bad_block != UINT64_MAX)
        return fail(BMU_ERR_DATA, "BGZF block %llu (at byte %llu) is bad: %s", (unsigned long long)c->bad_block,
                    (unsigned long long)c->members[c->bad_block].at, bm::inflate_reason_text(c->bad_reason));
    if (total) {
        HIP_TRY(hipMemcpyAsync(out, c->out.p, (size_t)total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *out_bytes = total;
    return BMU_OK;
}

int bmu_bad_block(bmu_ctx *c, uint64_t *block, uint32_t *reason) {
    if (!c) return fail(BMU_ERR_ARG, "bmu_bad_block: null argument");
    if (block) *block = c->bad_block;
    if (reason) *reason = c->bad_reason;
    return BMU_OK;
}

int bmu_last_stats(bmu_ctx *c, float *ms_kernels, uint64_t *n_stored, uint64_t *n_fixed, uint64_t *n_dynamic) {
    if (!c) return fail(BMU_ERR_ARG, "bmu_last_stats: null argument");
    if (ms_kernels) *ms_kernels = c->ms_kernels;
    if (n_stored) *n_stored = c->n_type[0];
    if (n_fixed) *n_fixed = c->n_type[1];
    if (n_dynamic) *n_dynamic = c->n_type[2];
    return BMU_OK;
}

}  // extern "C"
