// bmz_ctx.hip.h -- the compressor's context and its device-side entry, shared by bmz_api.hip (which owns both) and
// bms_api.hip (whose sorted stream is deflated where it lies).  Not part of the C ABI of include/bmz.h.
#pragma once

#include "../../include/bmz.h"

#include "bm_hip_util.h"

struct bmz_ctx {
    int device = 0;
    uint32_t n_cu = 1;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bmhip::DevBuf<uint8_t> in, stage, out, forms;
    bmhip::DevBuf<uint32_t> tokens, sizes;
    bmhip::DevBuf<uint64_t> offsets, scan_tmp;
    std::vector<uint64_t> h_offsets{0};
    float ms_kernels = 0.f;
    uint32_t n_form[3] = {0, 0, 0};
};

// bmz_deflate from the upload on: d_in[0, n_bytes) lies on the context's device (8 readable bytes of padding behind it) and
// whatever wrote it was enqueued on ctx->stream.  The arguments are bmz_deflate's and have passed its checks; n_bytes > 0.
// On failure the message is in bmz_last_error().
int bmz_deflate_device(bmz_ctx *ctx, const uint8_t *d_in, uint64_t n_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap,
                       uint64_t *out_bytes);
