// bms_ctx.hip.h -- the sorter's context and its device-side entries, shared by bms_api.hip (which owns both) and
// bmd_api.hip (whose marked stream is sorted and deflated where it lies, and whose own sorts are the same radix passes).
// Not part of the C ABI of include/bms.h.  The upload is split from the launches so that a caller may work on the device
// copy between the two.  Every entry enqueues on the compressor's stream; on failure the message is in bms_last_error().
#pragma once

#include "../../include/bms.h"

#include "bmz_ctx.hip.h"

struct bms_ctx {
    bmz_ctx *z = nullptr;                   // owns the device, the stream and the deflate
    uint32_t n_cu = 1;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // keys+hist | passes | gather: begin, end
    bmhip::DevBuf<uint8_t> in, sorted;
    bmhip::DevBuf<uint64_t> rec_offset, sorted_offset, key[2], scan_tmp64;
    bmhip::DevBuf<uint32_t> index[2], length, perm_length, counts, place, scan_tmp32, hist;
    float ms_sort = 0.f, ms_gather = 0.f, ms_deflate = 0.f;
    uint32_t n_passes = 0;
};


// what every entry point that takes a stream checks of it, without a device
int bms_check_stream(const char *who, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records);

// room for a stable sort of n (key, index) pairs: key[0..1], index[0..1], the tile counts and their scan, the digit counts
int bms_need_radix(bms_ctx *c, uint32_t n, uint64_t n_bytes);

// every buffer of a sort of n records in n_bytes of stream; makes the context's device current
int bms_need_sort(bms_ctx *c, uint32_t n, uint64_t n_bytes);

// the stream and its offsets to c->in and c->rec_offset (bms_need_sort has run)
int bms_upload_stream(bms_ctx *c, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint32_t n);

// The n keys of c->key[*side] with their companions c->index[*side], sorted stably by the whole key: the digit counts in
// one pass, read by the host (this waits for the stream), then one count / scan / scatter pass per digit on which the keys
// differ.  *side names the buffers that hold the result; *n_passes grows by the passes that ran.  The events, where given,
// are recorded after the histogram and around the passes.
int bms_radix_sort(bms_ctx *c, uint32_t n, int *side, uint32_t *n_passes, hipEvent_t ev_hist_end = nullptr, hipEvent_t ev_pass_begin = nullptr,
                   hipEvent_t ev_pass_end = nullptr);

// the records of c->in[0, n_bytes) (offsets in c->rec_offset) in order: c->sorted, c->index[*final_side] (perm) and
// c->sorted_offset on the device
int bms_sort_on_device(bms_ctx *c, uint64_t n_bytes, uint32_t n, int *final_side);

// the events of bms_sort_on_device into ms_sort and ms_gather; the stream has been waited for
int bms_read_times(bms_ctx *c);
void bms_reset_stats(bms_ctx *c);
