// bm_hip_util.h -- the host plumbing shared by the three translation units of libbmf.so (filter, locator, verifier).
#pragma once

#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

namespace bmhip {

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to (kernel, device), not to a context: several contexts --
// one per host thread with --gpus, possibly on the same device -- launch the same kernels with different LDS
// sizes.  Only ever raise it, under a lock, so that no context lowers it between another one's call and launch.
inline hipError_t raise_dynamic_lds(const void *fn, size_t bytes) {
    static std::mutex mu;
    static std::vector<std::tuple<const void *, int, size_t>> seen;
    int dev = 0;
    hipError_t r = hipGetDevice(&dev);
    if (r != hipSuccess) return r;
    std::lock_guard<std::mutex> lock(mu);
    for (auto &e : seen)
        if (std::get<0>(e) == fn && std::get<1>(e) == dev) {
            if (bytes <= std::get<2>(e)) return hipSuccess;
            r = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (r == hipSuccess) std::get<2>(e) = bytes;
            return r;
        }
    r = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (r == hipSuccess) seen.emplace_back(fn, dev, bytes);
    return r;
}

// A large upload from ORDINARY host memory that lies in pieces (the records of a genome, each a buffer of its own; one
// record for a flat buffer): hipMemcpy from pageable memory stages through the runtime's own small buffers on one thread
// (4-6 GB/s: 0.3 s for a 1.7 Gbp genome); here the records go to dst back to back, in order, through two page-locked
// 32 MiB buffers, filled by a few threads while the buffer before is on the link -- no flattened copy on the host.
// Synchronous: returns when the data is there.
inline hipError_t upload_pageable_records(void *dst, const uint8_t *const *rec, const uint64_t *rec_len, uint32_t n_records) {
    constexpr size_t kPiece = 32u << 20;
    uint64_t total = 0;
    for (uint32_t r = 0; r < n_records; r++) total += rec_len[r];
    if (total < 2 * kPiece) {                                           // small: not worth the staging
        hipError_t e = hipSuccess;
        uint64_t at = 0;
        for (uint32_t r = 0; r < n_records && e == hipSuccess; at += rec_len[r], r++)
            if (rec_len[r]) e = hipMemcpy(static_cast<char *>(dst) + at, rec[r], (size_t)rec_len[r], hipMemcpyHostToDevice);
        return e;
    }
    void *stage[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    hipStream_t stream = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = hipHostMalloc(&stage[i], kPiece, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&done[i], hipEventDisableTiming);
    }
    const unsigned threads = std::max(1u, std::min(3u, std::thread::hardware_concurrency() / 2u));
    uint32_t r = 0;                 // the record and the offset in it where the next piece begins
    uint64_t in_r = 0;
    size_t piece = 0;
    for (uint64_t at = 0; e == hipSuccess && at < total; at += kPiece, piece++) {
        const int slot = (int)(piece & 1);
        const size_t n = (size_t)std::min<uint64_t>(kPiece, total - at);
        if (piece >= 2) e = hipEventSynchronize(done[slot]);           // the buffer's previous copy has left it
        if (e != hipSuccess) break;
        // the stretches of records that make up this piece
        struct Part { const uint8_t *src; size_t to, len; };
        std::vector<Part> parts;
        for (size_t filled = 0; filled < n;) {
            while (in_r == rec_len[r]) {
                r++;
                in_r = 0;
            }
            const size_t take = (size_t)std::min<uint64_t>(rec_len[r] - in_r, n - filled);
            parts.push_back(Part{rec[r] + in_r, filled, take});
            filled += take;
            in_r += take;
        }
        // ... copied by a few threads, each a contiguous share of the piece's bytes (a page-cache or heap source into a
        // page-locked buffer runs at 5-8 GB/s per thread)
        auto share = [&](unsigned t) {
            const size_t lo = n * t / threads, hi = n * (t + 1) / threads;
            for (const Part &p : parts) {
                const size_t a = std::max(lo, p.to), b = std::min(hi, p.to + p.len);
                if (a < b) std::memcpy(static_cast<char *>(stage[slot]) + a, p.src + (a - p.to), b - a);
            }
        };
        if (threads <= 1 || n < (4u << 20)) {
            for (unsigned t = 0; t < threads; t++) share(t);
        } else {
            std::vector<std::thread> pool;
            for (unsigned t = 1; t < threads; t++) pool.emplace_back(share, t);
            share(0);
            for (auto &t : pool) t.join();
        }
        e = hipMemcpyAsync(static_cast<char *>(dst) + at, stage[slot], n, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipEventRecord(done[slot], stream);
    }
    if (stream) {
        const hipError_t s = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = s;
    }
    for (int i = 0; i < 2; i++) {
        if (done[i]) (void)hipEventDestroy(done[i]);
        if (stage[i]) (void)hipHostFree(stage[i]);
    }
    if (stream) (void)hipStreamDestroy(stream);
    return e;
}

// Grow-only buffers: a context or batch that is used again keeps its allocations.  need(n) leaves headroom (batches of a
// file differ a little in size), need_exact(n) takes what is asked; either holds at least one element.  DevBuf lives in
// device memory; PinnedBuf is page-locked host memory, staging for asynchronous copies.  `cap` counts elements.
// A buffer owns its memory: it frees it when it goes (so a context's `delete` releases every buffer it holds, with the
// context's device current), moves and does not copy.  None may have static storage: it would free after the runtime is gone.
template <typename T, bool kPinned>
struct GrowBuf {
    T *p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    ~GrowBuf() { release(); }
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    GrowBuf(GrowBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    GrowBuf &operator=(GrowBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    hipError_t need(size_t n) {
        const size_t bytes = n * sizeof(T);
        return grow(n, kPinned ? bytes + bytes / 8 + 64 : ((n ? n : 1) + n / 8) * sizeof(T));
    }
    hipError_t need_exact(size_t n) { return grow(n, (n ? n : 1) * sizeof(T)); }
    void release() {
        if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }

  private:
    hipError_t grow(size_t n, size_t bytes) {
        if (n <= cap && p) return hipSuccess;
        release();
        void *q = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
        if (e == hipSuccess) {
            p = static_cast<T *>(q);
            cap = bytes / sizeof(T);
        }
        return e;
    }
};
template <typename T>
using DevBuf = GrowBuf<T, false>;
template <typename T>
using PinnedBuf = GrowBuf<T, true>;

// SeqAn3 dna4 assign_char folding; built once, uploaded per context.
inline void build_dna4_lut(uint8_t *lut) {
    std::memset(lut, 0, 256);
    const char *m[4] = {"AaRrWwMmDdHhVv", "CcYySsBb", "GgKk", "TtUu"};
    for (int r = 0; r < 4; r++)
        for (const char *c = m[r]; *c; c++) lut[(uint8_t)*c] = (uint8_t)r;
}

}  // namespace bmhip

// Error reporting of the C ABIs.  The slot lies in an anonymous namespace, so every translation unit that includes this
// header -- bmf_api.hip, bml_api.hip, bmv_api.hip -- has its own: bmf_last_error() still reports the filter's last
// failure after the locator has failed.  Each file defines HIP_TRY(e) as BM_HIP_TRY(e, <its library's HIP error code>).
namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace

#define BM_HIP_TRY(expr, code)                                                                                \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return fail(code, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
