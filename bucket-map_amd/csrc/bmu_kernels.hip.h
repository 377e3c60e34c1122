// bmu_kernels.hip.h -- BGZF blocks inflated on gfx950: a full RFC 1951 decoder, one wavefront (a workgroup of 64 threads)
// per BGZF block, the grid as long as the call has blocks.
//
// Form.  The Huffman decode of a block is serial, so the parallelism comes from blocks (a million 300-bp reads are about
// 10 000 of them) and, inside a block, from the lanes that are not decoding:
//   decode   lane 0 runs the shared lines of host/inflate_rule.h -- block headers, table construction with its checks,
//            single-symbol decode -- with both tables and a 4 KiB window of the payload in LDS.  It decodes a batch of up
//            to 64 tokens (literal, or length and distance, each with its output position) into LDS and checks every
//            token against the output written so far and against ISIZE, so no later step can leave the block.
//   window   the whole wavefront slides the payload window forward from global memory whenever less than 1 KiB of it is
//            ahead (a dynamic header takes at most 0.6 KiB, a token 6 bytes).
//   write    the wavefront writes the batch: all literals at once, then the matches in order, 64 bytes a step.
//            A match with distance d < 64 is a periodic run: lane i reads out[p - d + i % d], bytes that lie BEFORE the
//            match, so no lane reads what a lane of the same step writes.  With d >= 64 step s reads bytes below
//            p + 64 s, which the steps before wrote.  A match whose source is an earlier token of the same batch finds it
//            written: the literals go first, the matches in order, a barrier after each.
//   stored   a stored block is copied by the wavefront straight from global memory.
//   crc      a slice per lane from a zero register, combined by x^(8k) mod P (the CRC is linear), against the trailer.
//
// The output window is the block's whole text, at most 64 KiB, IN LDS: matches read back what the same wavefront wrote
// through LDS, which is in order for a wavefront (and fenced by the barriers), so no argument about the visibility of
// global stores is needed.  Text leaves for global memory once, after the CRC, in coalesced stores.  64 KiB of text and
// 11 KiB of tables and buffers leave two workgroups per CU (160 KiB of LDS).
//
// Bounds.  Every output index is below ISIZE <= 65536 (checked by lane 0 before the token enters the batch), every payload
// index below the payload's length (the window is filled up to the end and no further; the bit reader feeds zeros beyond
// and the overrun ends in BMU_REASON_TRUNCATED).  The outer loop makes progress every turn -- a token, a block header or a
// slide -- and is capped besides.
#pragma once

#include "../host/inflate_rule.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmu {

constexpr uint32_t kThreads = 64, kWindow = 4096, kMargin = 1024, kBatch = 64, kOutMax = 65536;
constexpr uint32_t kMaxTurns = 1u << 18;     // a payload of 64 KiB holds fewer tokens, headers and slides than this

constexpr uint32_t kCrcPoly = 0xEDB88320u;

// a * b mod P in the reflected representation (bit 31 = x^0), and x^(8k) mod P: as in bmz_kernels.hip.h
__device__ __forceinline__ uint32_t mul_mod_p(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t x_pow_8(uint32_t k) {
    uint32_t p = 1u << 31, sq = 1u << 30;
    for (int i = 0; i < 3; i++) sq = mul_mod_p(sq, sq);
    for (; k; k >>= 1) {
        if (k & 1u) p = mul_mod_p(sq, p);
        sq = mul_mod_p(sq, sq);
    }
    return p;
}

struct Shared {
    uint8_t out[kOutMax];
    uint8_t win[kWindow];
    bmu_rule::Tables T;
    uint32_t tok[kBatch], pos[kBatch];
    uint32_t crc_table[256];
    uint32_t n_tok, copy_src, copy_dst, copy_len, next, done, reason, crc;
};

// what a block reports: the reason (0 = fine) and its DEFLATE blocks by type
struct Result {
    uint32_t reason, n_type[3];
};

__global__ __launch_bounds__(kThreads) void inflate_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ payload_at,
                                                          const uint32_t *__restrict__ payload_len, const uint64_t *__restrict__ out_offset,
                                                          uint8_t *__restrict__ out, Result *__restrict__ result) {
    using namespace bmu_rule;
    __shared__ Shared S;
    const uint32_t t = threadIdx.x, blk = blockIdx.x;
    const uint8_t *const src = in + payload_at[blk];
    const uint32_t end = payload_len[blk];
    const uint32_t isize = (uint32_t)(out_offset[blk + 1] - out_offset[blk]);     // <= kOutMax: the layout checked it
    for (uint32_t i = t; i < 256; i += kThreads) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        S.crc_table[i] = c;
    }
    if (t == 0) S.n_tok = 0, S.copy_len = 0, S.next = 0, S.done = 0, S.reason = 0, S.crc = 0;

    // lane 0's state; the other lanes carry copies they never use
    BitReader br;
    br.buf = S.win, br.end = end;
    uint32_t in_codes = 0, bfinal = 0, at = 0, n_type[3] = {0, 0, 0};
    uint32_t w_base = 0, w_limit = 0;
    bool first = true;
    __syncthreads();

    for (uint32_t turn = 0;; turn++) {
        // ---- window ----
        const uint32_t nx = S.next;
        if (first || (w_limit < end && nx + kMargin > w_limit)) {
            first = false;
            w_base = min(nx, end);
            w_limit = min(end, w_base + kWindow);
            for (uint32_t i = t; i < w_limit - w_base; i += kThreads) S.win[i] = src[w_base + i];
            __syncthreads();
        }
        br.base = w_base, br.limit = w_limit;

        // ---- decode: lane 0 ----
        if (t == 0) {
            uint32_t reason = turn >= kMaxTurns ? (uint32_t)kTruncated : (uint32_t)kOk, n_tok = 0, done = 0;
            S.copy_len = 0;
            if (!reason && !in_codes) {                                   // a block header: the margin is there
                br.refill();
                bfinal = br.bits(1);
                const uint32_t btype = br.bits(2);
                if (br.overrun()) reason = kTruncated;
                else if (btype == 3) reason = kBadType;
                else if (btype == 0) {
                    uint32_t start = 0, len = 0;
                    reason = read_stored_header(br, &start, &len);
                    if (!reason && len > isize - at) reason = kTooLong;
                    if (!reason) {
                        S.copy_src = start, S.copy_dst = at, S.copy_len = len;
                        at += len;
                        done = bfinal;
                    }
                } else {
                    reason = btype == 1 ? build_fixed(S.T) : read_dynamic_header(S.T, br);
                    in_codes = 1;
                }
                if (!reason) n_type[btype]++;
            }
            if (!reason && in_codes) {
                while (n_tok < kBatch && (br.limit >= end || br.next + 8 <= br.limit)) {
                    uint32_t tok = 0;
                    const int32_t r = next_token(S.T, br, &tok);
                    if (r < 0) {
                        reason = (uint32_t)(-r);
                        break;
                    }
                    if (r == kEndOfBlock) {
                        in_codes = 0;
                        done = bfinal;
                        break;
                    }
                    const uint32_t len = (tok & kTokMatch) ? (tok >> 16) & 0x1FFu : 1u;
                    if ((tok & kTokMatch) && (tok & 0xFFFFu) > at) {
                        reason = kDistance;
                        break;
                    }
                    if (len > isize - at) {
                        reason = kTooLong;
                        break;
                    }
                    S.tok[n_tok] = tok, S.pos[n_tok] = at;
                    n_tok++;
                    at += len;
                }
            }
            if (!reason && done && at != isize) reason = kTooShort;
            S.n_tok = reason ? 0u : n_tok;
            if (reason) S.copy_len = 0;
            S.next = br.next, S.done = done | (reason != 0), S.reason = reason;
        }
        __syncthreads();

        // ---- write: the wavefront ----
        const uint32_t n_tok = S.n_tok, copy_len = S.copy_len;
        if (copy_len) {
            const uint32_t from = S.copy_src, to = S.copy_dst;           // from + len <= end, to + len <= isize
            for (uint32_t i = t; i < copy_len; i += kThreads) S.out[to + i] = src[from + i];
        }
        if (n_tok) {
            const uint32_t tok = t < n_tok ? S.tok[t] : 0u, p = t < n_tok ? S.pos[t] : 0u;
            const bool is_match = (tok & kTokMatch) != 0;
            if (t < n_tok && !is_match) S.out[p] = (uint8_t)tok;
            __syncthreads();
            for (uint64_t m = __ballot(is_match); m; m &= m - 1) {
                const int k = __ffsll((unsigned long long)m) - 1;
                const uint32_t mt = __shfl(tok, k), mp = __shfl(p, k);
                const uint32_t len = (mt >> 16) & 0x1FFu, d = mt & 0xFFFFu;   // 1 <= d <= mp, mp + len <= isize
                if (d < kThreads) {
                    for (uint32_t i = t; i < len; i += kThreads) S.out[mp + i] = S.out[mp - d + i % d];
                } else {
                    for (uint32_t i0 = 0; i0 < len; i0 += kThreads) {
                        if (i0 + t < len) S.out[mp + i0 + t] = S.out[mp + i0 + t - d];
                        if (d < len) __syncthreads();
                    }
                }
                __syncthreads();
            }
        }
        const uint32_t done = S.done;
        __syncthreads();                                                 // S.* may be written again
        if (done) break;
    }

    // ---- crc, and the text to global memory ----
    uint32_t reason = S.reason;
    if (!reason) {
        const uint32_t slice = (isize + kThreads - 1) / kThreads;
        const uint32_t b0 = min(isize, t * slice), b1 = min(isize, b0 + slice);
        uint32_t c = 0;
        for (uint32_t i = b0; i < b1; i++) c = S.crc_table[(c ^ S.out[i]) & 0xFFu] ^ (c >> 8);
        if (c) atomicXor(&S.crc, mul_mod_p(c, x_pow_8(isize - b1)));
        __syncthreads();
        const uint32_t crc = S.crc ^ mul_mod_p(0xFFFFFFFFu, x_pow_8(isize)) ^ 0xFFFFFFFFu;
        const uint8_t *tail = src + end;                                 // the trailer: inside the buffer by the layout
        const uint32_t want = tail[0] | (uint32_t)tail[1] << 8 | (uint32_t)tail[2] << 16 | (uint32_t)tail[3] << 24;
        if (crc != want) reason = kCrc;
    }
    if (!reason) {
        uint8_t *const dst = out + out_offset[blk];
        // dwords where the destination allows: head bytes up to its alignment, then four LDS bytes a store
        const uint32_t head = min(isize, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
        if (t < head) dst[t] = S.out[t];
        const uint32_t words = (isize - head) / 4;
        for (uint32_t w = t; w < words; w += kThreads) {
            const uint8_t *q = S.out + head + 4 * w;
            *reinterpret_cast<uint32_t *>(dst + head + 4 * w) = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        }
        const uint32_t rest = head + 4 * words;
        if (rest + t < isize) dst[rest + t] = S.out[rest + t];
    }
    if (t == 0) {
        Result r;
        r.reason = reason;
        for (int k = 0; k < 3; k++) r.n_type[k] = n_type[k];
        result[blk] = r;
    }
}

}  // namespace bmu
