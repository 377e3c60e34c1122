// bmz_kernels.hip.h -- BGZF blocks deflated on gfx950: the rule of include/bmz.h, one workgroup of 256 threads per block,
// a persistent grid (one workgroup per CU: the hash table alone takes 128 KiB of the CU's 160 KiB LDS).
//
// Per block:
//   parse    a step of T = 256 positions at a time: every thread looks its position up in the LDS table (as the steps
//            before left it) and measures the match 8 bytes a time from global memory; after a barrier the step's
//            positions enter the table by LDS max atomics ("greatest wins": the race has one outcome).  The greedy chain
//            through the step is marked by pointer doubling over the step's 256 `next` values (8 rounds); the marked
//            positions take their token slots by ballot ranks and count themselves into the LDS histograms.
//   codes    ranks by (count, symbol) in parallel, the two-queue merge, the Kraft fix-up and the dealing on one lane.
//   emit     every thread takes a contiguous share of the tokens: a block scan of the shares' bit counts, then the bits
//            are ORed into the block's zeroed staging slot by 32-bit atomics (plain vector memory instructions).
//   crc      a slice per thread from a zero register, combined by x^(8k) mod P (the CRC is linear).
// A second kernel gathers the slots to their packed places (offsets by bm_scan.hip.h over the block sizes).
#pragma once

#include "bm_scan.hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmz {

constexpr uint32_t kThreads = 256, kT = 256, kHashBits = 15, kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr uint32_t kBlockMax = 65280;
constexpr uint32_t kSlotPad = 2;     // a block starts 2 bytes into its slot, so that its payload (18 bytes on) is 4-aligned
constexpr uint32_t kCrcPoly = 0xEDB88320u;

__host__ __device__ inline uint32_t slot_stride(uint32_t block_bytes) { return (kSlotPad + block_bytes + 31 + 3 + 4) & ~3u; }

__device__ static const uint16_t d_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ static const uint8_t d_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ static const uint8_t d_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Shared {
    uint32_t table[1u << kHashBits];   // position + 1 of the greatest position with this hash, 0 = none
    uint32_t ll_freq[288], d_freq[32], cl_freq[20];
    uint32_t w[2 * 286];               // code construction: node weights
    uint16_t parent[2 * 286], depth[2 * 286], order[288];
    uint32_t count[16];
    uint8_t ll_len[288], d_len[32], cl_len[20];
    uint16_t ll_code[288], d_code[32], cl_code[20];
    uint8_t len_sym[kMaxMatch + 2];    // match length -> length symbol - 257
    uint16_t jump[2][kT];
    uint32_t mark[kT];
    uint32_t wave_count[kThreads / 64];
    uint32_t scan_ws[kThreads / 64 + 1];
    uint32_t crc_table[256];
    uint32_t p_start, crc, fixed_bits, dyn_bits, extra_bits, hlit, hdist, hclen, form, payload;
};

__device__ __forceinline__ uint32_t load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t load64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// common prefix of a[0, cap) and b[0, cap); reads nothing beyond cap
__device__ __forceinline__ uint32_t match_length(const uint8_t *a, const uint8_t *b, uint32_t cap) {
    uint32_t len = 0;
    while (len + 8 <= cap) {
        const uint64_t x = load64(a + len) ^ load64(b + len);
        if (x) return len + ((uint32_t)__ffsll((unsigned long long)x) - 1u) / 8u;
        len += 8;
    }
    while (len < cap && a[len] == b[len]) len++;
    return len;
}

__device__ __forceinline__ uint32_t dist_sym(uint32_t dist, uint32_t *extra_bits, uint32_t *extra) {
    const uint32_t x = dist - 1;
    if (x < 4) {
        *extra_bits = 0, *extra = 0;
        return x;
    }
    const uint32_t nb = 31u - (uint32_t)__clz((int)x);
    *extra_bits = nb - 1;
    *extra = x & ((1u << (nb - 1)) - 1u);
    return 2 * nb + ((x >> (nb - 1)) & 1u);
}

// a * b mod P in the reflected representation (bit 31 = x^0)
__device__ __forceinline__ uint32_t mul_mod_p(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
// x^(8k) mod P
__device__ __forceinline__ uint32_t x_pow_8(uint32_t k) {
    uint32_t p = 1u << 31, sq = 1u << 30;
    for (int i = 0; i < 3; i++) sq = mul_mod_p(sq, sq);
    for (; k; k >>= 1) {
        if (k & 1u) p = mul_mod_p(sq, p);
        sq = mul_mod_p(sq, sq);
    }
    return p;
}

// The code construction of include/bmz.h for freq[0, n_sym) -> lens.  Called by the whole workgroup; ends on a barrier.
__device__ void build_lengths(Shared &S, const uint32_t *freq, uint32_t n_sym, uint32_t max_bits, uint8_t *lens) {
    const uint32_t t = threadIdx.x;
    for (uint32_t s = t; s < n_sym; s += kThreads) {
        lens[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        uint32_t r = 0;
        for (uint32_t u = 0; u < n_sym; u++) {
            const uint32_t fu = freq[u];
            r += (fu && (fu < f || (fu == f && u < s))) ? 1u : 0u;
        }
        S.order[r] = (uint16_t)s;
        S.w[r] = f;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t m = 0;
        for (uint32_t u = 0; u < n_sym; u++) m += freq[u] ? 1u : 0u;
        if (m <= 1) {
            lens[m ? S.order[0] : 0] = 1;
        } else {
            uint32_t a = 0, q = m, nxt = m;
            for (uint32_t k = 0; k + 1 < m; k++) {
                uint32_t pair[2];
                for (int j = 0; j < 2; j++) pair[j] = (a < m && (q >= nxt || S.w[a] <= S.w[q])) ? a++ : q++;
                S.w[nxt] = S.w[pair[0]] + S.w[pair[1]];
                S.parent[pair[0]] = S.parent[pair[1]] = (uint16_t)nxt;
                nxt++;
            }
            S.depth[2 * m - 2] = 0;
            for (uint32_t node = 2 * m - 2; node-- > 0;) S.depth[node] = (uint16_t)(S.depth[S.parent[node]] + 1);
            for (uint32_t l = 0; l < 16; l++) S.count[l] = 0;
            for (uint32_t leaf = 0; leaf < m; leaf++) S.count[min((uint32_t)S.depth[leaf], max_bits)]++;
            uint32_t kraft = 0;
            for (uint32_t l = 1; l <= max_bits; l++) kraft += S.count[l] << (max_bits - l);
            while (kraft > (1u << max_bits)) {
                uint32_t bits = max_bits - 1;
                while (bits && S.count[bits] == 0) bits--;
                if (!bits) break;                                 // (cannot happen: at most 286 leaves, K counts them all)
                S.count[bits]--;
                S.count[bits + 1] += 2;
                S.count[max_bits]--;
                kraft--;
            }
            uint32_t at = 0;
            for (uint32_t l = max_bits; l >= 1; l--)
                for (uint32_t k = 0; k < S.count[l]; k++) lens[S.order[at++]] = (uint8_t)l;
        }
    }
    __syncthreads();
}

// RFC 1951 3.2.2 on one lane; the codes bit-reversed as they enter the stream
__device__ void canonical(const uint8_t *lens, uint32_t n_sym, uint16_t *codes) {
    uint32_t count[17], next[17], code = 0;
    for (int l = 0; l < 17; l++) count[l] = 0, next[l] = 0;
    for (uint32_t s = 0; s < n_sym; s++)
        if (lens[s]) count[lens[s]]++;
    for (uint32_t l = 1; l <= 15; l++) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    for (uint32_t s = 0; s < n_sym; s++) {
        const uint32_t l = lens[s];
        codes[s] = l ? (uint16_t)(__brev(next[l]++) >> (32 - l)) : (uint16_t)0;
    }
}

struct BitOut {
    uint32_t *words;
    uint64_t acc = 0;
    uint32_t have, at, limit;          // limit: the words of the slot from the payload on (no write ever leaves the slot)
    __device__ BitOut(uint32_t *w, uint32_t bit_offset, uint32_t n_words) : words(w), have(bit_offset & 31u), at(bit_offset >> 5), limit(n_words) {}
    __device__ __forceinline__ void put(uint32_t value, uint32_t bits) {   // bits <= 16
        acc |= (uint64_t)value << have;
        have += bits;
        if (have >= 32) {
            if (at < limit) atomicOr(&words[at], (uint32_t)acc);
            at++;
            acc >>= 32;
            have -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if (have && (uint32_t)acc && at < limit) atomicOr(&words[at], (uint32_t)acc);
    }
};

// a token: a literal is its byte; a match is bit 31 | length << 15 | distance - 1
__device__ __forceinline__ uint32_t token_bits(const Shared &S, uint32_t tok) {
    if (tok >> 31) {
        const uint32_t s = S.len_sym[(tok >> 15) & 0x1FFu];
        uint32_t eb, ev;
        const uint32_t ds = dist_sym((tok & 0x7FFFu) + 1, &eb, &ev);
        return S.ll_len[257 + s] + d_len_extra[s] + S.d_len[ds] + eb;
    }
    return S.ll_len[tok];
}

// stage: n_blocks slots of slot_stride(block_bytes) bytes, ZEROED by the caller; tokens: gridDim.x * kBlockMax entries
__global__ __launch_bounds__(kThreads) void deflate_kernel(const uint8_t *__restrict__ in, uint64_t n_bytes, uint32_t block_bytes,
                                                          uint32_t n_blocks, uint8_t *__restrict__ stage, uint32_t *__restrict__ tokens,
                                                          uint32_t *__restrict__ sizes, uint8_t *__restrict__ forms) {
    __shared__ Shared S;
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    {
        uint32_t c = t;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        S.crc_table[t] = c;
        for (uint32_t len = 3 + t; len <= kMaxMatch; len += kThreads) {
            uint32_t s = 28;
            while (d_len_base[s] > len) s--;
            S.len_sym[len] = (uint8_t)s;
        }
    }
    uint32_t *const tok = tokens + (size_t)blockIdx.x * kBlockMax;
    const uint32_t stride = slot_stride(block_bytes), slot_words = (stride - kSlotPad - 18) / 4;

    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint8_t *const src = in + (uint64_t)blk * block_bytes;
        const uint32_t n = (uint32_t)min((uint64_t)block_bytes, n_bytes - (uint64_t)blk * block_bytes);
        uint8_t *const dst = stage + (size_t)blk * stride + kSlotPad;
        uint32_t *const payload_words = reinterpret_cast<uint32_t *>(dst + 18);

        __syncthreads();                                         // the block before is done with S
        for (uint32_t i = t; i < (1u << kHashBits); i += kThreads) S.table[i] = 0;
        for (uint32_t i = t; i < 288; i += kThreads) S.ll_freq[i] = 0;
        if (t < 32) S.d_freq[t] = 0;
        if (t < 20) S.cl_freq[t] = 0;
        if (t == 0) S.p_start = 0, S.crc = 0, S.fixed_bits = 0, S.dyn_bits = 0, S.extra_bits = 0, S.ll_len[286] = 0, S.ll_len[287] = 0;
        __syncthreads();

        // ---- parse ----
        uint32_t n_tok = 0;
        for (uint32_t lo = 0; lo < n; lo += kT) {
            const uint32_t i = lo + t;
            uint32_t h = 0, len = 0, dist = 0;
            const bool hashed = i + 4 <= n;
            if (hashed) {
                h = (load32(src + i) * 2654435761u) >> (32 - kHashBits);
                const uint32_t c1 = S.table[h];
                if (c1 && i - (c1 - 1) <= kMaxDist) {
                    dist = i - (c1 - 1);
                    len = match_length(src + (c1 - 1), src + i, min(kMaxMatch, n - i));
                }
            }
            const uint32_t adv = len >= kMinMatch ? len : 1u;
            const uint32_t start = S.p_start;                    // (written before the barrier that ended the step before)
            S.jump[0][t] = (uint16_t)((i < n && t + adv < kT) ? t + adv : kT);
            S.mark[t] = (start == i) ? 1u : 0u;
            __syncthreads();                                     // every lookup of the step is done
            if (hashed) atomicMax(&S.table[h], i + 1);
            for (uint32_t k = 0; k < 8; k++) {
                const uint32_t cur = k & 1u;
                const uint32_t j = S.jump[cur][t];
                if (S.mark[t] && j < kT) S.mark[j] = 1u;         // only positions on the chain are ever marked
                S.jump[cur ^ 1u][t] = (uint16_t)(j < kT ? S.jump[cur][j] : kT);
                __syncthreads();
            }
            const bool on = S.mark[t] != 0 && i < n;
            const unsigned long long ballot = __ballot(on);
            if (lane == 0) S.wave_count[wave] = (uint32_t)__popcll(ballot);
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t wv = 0; wv < kThreads / 64; wv++) {
                const uint32_t cnt = S.wave_count[wv];
                before += wv < wave ? cnt : 0u;
                all += cnt;
            }
            if (on) {
                const uint32_t slot = n_tok + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
                if (len >= kMinMatch) {
                    tok[slot] = 0x80000000u | len << 15 | (dist - 1);
                    uint32_t eb, ev;
                    atomicAdd(&S.ll_freq[257 + S.len_sym[len]], 1u);
                    atomicAdd(&S.d_freq[dist_sym(dist, &eb, &ev)], 1u);
                } else {
                    const uint32_t byte = src[i];
                    tok[slot] = byte;
                    atomicAdd(&S.ll_freq[byte], 1u);
                }
                if (i + adv >= lo + kT) S.p_start = i + adv;     // the one position whose step leaves this step
            }
            n_tok += all;
            __syncthreads();
        }
        if (t == 0) S.ll_freq[256] = 1;
        __syncthreads();

        // ---- codes ----
        build_lengths(S, S.ll_freq, 286, 15, S.ll_len);
        build_lengths(S, S.d_freq, 30, 15, S.d_len);
        if (t == 0) {
            uint32_t hlit = 286, hdist = 30;
            while (!S.ll_len[hlit - 1]) hlit--;
            while (!S.d_len[hdist - 1]) hdist--;
            S.hlit = hlit, S.hdist = hdist;
        }
        __syncthreads();
        for (uint32_t s = t; s < S.hlit; s += kThreads) atomicAdd(&S.cl_freq[S.ll_len[s]], 1u);
        if (t < S.hdist) atomicAdd(&S.cl_freq[S.d_len[t]], 1u);
        __syncthreads();
        build_lengths(S, S.cl_freq, 19, 7, S.cl_len);
        {
            uint32_t fixed = 0, dyn = 0, extra = 0;
            for (uint32_t s = t; s < 286; s += kThreads) {
                const uint32_t f = S.ll_freq[s];
                fixed += f * (s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u);
                dyn += f * S.ll_len[s];
                if (s >= 257) extra += f * d_len_extra[s - 257];
            }
            if (t < 30) {
                const uint32_t f = S.d_freq[t];
                fixed += f * 5u;
                dyn += f * S.d_len[t];
                extra += f * (t < 4 ? 0u : t / 2 - 1);
            }
            if (t < 16) dyn += S.cl_freq[t] * S.cl_len[t];
            atomicAdd(&S.fixed_bits, fixed);
            atomicAdd(&S.dyn_bits, dyn);
            atomicAdd(&S.extra_bits, extra);
        }
        __syncthreads();
        if (t == 0) {
            uint32_t hclen = 19;
            while (hclen > 4 && !S.cl_len[d_cl_order[hclen - 1]]) hclen--;
            S.hclen = hclen;
            const uint32_t size[3] = {5u + n, (3u + S.fixed_bits + S.extra_bits + 7u) / 8u,
                                      (17u + 3u * hclen + S.dyn_bits + S.extra_bits + 7u) / 8u};
            uint32_t f = 0;
            for (uint32_t k = 1; k < 3; k++)
                if (size[k] < size[f]) f = k;
            S.form = f;
            S.payload = size[f];
        }
        __syncthreads();
        const uint32_t form = S.form, payload = S.payload;

        // ---- emit ----
        if (form == 0) {
            if (t == 0) {
                dst[18] = 1;
                dst[19] = (uint8_t)n, dst[20] = (uint8_t)(n >> 8);
                dst[21] = (uint8_t)~n, dst[22] = (uint8_t)(~n >> 8);
            }
            for (uint32_t i = t; i < n; i += kThreads) dst[23 + i] = src[i];
        } else {
            if (form == 1) {
                for (uint32_t s = t; s < 288; s += kThreads) S.ll_len[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
                if (t < 32) S.d_len[t] = 5;
            }
            __syncthreads();
            uint32_t header_bits = 3;
            if (form == 2) header_bits = 17 + 3 * S.hclen;
            if (t == 0) canonical(S.ll_len, 288, S.ll_code);    // 288: the fixed code counts the two symbols deflate never uses
            if (t == 64) canonical(S.d_len, 30, S.d_code);
            if (t == 128 && form == 2) canonical(S.cl_len, 19, S.cl_code);
            if (form == 2)
                for (uint32_t l = 0; l < 16; l++) header_bits += S.cl_freq[l] * S.cl_len[l];
            __syncthreads();
            if (t == 0) {
                BitOut w(payload_words, 0, slot_words);
                w.put(1, 1);
                w.put(form, 2);
                if (form == 2) {
                    w.put(S.hlit - 257, 5);
                    w.put(S.hdist - 1, 5);
                    w.put(S.hclen - 4, 4);
                    for (uint32_t k = 0; k < S.hclen; k++) w.put(S.cl_len[d_cl_order[k]], 3);
                    for (uint32_t s = 0; s < S.hlit; s++) w.put(S.cl_code[S.ll_len[s]], S.cl_len[S.ll_len[s]]);
                    for (uint32_t s = 0; s < S.hdist; s++) w.put(S.cl_code[S.d_len[s]], S.cl_len[S.d_len[s]]);
                }
                w.flush();
            }
            // a contiguous share of the tokens per thread
            const uint32_t share = (n_tok + kThreads - 1) / kThreads;
            const uint32_t t0 = min(n_tok, t * share), t1 = min(n_tok, t0 + share);
            uint32_t bits = 0;
            for (uint32_t k = t0; k < t1; k++) bits += token_bits(S, tok[k]);
            uint32_t total;
            const uint32_t incl = bmscan::block_inclusive<uint32_t>(bits, S.scan_ws, &total);
            BitOut w(payload_words, header_bits + incl - bits, slot_words);
            for (uint32_t k = t0; k < t1; k++) {
                const uint32_t v = tok[k];
                if (v >> 31) {
                    const uint32_t len = (v >> 15) & 0x1FFu, s = S.len_sym[len];
                    w.put(S.ll_code[257 + s], S.ll_len[257 + s]);
                    w.put(len - d_len_base[s], d_len_extra[s]);
                    uint32_t eb, ev;
                    const uint32_t ds = dist_sym((v & 0x7FFFu) + 1, &eb, &ev);
                    w.put(S.d_code[ds], S.d_len[ds]);
                    w.put(ev, eb);
                } else {
                    w.put(S.ll_code[v], S.ll_len[v]);
                }
            }
            if (t == kThreads - 1) w.put(S.ll_code[256], S.ll_len[256]);   // the last share ends where the tokens end
            w.flush();
        }

        // ---- crc ----
        {
            const uint32_t slice = (n + kThreads - 1) / kThreads;
            const uint32_t b0 = min(n, t * slice), b1 = min(n, b0 + slice);
            uint32_t c = 0;
            for (uint32_t i = b0; i < b1; i++) c = S.crc_table[(c ^ src[i]) & 0xFFu] ^ (c >> 8);
            if (c) atomicXor(&S.crc, mul_mod_p(c, x_pow_8(n - b1)));
        }
        __syncthreads();
        if (t == 0) {
            const uint32_t crc = S.crc ^ mul_mod_p(0xFFFFFFFFu, x_pow_8(n)) ^ 0xFFFFFFFFu;
            const uint32_t total = 18 + payload + 8;
            const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
            for (int k = 0; k < 16; k++) dst[k] = head[k];
            dst[16] = (uint8_t)(total - 1), dst[17] = (uint8_t)((total - 1) >> 8);
            uint8_t *tail = dst + 18 + payload;
            for (int k = 0; k < 4; k++) tail[k] = (uint8_t)(crc >> (8 * k)), tail[4 + k] = (uint8_t)(n >> (8 * k));
            sizes[blk] = total;
            forms[blk] = (uint8_t)form;
        }
    }
}

// the slots to their packed places: one workgroup per block
__global__ __launch_bounds__(kThreads) void gather_kernel(const uint8_t *__restrict__ stage, uint32_t stride, const uint32_t *__restrict__ sizes,
                                                         const uint64_t *__restrict__ offsets, uint8_t *__restrict__ out) {
    const uint8_t *src = stage + (size_t)blockIdx.x * stride + kSlotPad;
    uint8_t *dst = out + offsets[blockIdx.x];
    const uint32_t n = sizes[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) dst[i] = src[i];
}

}  // namespace bmz
