// bms_kernels.hip.h -- BAM records put in coordinate order on gfx950 (include/bms.h): keys, a stable LSD radix sort of
// (key, index) pairs, and a gather of the records that is balanced by bytes.
//
//   keys     one thread per record: the eight key bytes (records are not 4-aligned), the 64-bit key, the length, index i.
//   hist     the counts of all eight 8-bit digits in one pass over the keys (LDS counts, then one add per bucket and
//            workgroup; sums do not depend on the order of the adds).  The host reads the 2 048 counts: a digit on which
//            all keys agree has one bucket holding n and costs no pass.
//   per remaining digit, over tiles of kTile = 1 024 consecutive items:
//     count    a tile's 256 bucket counts, written digit-major: counts[digit * n_tiles + tile]
//     scan     bmscan::exclusive_sum over them: the place of the first item of (digit, tile)
//     scatter  the tile again, 256 items a round.  An item's rank among the equal digits of its wave comes from eight ballots
//              (the lanes below it that match in every bit); each wave leaves the size of every group in an LDS slot of its
//              own, slot[round * 4 + wave][digit]; thread d turns the 16 slots of digit d into running places, starting at
//              the scanned place of (d, tile).  No atomics: the order is that of the items.
//   perm_len the sorted records' lengths, scanned (64-bit) into sorted_offset
//   gather   one workgroup per kChunk = 8 192 bytes of the SORTED stream, whatever the records are: the chunk's first
//            record by bisection over sorted_offset, the at most 229 records that touch it (a record has 36 bytes or more)
//            into LDS, then every thread takes aligned 16-byte words of the destination: a word inside one record is a
//            16-byte load from the (unaligned) source and an aligned 16-byte store, a word that holds a record border or the
//            stream's end goes byte by byte.
// No kernel waits for another workgroup; every ordering comes from the scans.
#pragma once

#include "bm_scan.hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bms {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kRounds = 4, kTile = kThreads * kRounds;      // items of one sort tile
constexpr uint32_t kChunk = 8192, kWord = 16;                     // gather: bytes per workgroup, bytes per access
constexpr uint32_t kMinRecord = 36;                               // block_size + the 32 fixed bytes
constexpr uint32_t kChunkRecords = 256;                           // LDS room; kChunk / kMinRecord + 2 = 229 are possible

__device__ __forceinline__ uint32_t load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// key = (uint64)(uint32)refID << 32 | (uint32)(pos + 1), from bytes 4..12 of the record
__global__ __launch_bounds__(kThreads) void keys_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset,
                                                        uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ index,
                                                        uint32_t *__restrict__ length) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t at = rec_offset[i];
    const uint32_t ref = load32(in + at + 4), pos = load32(in + at + 8);
    key[i] = (uint64_t)ref << 32 | (uint32_t)(pos + 1u);
    index[i] = i;
    length[i] = (uint32_t)(rec_offset[i + 1] - at);
}

// hist[d * 256 + b] += the keys whose digit d is b; hist is zero before the launch
__global__ __launch_bounds__(kThreads) void hist_kernel(const uint64_t *__restrict__ key, uint32_t n, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[8 * 256];
    for (uint32_t k = threadIdx.x; k < 8 * 256; k += kThreads) h[k] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kThreads) {
        const uint64_t v = key[i];
#pragma unroll
        for (uint32_t d = 0; d < 8; d++) atomicAdd(&h[d * 256 + (uint32_t)((v >> (8 * d)) & 255u)], 1u);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 8 * 256; k += kThreads)
        if (h[k]) atomicAdd(&hist[k], h[k]);
}

__global__ __launch_bounds__(kThreads) void count_kernel(const uint64_t *__restrict__ key, uint32_t n, uint32_t shift, uint32_t n_tiles,
                                                         uint32_t *__restrict__ counts) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint64_t i = base + r * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)((key[i] >> shift) & 255u)], 1u);
    }
    __syncthreads();
    counts[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kThreads) void scatter_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ index, uint32_t n,
                                                           uint32_t shift, uint32_t n_tiles, const uint32_t *__restrict__ place,
                                                           uint64_t *__restrict__ key_out, uint32_t *__restrict__ index_out) {
    __shared__ uint32_t slot[kRounds * kWaves][256];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t k = threadIdx.x; k < kRounds * kWaves * 256; k += kThreads) (&slot[0][0])[k] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    uint64_t v[kRounds];
    uint32_t idx[kRounds], rank[kRounds];
    bool live[kRounds];
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        const uint64_t i = base + r * kThreads + threadIdx.x;
        live[r] = i < n;
        v[r] = live[r] ? key[i] : 0;
        idx[r] = live[r] ? index[i] : 0;
        const uint32_t digit = (uint32_t)((v[r] >> shift) & 255u);
        uint64_t same = __ballot(live[r]);              // the live lanes of the wave whose digit equals this lane's
#pragma unroll
        for (uint32_t b = 0; b < 8; b++) {
            const uint64_t set = __ballot(live[r] && ((digit >> b) & 1u));
            same &= ((digit >> b) & 1u) ? set : ~set;
        }
        rank[r] = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (live[r] && rank[r] == 0) slot[r * kWaves + wave][digit] = (uint32_t)__popcll(same);   // one lane per group
    }
    __syncthreads();
    {
        uint32_t run = place[(uint64_t)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
        for (uint32_t s = 0; s < kRounds * kWaves; s++) {
            const uint32_t c = slot[s][threadIdx.x];
            slot[s][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRounds; r++) {
        if (!live[r]) continue;
        const uint32_t digit = (uint32_t)((v[r] >> shift) & 255u);
        const uint32_t to = slot[r * kWaves + wave][digit] + rank[r];
        if (to < n) {                                    // always; keeps a wrong count from becoming a wild store
            key_out[to] = v[r];
            index_out[to] = idx[r];
        }
    }
}

__global__ __launch_bounds__(kThreads) void perm_len_kernel(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ length, uint32_t n,
                                                            uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = length[perm[i]];
}

// out[sorted_offset[i] ..) = in[rec_offset[perm[i]] ..), one workgroup per kChunk bytes of out; out is 16-aligned
__global__ __launch_bounds__(kThreads) void gather_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset,
                                                          const uint32_t *__restrict__ perm, const uint64_t *__restrict__ sorted_offset,
                                                          uint32_t n, uint64_t n_bytes, uint8_t *__restrict__ out) {
    __shared__ uint64_t s_to[kChunkRecords + 1], s_from[kChunkRecords];
    __shared__ uint32_t s_first, s_count;
    const uint64_t lo = (uint64_t)blockIdx.x * kChunk, hi = lo + kChunk < n_bytes ? lo + kChunk : n_bytes;
    if (threadIdx.x == 0) {
        // the last record that starts at or before lo (sorted_offset[0] = 0 <= lo), the first that starts at or after hi
        uint32_t a = 0, b = n;
        while (b - a > 1) {
            const uint32_t m = a + (b - a) / 2;
            if (sorted_offset[m] <= lo) a = m; else b = m;
        }
        uint32_t e = a + 1, f = n;
        while (e < f) {
            const uint32_t m = e + (f - e) / 2;
            if (sorted_offset[m] < hi) e = m + 1; else f = m;
        }
        s_first = a;
        s_count = e - a < kChunkRecords ? e - a : kChunkRecords;
    }
    __syncthreads();
    const uint32_t first = s_first, count = s_count;
    for (uint32_t k = threadIdx.x; k <= count; k += kThreads) {
        s_to[k] = sorted_offset[first + k];
        if (k < count) s_from[k] = rec_offset[perm[first + k]];
    }
    __syncthreads();
    for (uint64_t w = lo + (uint64_t)threadIdx.x * kWord; w < hi; w += (uint64_t)kThreads * kWord) {
        uint32_t a = 0, b = count;                       // the record that holds byte w
        while (b - a > 1) {
            const uint32_t m = a + (b - a) / 2;
            if (s_to[m] <= w) a = m; else b = m;
        }
        if (w + kWord <= s_to[a + 1]) {
            uint4 x;
            __builtin_memcpy(&x, in + s_from[a] + (w - s_to[a]), kWord);
            *reinterpret_cast<uint4 *>(out + w) = x;
        } else {
            const uint64_t end = w + kWord < hi ? w + kWord : hi;
            for (uint64_t p = w; p < end; p++) {
                while (a + 1 < count && p >= s_to[a + 1]) a++;
                out[p] = in[s_from[a] + (p - s_to[a])];
            }
        }
    }
}

}  // namespace bms
