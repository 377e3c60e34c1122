// bmd_kernels.hip.h -- duplicate marking of a BAM record stream on gfx950 (include/bmd.h states the rule).
//
//   qual_sum   one workgroup per kChunk = 8 192 bytes of the STREAM, whatever the records are (as bms::gather_kernel): the
//              chunk's first record by bisection over rec_offset, the at most 229 records that touch it into LDS with the
//              extent of their quality bytes; every lane takes aligned 16-byte words, skips those that hold no quality byte,
//              masks the bytes outside a record's quality range and adds what is left to the record's LDS sum (a wave whose
//              lanes all sit in one record reduces first: a long read is one LDS add per wave, not 64).  One u64 global
//              atomic per (record, chunk) into the zeroed score: integer sums, so the order of the adds does not matter.
//   cigar_ends one wave per record: lanes stride over the ops (reflen, the first and the last op that is no clip), a second
//              pass adds the clips before / after them; wave reductions by shuffles.  E(i) or 0, and eligible(i).
//   kinds      one thread per record: the flags of i - 1, i, i + 1; names are compared only where the flags allow a pair.
//   unit_flags / build   the pair units and the fragment units compacted by two scans: per pair unit (min E, max E, ~score),
//              per item of the fragment pass (E, ~score): the 2 P pair ends first with the score key 0, then the fragments.
//   iota / rekey         index = 0, 1, ...; key[j] = word[index[j]]: the next word of a multi-word key, in the order so far.
//   heads      neighbour compare over a sorted order: everything that is not the head of its run of equal keys is marked
//              (pair pass: every unit; fragment pass: fragments only, a pair end heads a run and is never marked).
//   apply      one thread per record: dup[i] from its unit's mark, and in the fused call bit 2 of the record's byte 19.
// The sorts between them are bms::count_kernel / bms::scatter_kernel over (u64 key, u32 index).  Marking uses no atomics and
// no hash tables, and no kernel waits for another workgroup.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmd {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kChunk = 8192, kWord = 16;                     // qual_sum: bytes per workgroup, bytes per access
constexpr uint32_t kMinRecord = 36, kChunkRecords = 256;          // LDS room; kChunk / kMinRecord + 2 = 229 are possible
constexpr uint32_t kQualMin = 15, kQualNone = 0xFF;
static_assert(kChunk / kMinRecord + 2 <= kChunkRecords, "a chunk's records must fit its LDS table");
static_assert(kWord <= kMinRecord && kChunk % (kThreads * kWord) == 0, "every thread makes the same number of trips over a chunk");

__device__ __forceinline__ uint32_t load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__device__ __forceinline__ uint32_t load16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// bytes j in [from, to) of the word x that count towards a score
__device__ __forceinline__ uint32_t masked_sum(const uint32_t (&x)[kWord / 4], uint32_t from, uint32_t to) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWord; j++) {
        const uint32_t q = (x[j >> 2] >> (8 * (j & 3u))) & 255u;
        sum += (j >= from && j < to && q >= kQualMin && q != kQualNone) ? q : 0u;
    }
    return sum;
}

__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int32_t wave_max32(int32_t v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) {
        const int32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// score[i] += the qualifying quality bytes of record i that lie in this workgroup's chunk; score is zero before the launch.
// `in` is 16-aligned; a record's fields fit its extent (checked on the host).
__global__ __launch_bounds__(kThreads) void qual_sum_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                            uint64_t n_bytes, uint64_t *__restrict__ score) {
    __shared__ uint64_t s_at[kChunkRecords + 1], s_qlo[kChunkRecords], s_qhi[kChunkRecords];
    __shared__ uint32_t s_sum[kChunkRecords];
    __shared__ uint32_t s_first, s_count;
    const uint64_t lo = (uint64_t)blockIdx.x * kChunk, hi = lo + kChunk < n_bytes ? lo + kChunk : n_bytes;
    if (threadIdx.x == 0) {
        // the last record that starts at or before lo (rec_offset[0] = 0 <= lo), the first that starts at or after hi
        uint32_t a = 0, b = n;
        while (b - a > 1) {
            const uint32_t m = a + (b - a) / 2;
            if (rec_offset[m] <= lo) a = m; else b = m;
        }
        uint32_t e = a + 1, f = n;
        while (e < f) {
            const uint32_t m = e + (f - e) / 2;
            if (rec_offset[m] < hi) e = m + 1; else f = m;
        }
        s_first = a;
        s_count = e - a < kChunkRecords ? e - a : kChunkRecords;
    }
    __syncthreads();
    const uint32_t first = s_first, count = s_count;
    for (uint32_t k = threadIdx.x; k <= count; k += kThreads) {
        const uint64_t at = rec_offset[first + k];
        s_at[k] = at;
        if (k < count) {
            const uint8_t *r = in + at;
            const uint64_t l_seq = load32(r + 20);
            const uint64_t qlo = at + 36 + r[12] + 4ull * load16(r + 16) + (l_seq + 1) / 2;
            s_qlo[k] = qlo;
            s_qhi[k] = qlo + l_seq;
            s_sum[k] = 0;
        }
    }
    __syncthreads();
    for (uint64_t w0 = lo; w0 < hi; w0 += (uint64_t)kThreads * kWord) {   // the same trip count in every lane: shuffles below
        const uint64_t w = w0 + (uint64_t)threadIdx.x * kWord;
        uint32_t a = 0, sum = 0;
        if (w < hi) {
            uint32_t b = count;                          // the record that holds byte w
            while (b - a > 1) {
                const uint32_t m = a + (b - a) / 2;
                if (s_at[m] <= w) a = m; else b = m;
            }
            // Where the word reaches into record a + 1 it holds none of that record's quality bytes: they begin 36 bytes or
            // more behind its start.  So the word's quality bytes are record a's, and those end with the record.
            const uint64_t end = w + kWord < hi ? w + kWord : hi;
            const uint64_t q_lo = s_qlo[a] > w ? s_qlo[a] : w, q_hi = s_qhi[a] < end ? s_qhi[a] : end;
            if (q_lo < q_hi) {                           // the word holds a quality byte: only then is it read
                uint32_t x[kWord / 4] = {0, 0, 0, 0};
                if (w + kWord <= n_bytes) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(in + w);
                    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
                } else {                                 // the stream's last word: no byte beyond its end is read
#pragma unroll
                    for (uint32_t j = 0; j < kWord; j++)
                        if (w + j < n_bytes) x[j >> 2] |= (uint32_t)in[w + j] << (8 * (j & 3u));
                }
                sum = masked_sum(x, (uint32_t)(q_lo - w), (uint32_t)(q_hi - w));
            }
        }
        const uint32_t a0 = __builtin_amdgcn_readfirstlane(a);
        if (__all(a == a0)) {                            // one record under the whole wave (idle lanes have a = 0 and add 0)
            const uint32_t total = wave_sum32(sum);
            if ((threadIdx.x & 63u) == 0 && total) atomicAdd(&s_sum[a0], total);
        } else if (sum) {
            atomicAdd(&s_sum[a], sum);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < count; k += kThreads)
        if (s_sum[k]) atomicAdd(reinterpret_cast<unsigned long long *>(&score[first + k]), (unsigned long long)s_sum[k]);
}

// end[i] = E(i) or 0, eligible[i]; one wave per record, kWaves records per workgroup
__global__ __launch_bounds__(kThreads) void cigar_ends_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                              uint64_t *__restrict__ end, uint8_t *__restrict__ eligible) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i64 = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i64 >= n) return;                                // the whole wave
    const uint32_t i = (uint32_t)i64;
    const uint8_t *r = in + rec_offset[i];
    const int32_t ref = (int32_t)load32(r + 4), pos = (int32_t)load32(r + 8);
    const uint32_t n_cigar = load16(r + 16), flag = load16(r + 18), l_seq = load32(r + 20);
    const uint8_t *cigar = r + 36 + r[12];
    uint64_t reflen = 0;
    uint32_t first_nc = n_cigar;                         // the first op that is no clip, the last one (-1: none)
    int32_t last_nc = -1;
    for (uint32_t k = lane; k < n_cigar; k += 64) {
        const uint32_t c = load32(cigar + 4ull * k), op = c & 15u;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += c >> 4;
        if (op != 4 && op != 5) {
            first_nc = k < first_nc ? k : first_nc;
            last_nc = (int32_t)k;
        }
    }
    reflen = wave_sum64(reflen);
    first_nc = wave_min32(first_nc);
    last_nc = wave_max32(last_nc);
    uint64_t lead = 0, trail = 0;
    for (uint32_t k = lane; k < n_cigar; k += 64) {      // every op outside [first_nc, last_nc] is a clip
        if (k >= first_nc && (int32_t)k <= last_nc) continue;
        const uint32_t len = load32(cigar + 4ull * k) >> 4;
        if (k < first_nc) lead += len;
        if ((int32_t)k > last_nc) trail += len;
    }
    lead = wave_sum64(lead);
    trail = wave_sum64(trail);
    if (lane != 0) return;
    const bool reverse = flag & 0x10u;
    const int64_t end5 = reverse ? (int64_t)pos + (int64_t)reflen + (int64_t)trail - 1 : (int64_t)pos - (int64_t)lead;
    bool ok = !(flag & (0x4u | 0x100u | 0x800u)) && ref >= 0 && end5 >= -(int64_t{1} << 31) && end5 < (int64_t{1} << 31);
    if (ok && n_cigar == 2) {
        const uint32_t c0 = load32(cigar), c1 = load32(cigar + 4);
        if (c0 == (l_seq << 4 | 4u) && (c1 & 15u) == 3u) ok = false;   // the long-CIGAR placeholder
    }
    end[i] = ok ? (uint64_t)(uint32_t)ref << 33 | (uint64_t)(end5 + (int64_t{1} << 31)) << 1 | (reverse ? 1u : 0u) : 0;
    eligible[i] = ok ? 1 : 0;
}

// records a (0x40) and a + 1 (0x80) are mates
__device__ __forceinline__ bool mates(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t a) {
    const uint8_t *x = in + rec_offset[a], *y = in + rec_offset[a + 1];
    const uint32_t fx = load16(x + 18), fy = load16(y + 18);
    if ((fx & (0x1u | 0x40u | 0x80u | 0x100u | 0x800u)) != (0x1u | 0x40u)) return false;
    if ((fy & (0x1u | 0x40u | 0x80u | 0x100u | 0x800u)) != (0x1u | 0x80u)) return false;
    const uint32_t len = x[12];
    if (len != y[12]) return false;
    for (uint32_t k = 0; k < len; k++)
        if (x[36 + k] != y[36 + k]) return false;
    return true;
}

__global__ __launch_bounds__(kThreads) void kinds_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                         const uint8_t *__restrict__ eligible, uint8_t *__restrict__ kind) {
    const uint64_t i64 = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    uint8_t k = 0;
    if (eligible[i]) {
        k = 1;
        if (i + 1 < n && eligible[i + 1] && mates(in, rec_offset, i)) k = 2;
        else if (i > 0 && eligible[i - 1] && mates(in, rec_offset, i - 1)) k = 3;
    }
    kind[i] = k;
}

__global__ __launch_bounds__(kThreads) void unit_flags_kernel(const uint8_t *__restrict__ kind, uint32_t n, uint32_t *__restrict__ is_pair,
                                                              uint32_t *__restrict__ is_frag) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    is_pair[i] = kind[i] == 2;
    is_frag[i] = kind[i] == 1;
}

// pair unit u = pair_slot[i] of a kind-2 record i: (lo, hi, ~score); items 2u, 2u + 1 of the fragment pass: its ends, key 0;
// fragment f = frag_slot[i] of a kind-1 record: item 2 P + f
__global__ __launch_bounds__(kThreads) void build_kernel(const uint64_t *__restrict__ end, const uint64_t *__restrict__ score,
                                                         const uint8_t *__restrict__ kind, uint32_t n, const uint32_t *__restrict__ pair_slot,
                                                         const uint32_t *__restrict__ frag_slot, uint32_t n_pairs, uint32_t n_frags,
                                                         uint64_t *__restrict__ p_lo, uint64_t *__restrict__ p_hi, uint64_t *__restrict__ p_key,
                                                         uint64_t *__restrict__ a_end, uint64_t *__restrict__ a_key) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (kind[i] == 2 && i + 1 < n) {
        const uint32_t u = pair_slot[i];
        if (u >= n_pairs) return;                        // never; keeps a wrong scan from becoming a wild store
        const uint64_t x = end[i], y = end[i + 1];
        p_lo[u] = x < y ? x : y;
        p_hi[u] = x < y ? y : x;
        p_key[u] = ~(score[i] + score[i + 1]);
        a_end[2ull * u] = x, a_end[2ull * u + 1] = y;
        a_key[2ull * u] = 0, a_key[2ull * u + 1] = 0;
    } else if (kind[i] == 1) {
        const uint32_t f = frag_slot[i];
        if (f >= n_frags) return;
        a_end[2ull * n_pairs + f] = end[i];
        a_key[2ull * n_pairs + f] = ~score[i];
    }
}

__global__ __launch_bounds__(kThreads) void iota_kernel(const uint64_t *__restrict__ word, uint32_t n, uint64_t *__restrict__ key,
                                                        uint32_t *__restrict__ index) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    key[j] = word[j];
    index[j] = (uint32_t)j;
}

__global__ __launch_bounds__(kThreads) void rekey_kernel(const uint64_t *__restrict__ word, const uint32_t *__restrict__ index, uint32_t n,
                                                         uint64_t *__restrict__ key) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j < n) key[j] = word[index[j]];
}

// mark[index[j]] = the item at place j is not the head of its run of equal (lo, hi)
__global__ __launch_bounds__(kThreads) void pair_heads_kernel(const uint32_t *__restrict__ index, uint32_t n, const uint64_t *__restrict__ p_lo,
                                                              const uint64_t *__restrict__ p_hi, uint32_t *__restrict__ mark) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const uint32_t u = index[j];
    uint32_t m = 0;
    if (j > 0) {
        const uint32_t v = index[j - 1];
        m = p_lo[u] == p_lo[v] && p_hi[u] == p_hi[v];
    }
    if (u < n) mark[u] = m;
}

// the same over the items of the fragment pass; items below first_frag are pair ends and are never marked
__global__ __launch_bounds__(kThreads) void frag_heads_kernel(const uint32_t *__restrict__ index, uint32_t n, const uint64_t *__restrict__ a_end,
                                                              uint32_t first_frag, uint32_t *__restrict__ mark) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const uint32_t a = index[j];
    if (a < first_frag || a >= n) return;
    mark[a - first_frag] = j > 0 && a_end[a] == a_end[index[j - 1]];
}

// dup[i] from the unit's mark; stream != nullptr: bit 2 of byte 19 of a duplicate's record (its own byte, one writer)
__global__ __launch_bounds__(kThreads) void apply_kernel(const uint8_t *__restrict__ kind, uint32_t n, const uint32_t *__restrict__ pair_slot,
                                                         const uint32_t *__restrict__ frag_slot, const uint32_t *__restrict__ pair_mark,
                                                         const uint32_t *__restrict__ frag_mark, uint8_t *__restrict__ dup,
                                                         uint8_t *__restrict__ stream, const uint64_t *__restrict__ rec_offset) {
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = kind[i];
    uint32_t m = 0;
    if (k == 2) m = pair_mark[pair_slot[i]];
    else if (k == 3 && i > 0) m = pair_mark[pair_slot[i - 1]];
    else if (k == 1) m = frag_mark[frag_slot[i]];
    dup[i] = m ? 1 : 0;
    if (m && stream) stream[rec_offset[i] + 19] |= 4;
}

}  // namespace bmd
