// bmf_kmer_lists.hip.h -- the default vote on per-k-mer bucket-id lists.
//
// A sample contributes the AND of the rows of its G q-grams, and that AND is a function of the k-mer and the index
// alone.  Where the index is sparse enough (build_kmer_lists in bmf_api.hip decides, once per load) it is stored for
// every k-mer x < 4^k as the ascending 16-bit ids of its set bits:
//
//   offsets[x] .. offsets[x + 1]   64-bit, in 16-byte units (8 ids): every list starts on a 16-byte boundary, a lane
//                                  loads 8 ids with one 16-byte load and a wave reads 1 KiB contiguous
//   ids                            the last unit of a list is filled up with kPadId, which is no bucket (NB <= 65 535)
//
// A k-mer none of whose q-grams is indexed ANDs nothing but all-ones rows: its list holds all NB ids, in the same form.
//
//   bmf_kmer_count_kernel  AND + popcount: units per k-mer.  One wave per (k-1)-prefix p: the k-mers 4p .. 4p + 3 share
//                          the rows of their q-grams 1 .. G-1, and their q-grams 0 are neighbours in kmer_to_index
//                          (as in bmf_pair_rows_kernel): G + 3 row reads for four k-mers.
//   (bm_scan.hip.h)        units -> offsets
//   bmf_kmer_fill_kernel   the same ANDs again, the ids written in order (ballot-free: a wave prefix sum of the lanes'
//                          popcounts per round of 64 chunks)
//   bmf_vote_kernel_lists  one wave per (window, orientation); the list entries of the sample kernel are the k-mer
//                          hashes themselves (DevParams::pair == 2).  Per-wave hit counters in LDS, BITS = 4 (S <= 15)
//                          or 8 bits per bucket packed in dwords, incremented with returning LDS atomic adds: the
//                          value that comes back is the count before, so the wave knows its highest hit count without
//                          looking at the counters.  misses = S - hits: an item whose highest count is at most S - F
//                          is empty and is done; the others scan the counters once, in bucket order, for the buckets
//                          at the maximum (ids staged in LDS: more than max_candidates of them is "cleared").
//                          The adds are not waited for one by one: the eight of a unit are issued back to back, with no
//                          branch per id (a padding id adds 0 where it harms nothing), and folded into the maximum after
//                          the next unit's are issued (kmer_count_units).
//                          A workgroup is one wave and one item, and starts by zeroing its counters: ceil(NB / 128 or
//                          64) 16-byte LDS stores per lane round, far fewer instructions than a second walk over the
//                          lists would be.  (One resident round of waves, each walking its items with the next items'
//                          loads issued ahead, was built and measured slower than this: profiles/r07/README.md.)
//                          Nothing depends on lists being short: the first 64 units of up to 16 lists are in flight
//                          at once, what lies beyond them is walked four wave loads at a time.
#pragma once

#include "bmf_kernels.hip.h"

namespace bmf {

constexpr uint32_t kPadId = 0xFFFFu;

// the AND of the G - 1 rows the four k-mers of prefix p share, and the rows of their four q-grams 0: chunk c
struct KmerPrefixRows {
    int32_t shared[7];
    int4 low;
};

__device__ __forceinline__ KmerPrefixRows kmer_prefix_rows(const int32_t *__restrict__ k2i, uint32_t n_kmers, uint32_t qbits,
                                                           uint32_t G, uint32_t p) {
    KmerPrefixRows r;
#pragma unroll
    for (uint32_t g = 1; g < 8; g++) {
        const uint32_t gram = (p >> (2u * (g - 1u))) & qbits;
        r.shared[g - 1] = g < G && gram < n_kmers ? k2i[gram] : -1;
    }
    const uint32_t lo0 = (p * 4u) & qbits;
    r.low = lo0 + 3u < n_kmers ? *reinterpret_cast<const int4 *>(k2i + lo0) : make_int4(-1, -1, -1, -1);
    return r;
}

// out[d] = chunk c of the AND of k-mer 4p + d (all ones, cut at NB, for a q-gram that is not indexed)
__device__ __forceinline__ void kmer_and_chunk(const uint8_t *__restrict__ rows, uint32_t pitch, uint32_t nb,
                                               const KmerPrefixRows &r, uint32_t c, uint4 (&out)[4]) {
    const uint32_t b0 = c * 128u;
    auto word = [&](uint32_t b) { return b >= nb ? 0u : (nb - b >= 32u ? 0xFFFFFFFFu : (1u << (nb - b)) - 1u); };
    uint4 a = make_uint4(word(b0), word(b0 + 32u), word(b0 + 64u), word(b0 + 96u));
#pragma unroll
    for (int g = 0; g < 7; g++) {
        if (r.shared[g] >= 0) {                       // wave-uniform
            const uint4 t = *reinterpret_cast<const uint4 *>(rows + (size_t)r.shared[g] * pitch + 16u * c);
            a = make_uint4(a.x & t.x, a.y & t.y, a.z & t.z, a.w & t.w);
        }
    }
    const int32_t low[4] = {r.low.x, r.low.y, r.low.z, r.low.w};
#pragma unroll
    for (int d = 0; d < 4; d++) {
        out[d] = a;
        if (low[d] >= 0) {
            const uint4 t = *reinterpret_cast<const uint4 *>(rows + (size_t)low[d] * pitch + 16u * c);
            out[d] = make_uint4(a.x & t.x, a.y & t.y, a.z & t.z, a.w & t.w);
        }
    }
}

// units[4 i + d] = 16-byte units of the list of k-mer 4 p + d, p = (p_first + i * p_stride) & p_mask, i < n_p.  The full
// pass has p_first 0 and p_stride 1; the estimate before it looks at a strided sample (p_mask = 4^(k-1) - 1).
__global__ __launch_bounds__(kWave) void bmf_kmer_count_kernel(const uint8_t *__restrict__ rows, const int32_t *__restrict__ k2i,
                                                              uint32_t n_kmers, uint32_t qbits, uint32_t G, uint32_t pitch, uint32_t nb,
                                                              uint32_t n_chunks, uint32_t p_first, uint32_t p_stride, uint32_t p_mask,
                                                              uint32_t n_p, uint32_t *__restrict__ units) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = blockIdx.x; i < n_p; i += gridDim.x) {
        const KmerPrefixRows r = kmer_prefix_rows(k2i, n_kmers, qbits, G, (p_first + i * p_stride) & p_mask);
        uint32_t n[4] = {0, 0, 0, 0};
        for (uint32_t c = lane; c < n_chunks; c += kWave) {
            uint4 a[4];
            kmer_and_chunk(rows, pitch, nb, r, c, a);
#pragma unroll
            for (int d = 0; d < 4; d++) n[d] += __popc(a[d].x) + __popc(a[d].y) + __popc(a[d].z) + __popc(a[d].w);
        }
#pragma unroll
        for (int d = 0; d < 4; d++) n[d] = wave_sum(n[d]);
        if (lane < 4u) units[(size_t)i * 4u + lane] = ((lane == 0 ? n[0] : lane == 1 ? n[1] : lane == 2 ? n[2] : n[3]) + 7u) >> 3;
    }
}

__global__ __launch_bounds__(kWave) void bmf_kmer_fill_kernel(const uint8_t *__restrict__ rows, const int32_t *__restrict__ k2i,
                                                             uint32_t n_kmers, uint32_t qbits, uint32_t G, uint32_t pitch, uint32_t nb,
                                                             uint32_t n_chunks, uint32_t n_p, const uint64_t *__restrict__ offsets,
                                                             uint16_t *__restrict__ ids) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t p = blockIdx.x; p < n_p; p += gridDim.x) {
        const KmerPrefixRows r = kmer_prefix_rows(k2i, n_kmers, qbits, G, p);
        uint32_t done[4] = {0, 0, 0, 0};              // ids of each list written by the rounds before (wave-uniform)
        for (uint32_t c0 = 0; c0 < n_chunks; c0 += kWave) {
            const uint32_t c = c0 + lane;
            uint4 a[4];
            if (c < n_chunks) {
                kmer_and_chunk(rows, pitch, nb, r, c, a);
            } else {
#pragma unroll
                for (int d = 0; d < 4; d++) a[d] = make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int d = 0; d < 4; d++) {
                const uint32_t w[4] = {a[d].x, a[d].y, a[d].z, a[d].w};
                const uint32_t pc = __popc(w[0]) + __popc(w[1]) + __popc(w[2]) + __popc(w[3]);
                uint32_t incl = pc;
#pragma unroll
                for (int o = 1; o < kWave; o <<= 1) {
                    const uint32_t t = __shfl_up(incl, o, kWave);
                    if (lane >= (uint32_t)o) incl += t;
                }
                uint16_t *out = ids + offsets[(size_t)p * 4u + d] * 8u + done[d] + (incl - pc);
                done[d] += __shfl(incl, kWave - 1, kWave);
#pragma unroll
                for (int x = 0; x < 4; x++) {
                    uint32_t bits = w[x];
                    while (bits) {
                        *out++ = (uint16_t)(c * 128u + x * 32u + (uint32_t)__builtin_ctz(bits));
                        bits &= bits - 1u;
                    }
                }
            }
        }
#pragma unroll
        for (int d = 0; d < 4; d++) {                 // fill the last unit
            const uint32_t pad = (8u - (done[d] & 7u)) & 7u;
            if (lane < pad) ids[offsets[(size_t)p * 4u + d] * 8u + done[d] + lane] = (uint16_t)kPadId;
        }
    }
}

// LDS bytes per wave of bmf_vote_kernel_lists: the counters, rounded up to whole 16-byte stores, then the staged ids
inline uint32_t kmer_vote_counter_bytes(uint32_t nb, uint32_t bits) { return ((nb * bits + 127u) / 128u) * 16u; }
inline uint32_t kmer_vote_lds_bytes(uint32_t nb, uint32_t bits) { return kmer_vote_counter_bytes(nb, bits) + 64u * 4u + 16u; }

// The eight ids of one unit, their adds issued back to back: old[j] is what the dword of id j held before.  An id that
// is no bucket (kPadId, anything >= NB) adds 0, at its own dword where that lies inside the counters and else at the
// lane's dword of the staging area (dword `spare`): it counts nowhere and no two lanes pile onto one address.  A lane
// whose first id is no bucket holds no unit and takes no part.
template <int BITS>
__device__ __forceinline__ void kmer_unit_issue(uint32_t *cnt, uint32_t spare, const uint4 &u, uint32_t nb, uint32_t (&old)[8]) {
    constexpr uint32_t kPer = 32u / BITS;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 8; j++) old[j] = 0;
    if ((w[0] & 0xFFFFu) < nb) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t id = j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xFFFFu;
            old[j] = atomicAdd(&cnt[min(id / kPer, spare)], id < nb ? 1u << ((id % kPer) * BITS) : 0u);
        }
    }
}

// ... and the highest count any of them reached, once the adds have returned
template <int BITS>
__device__ __forceinline__ uint32_t kmer_unit_fold(const uint4 &u, uint32_t nb, const uint32_t (&old)[8], uint32_t mx) {
    constexpr uint32_t kPer = 32u / BITS, kMask = (1u << BITS) - 1u;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t id = j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xFFFFu;
        mx = max(mx, id < nb ? ((old[j] >> ((id % kPer) * BITS)) & kMask) + 1u : 0u);
    }
    return mx;
}

// N units counted with no wait per add: the adds of unit i are issued before the returns of unit i - 1 are folded into mx
// (LDS returns come back in order, so up to 16 are in flight; a lane without a unit skips its adds, which is why the
// compiler's counted waits let a fold wait for at most the first add of the unit after its own).  after(i) runs when u[i]
// has been folded.
template <int BITS, int N, class After>
__device__ __forceinline__ uint32_t kmer_count_units(uint32_t *cnt, uint32_t spare, const uint4 (&u)[N], uint32_t nb, uint32_t mx,
                                                     After after) {
    uint32_t old[2][8];
#pragma unroll
    for (int i = 0; i < N; i++) {
        kmer_unit_issue<BITS>(cnt, spare, u[i], nb, old[i & 1]);
        if (i > 0) {
            mx = kmer_unit_fold<BITS>(u[i - 1], nb, old[(i - 1) & 1], mx);
            asm volatile("" : "+v"(mx) : : "memory");      // folded here, not after the last unit (the compiler sinks the
                                                           // folds there, 128 returns live): the returns die now
            after(i - 1);
        }

    }
    mx = kmer_unit_fold<BITS>(u[N - 1], nb, old[(N - 1) & 1], mx);
    after(N - 1);
    return mx;
}

template <int BITS>
__global__ __launch_bounds__(kWave) void bmf_vote_kernel_lists(DevParams P, const uint64_t *__restrict__ offsets,
                                                              const uint4 *__restrict__ units,
                                                              const uint32_t *__restrict__ kmer_lists,
                                                              const uint32_t *__restrict__ list_n,
                                                              uint32_t *__restrict__ out_counts,
                                                              uint32_t *__restrict__ out_buckets) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cnt[];
    constexpr uint32_t kPer = 32u / BITS, kField = (1u << BITS) - 1u;
    constexpr uint32_t kTop = BITS == 4 ? 0x88888888u : 0x80808080u, kLow = ~kTop;
    const uint32_t lane = threadIdx.x, item = blockIdx.x;
    if (list_n[item >> 1] == 0) {              // window rejected by the sample kernel
        if (lane == 0) out_counts[item] = 0;
        return;
    }
    const uint32_t n_dw = (P.nb + kPer - 1u) / kPer, n_q = (n_dw + 3u) >> 2;   // counter dwords, 16-byte groups of them
    uint32_t *stage = lds_cnt + n_q * 4u;      // [0..63] ids at the maximum, [64] how many
    const uint32_t spare = n_q * 4u + lane;    // (adding 0 to a staged id changes nothing)
    for (uint32_t i = lane; i < n_q; i += kWave) reinterpret_cast<uint4 *>(lds_cnt)[i] = make_uint4(0, 0, 0, 0);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // lane s holds the extent of sample s's list
    uint64_t first = 0;
    uint32_t n_units = 0;
    if (lane < P.S) {
        const uint32_t h = kmer_lists[(size_t)item * P.list_len + lane];
        first = offsets[h];
        n_units = (uint32_t)(offsets[(size_t)h + 1u] - first);
    }
    uint32_t mx = 0;
    for (uint32_t s0 = 0; s0 < P.S; s0 += 16u) {
        // the first 64 units of up to 16 lists, all issued before the first is counted
        uint4 u[16];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint64_t f = __shfl(first, (int)(s0 + i) & 63, kWave);
            const uint32_t n = s0 + i < P.S ? __shfl(n_units, (int)(s0 + i) & 63, kWave) : 0u;
            u[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            if (lane < n) u[i] = units[f + lane];
        }
        mx = kmer_count_units<BITS>(lds_cnt, spare, u, P.nb, mx, [](int) {});
    }
    // what lies beyond 64 units (heavy k-mers; a k-mer with no indexed q-gram holds all NB ids): four wave loads at a time
    if (__ballot(n_units > (uint32_t)kWave) != 0) {
        for (uint32_t s = 0; s < P.S; s++) {
            const uint64_t f = __shfl(first, (int)s, kWave);
            const uint32_t n = __shfl(n_units, (int)s, kWave);
            for (uint32_t at = kWave; at < n; at += 4u * kWave) {
                uint4 u[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t t = at + (uint32_t)i * kWave + lane;
                    u[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
                    if (t < n) u[i] = units[f + t];
                }
                mx = kmer_count_units<BITS>(lds_cnt, spare, u, P.nb, mx, [](int) {});
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, kWave));
    // fewest misses = S - mx; nothing below F misses: every level of the reference's filter is empty
    if (mx + P.F <= P.S) {
        if (lane == 0) out_counts[item] = 0;
        return;                                 // (the counters die with the workgroup)
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the buckets whose counter is mx, in ascending order: lane l of round r holds counter dwords 4 (64 r + l) .. + 3
    const uint32_t want = mx * (0xFFFFFFFFu / kField);        // mx in every field
    uint32_t total = 0;
    for (uint32_t q0 = 0; q0 < n_q; q0 += kWave) {
        const uint32_t qi = q0 + lane;
        uint4 v = make_uint4(~want, ~want, ~want, ~want);
        if (qi < n_q) v = reinterpret_cast<const uint4 *>(lds_cnt)[qi];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t eq[4], pc = 0;
#pragma unroll
        for (int x = 0; x < 4; x++) {
            const uint32_t d = w[x] ^ want;                     // a field is zero where the counter is mx
            eq[x] = ~(((d & kLow) + kLow) | d | kLow);          // its top bit, exactly (no carry leaves a field)
            const uint32_t b0 = (qi * 4u + (uint32_t)x) * kPer; // fields past NB are no buckets (they matter when mx is 0)
            const uint32_t left = b0 < P.nb ? P.nb - b0 : 0u;
            if (left < kPer) eq[x] &= (1u << (left * BITS)) - 1u;
            pc += __popc(eq[x]);
        }
        if (__ballot(pc != 0) == 0) continue;
        uint32_t incl = pc;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, kWave);
            if (lane >= (uint32_t)o) incl += t;
        }
        uint32_t pos = total + incl - pc;
        total += __shfl(incl, kWave - 1, kWave);
#pragma unroll
        for (int x = 0; x < 4; x++) {
            uint32_t bits = eq[x];
            while (bits) {
                if (pos < (uint32_t)kWave) stage[pos] = (qi * 4u + (uint32_t)x) * kPer + (uint32_t)__builtin_ctz(bits) / BITS;
                pos++;
                bits &= bits - 1u;
            }
        }
        if (total > P.max_cand) break;          // cleared whatever follows (wave-uniform)
    }
    if (total > P.max_cand) {                   // q_gram_mapper.h:471-476
        if (lane == 0) out_counts[item] = 0;
        return;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < total) out_buckets[(size_t)item * P.max_cand + lane] = stage[lane];
    if (lane == 0) out_counts[item] = total;
}

}  // namespace bmf
