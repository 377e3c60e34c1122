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
//   bmf_vote_kernel_lists  one workgroup of W waves per (window, orientation), W = 1 or, where the counters leave room for
//                          few workgroups per CU, 2 or 4 (below: "Several waves per item"; what follows first describes
//                          one wave); the list entries of the sample kernel are the extents
//                          of the sampled k-mers' lists (DevParams::pair == 2; kmer_extent_pack below: the sample
//                          kernel reads offsets[x] and offsets[x + 1], so an item goes from {list_n, its extents},
//                          loaded together, straight to the units).  Per-item hit counters in LDS, BITS = 4 (S <= 15)
//                          or 8 bits per bucket packed in dwords, incremented with LDS atomic adds.  A returning add
//                          brings back the count before, so the wave knows its highest hit count without looking at
//                          the counters.  misses = S - hits: an item whose highest count is at most S - F is empty and
//                          is done; the others scan the counters once, in bucket order, for the buckets at the
//                          maximum (ids staged in LDS: more than max_candidates of them is "cleared").
//                          Two phases.  The counter of bucket b ends at h(b), the number of the item's S lists that
//                          hold b, and the kernel needs only whether max h >= S - F + 1 and, if so, max h exactly.
//                          So the first n_plain = S - F lists (0 when F >= S) are counted with plain adds, no return
//                          and no fold (kmer_unit_plain), then comes a fence, then the other lists with returning adds
//                          (kmer_count_units).  After the plain phase no counter exceeds S - F, so a counter that ends
//                          at h >= S - F + 1 takes its last increment from a returning add, which brings back h - 1
//                          and folds h; if no counter gets that far the folded maximum is at most S - F and the item
//                          is empty, as it should be.  Unlike the all-returning form this depends on the order of the
//                          adds, and it is exact under two invariants:
//                            1. at most S - F lists of an item are counted with plain adds, each of them wholly (its
//                               first 64 units and whatever tail lies beyond them);
//                            2. every plain add precedes the fence and every returning add follows it: plain heads,
//                               then the plain lists' tails, the fence, then returning heads and returning tails.
//                          The LDS executes one wave's instructions in issue order, so issue order is enough in
//                          hardware; the wavefront-scope release/acquire pair with wave_barrier keeps the compiler from
//                          moving a relaxed atomic across it (it compiles to no instruction).
//                          The returning adds are not waited for one by one: the eight of a unit are issued back to
//                          back, with no branch per id (a padding id adds 0 where it harms nothing), and folded into
//                          the maximum after the next unit's are issued.  A plain padding id adds a nonzero value at
//                          a dword nobody reads (kmer_unit_plain).
//                          Both unit bodies stand in each of the 16 unrolled slots behind wave-uniform tests (slot
//                          i is plain iff i < np, returning iff i >= np), not one kernel per plain count: 5 574
//                          instructions, about 33 KiB of the 64 KiB instruction cache, and n_plain stays a run-time
//                          value from DevParams.
//                          A workgroup is one wave and one item, and starts by zeroing its counters: ceil(NB / 128 or
//                          64) 16-byte LDS stores per lane round, far fewer instructions than a second walk over the
//                          lists would be.  (One resident round of waves, each walking its items with the next items'
//                          loads issued ahead, was built and measured slower than this: profiles/r07/README.md.)
//                          Nothing depends on lists being short: the first 64 units of up to 16 lists are in flight
//                          at once, what lies beyond them is walked four wave loads at a time.
//                          Several waves per item (template parameter W; build_kmer_lists chooses once per load,
//                          BMF_LISTS_ITEM_WAVES forces).  One wave needs about 12 us per item whatever runs beside it,
//                          and at the headline shape the counters (13.2 KB) let 11 workgroups reside per CU: 11 waves
//                          out of 32.  An item's S lists are independent streams of atomic adds into one array, so
//                          W waves of one workgroup share the item and its counters: as many workgroups, W times the
//                          waves, and each wave's chain of instructions, LDS round trips and zeroing about 1/W as long.
//                            - Wave w owns the lists s = w, w + W, w + 2 W ... (lane j of the wave holds the extent of
//                              its list j); its heads go K = 16 / W lists at a time.  A wave with no list (S <= w)
//                              loads and adds nothing and takes part in every barrier.
//                            - The zeroing stores are spread over the 64 W lanes; a workgroup barrier follows, since a
//                              wave's adds land in dwords another wave zeroed.
//                            - The two invariants hold for the workgroup: (1) at most S - F lists of the item are
//                              plain, each wholly -- the first S - F in sample order as before, so the plain lists of
//                              wave w are those of its share with s < S - F, the first ones of its own numbering;
//                              (2) every plain add of every wave precedes every returning add of every wave: each wave
//                              issues its plain heads and its plain lists' tails, waits for them (lgkmcnt(0): an LDS
//                              operation has then been executed) and meets ONE workgroup barrier (kmer_item_sync),
//                              then come its returning heads and tails.  The adds are atomic per dword, so after the
//                              barrier no counter exceeds S - F, and a counter that ends at h >= S - F + 1 takes its
//                              last increment, in the LDS's own order, from a returning add of some wave, which
//                              brings back h - 1; that wave folds h.
//                            - Each wave reduces its maximum; the W maxima meet in W dwords of LDS behind a barrier
//                              (which also puts every add before the scan), so the "empty" exit is taken by all waves
//                              or by none, like the list_n == 0 exit.  No wave leaves before a barrier others reach.
//                            - Each wave scans a contiguous range of the counter groups and stages its ids in its own
//                              64 dwords; the W match counts meet in LDS, the item is cleared iff their sum exceeds
//                              max_candidates, else wave w writes its ids behind those of the waves before it: the
//                              same bytes in out_buckets[0 .. count) as with one wave.
//                            - A padding id of a plain unit adds at the dword of its own lane of its own wave in the
//                              staging area (64 W dwords, none of them read before it is overwritten); where the
//                              padding id's dword lies inside the counters (NB > 65 528) it is the top field of the
//                              last dword, no bucket, for every wave alike.
//                          LDS per workgroup: the counters + 256 W bytes of staging + 32 bytes of exchange words
//                          (W > 1).  W = 1 compiles to the one-wave kernel as it was (wavefront-scope fences, no
//                          barrier).  Registers: W = 2 is held to 6 waves per SIMD (75 VGPRs), so that 11 workgroups =
//                          22 waves fit; W = 4 to 7 (67 VGPRs: 7 workgroups = 28 waves; 8 per SIMD would spill).
//   bmf_vote_kernel_cells  the same vote where the lists are sparse (host/lists_cells_rule.h decides, once per load;
//                          S <= 31, F <= S): every id is counted into its CELL of 4 or 8 consecutive buckets first, in
//                          byte counters half or a quarter the size of the 4-bit ones, plain adds only, in any order.  A
//                          cell's sum is at least the highest hit count among its buckets, so an item none of whose
//                          cells reaches S - F + 1 -- the wrong orientation of a read, a read that maps nowhere: half
//                          of all items -- is empty and leaves after one scan; an item that keeps 1 .. 8 cells walks
//                          its units again (two or four waves: the heads still in registers; one wave: from the L2)
//                          and counts hits per bucket of those cells alone; one that keeps more is appended to the
//                          overflow list.  The comment above the kernel has the argument, the LDS layout and the
//                          registers.  LDS no longer limits the residency, the registers do (W = 2: 73 VGPRs, 6 waves
//                          per SIMD, 12 items per CU; W = 1: 74 VGPRs, 24 items; W = 4: 50 VGPRs, 8 items).
//   bmf_vote_kernel_lists_over  the overflow list's items, by the full-width vote (kmer_vote_item, the body of
//                          bmf_vote_kernel_lists): one resident round of workgroups walks the list, launched behind
//                          the cells kernel in every run, so the host makes no round trip.
#pragma once

#include "bmf_kernels.hip.h"

namespace bmf {

constexpr uint32_t kPadId = 0xFFFFu;

// A list entry (DevParams::pair == 2): the extent of the sampled k-mer's list, written by the sample kernel from
// offsets[x] and offsets[x + 1] -- the first unit in the low 48 bits, the unit count in the high 16.  The longest list
// holds all of 65 535 ids, ceil(65 535 / 8) = 8 192 units; 2^48 units are 4 PiB of ids, far beyond any device, and
// build_kmer_lists refuses a table that would not fit (the pair table serves then), like one that does not fit memory.
constexpr uint64_t kKmerExtentFirstMax = (1ull << 48) - 1ull;
constexpr uint32_t kKmerExtentUnitsMax = 0xFFFFu;
__host__ __device__ constexpr uint64_t kmer_extent_pack(uint64_t first, uint32_t n_units) {
    return first | ((uint64_t)n_units << 48);
}
__host__ __device__ constexpr uint64_t kmer_extent_first(uint64_t e) { return e & kKmerExtentFirstMax; }
__host__ __device__ constexpr uint32_t kmer_extent_units(uint64_t e) { return (uint32_t)(e >> 48); }
static_assert(kKmerExtentUnitsMax >= (65535u + 7u) / 8u, "the longest list: all of 65 535 ids");
static_assert(kmer_extent_first(kmer_extent_pack(kKmerExtentFirstMax, kKmerExtentUnitsMax)) == kKmerExtentFirstMax &&
                  kmer_extent_units(kmer_extent_pack(kKmerExtentFirstMax, kKmerExtentUnitsMax)) == kKmerExtentUnitsMax,
              "both fields at their maxima");
static_assert(kmer_extent_first(kmer_extent_pack(kKmerExtentFirstMax, 0u)) == kKmerExtentFirstMax &&
                  kmer_extent_units(kmer_extent_pack(kKmerExtentFirstMax, 0u)) == 0u &&
                  kmer_extent_first(kmer_extent_pack(0u, kKmerExtentUnitsMax)) == 0u &&
                  kmer_extent_units(kmer_extent_pack(0u, kKmerExtentUnitsMax)) == kKmerExtentUnitsMax,
              "neither field reaches into the other");

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

// LDS bytes per workgroup of bmf_vote_kernel_lists: the counters, rounded up to whole 16-byte stores, then the staging
// area: a dword per lane of each of the item's `waves` waves (its padding ids add there, its ids at the maximum are
// staged there), and behind them, where several waves share the item, the words through which their maxima and their
// match counts meet (2 per wave)
inline uint32_t kmer_vote_counter_bytes(uint32_t nb, uint32_t bits) { return ((nb * bits + 127u) / 128u) * 16u; }
inline uint32_t kmer_vote_lds_bytes(uint32_t nb, uint32_t bits, uint32_t waves = 1u) {
    return kmer_vote_counter_bytes(nb, bits) + waves * 64u * 4u + (waves == 1u ? 16u : 32u);
}

// What separates the phases of an item.  One wave: the LDS executes a wave's instructions in issue order, the
// wavefront-scope pair only keeps the compiler from moving a relaxed atomic across (no instruction).  W > 1 waves: a
// workgroup barrier behind a workgroup-scope release (the wave's LDS operations, plain adds included, have been
// executed: s_waitcnt lgkmcnt(0)), so every LDS operation any wave issued before it precedes every one issued after it.
// Every wave of the workgroup reaches every one of these, the same number of times.
template <int W>
__device__ __forceinline__ void kmer_item_sync() {
    if constexpr (W == 1) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

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

// The eight ids of one unit of a plain list (see bmf_vote_kernel_lists): adds whose result nobody uses (ds_add_u32), so
// nothing to wait for and nothing to fold.  A padding id adds its 1 << ... as well, where nobody reads: at the lane's dword
// of the staging area (written only after the counting, read only below `total`), or, where its own dword lies inside
// the counters (NB > 65 528 in the 4-bit form), in the top field of the last counter dword, which is no bucket (the scan
// masks the fields >= NB, and a carry out of the top field leaves the dword).  That garbage is never read, and it spares
// the add path the `id < nb` compare and select.
// Precondition (bmf_kmer_fill_kernel keeps it): the only id >= NB in a list is kPadId, whose field is the top one of its
// dword in both forms (field 7 of dword 8 191, field 3 of dword 16 383), and NB <= 65 535.  Any other id >= NB would
// count in a bucket's field; kmer_unit_issue, which adds 0 for every id >= NB, does not need the precondition.
template <int BITS>
__device__ __forceinline__ void kmer_unit_plain(uint32_t *cnt, uint32_t spare, const uint4 &u, uint32_t nb) {
    constexpr uint32_t kPer = 32u / BITS;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
    if ((w[0] & 0xFFFFu) < nb) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t id = j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xFFFFu;
            atomicAdd(&cnt[min(id / kPer, spare)], 1u << ((id % kPer) * BITS));
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
// has been folded.  Only u[from .. N - 1] are counted (from < N, wave-uniform: the units before them belong to plain lists).
template <int BITS, int N, class After>
__device__ __forceinline__ uint32_t kmer_count_units(uint32_t *cnt, uint32_t spare, const uint4 (&u)[N], uint32_t nb, uint32_t mx,
                                                     After after, uint32_t from = 0) {
    uint32_t old[2][8];
#pragma unroll
    for (int i = 0; i < N; i++) {
        if ((uint32_t)i < from) continue;
        kmer_unit_issue<BITS>(cnt, spare, u[i], nb, old[i & 1]);
        if ((uint32_t)i > from) {
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

// Lane s holds where the list of sample s starts (in units, two halves) and how many units it has.  The sample asked
// for is wave-uniform, so its extent is read into scalar registers (no LDS permute): a unit's address is then a scalar
// base plus the lane.
struct KmerListExtents {
    uint32_t first_lo, first_hi, n_units;
    __device__ __forceinline__ uint32_t units_of(uint32_t s) const {
        return (uint32_t)__builtin_amdgcn_readlane((int)n_units, (int)s);
    }
    __device__ __forceinline__ uint64_t first_of(uint32_t s) const {
        return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)first_hi, (int)s) << 32) |
               (uint32_t)__builtin_amdgcn_readlane((int)first_lo, (int)s);
    }
};

// What lies beyond the first 64 units of the lists s_begin .. s_end - 1, four wave loads at a time: plain adds, or
// returning ones folded into mx.
template <int BITS, bool PLAIN>
__device__ __forceinline__ uint32_t kmer_count_tails(uint32_t *cnt, uint32_t spare, const uint4 *__restrict__ units,
                                                     const KmerListExtents &ext, uint32_t s_begin, uint32_t s_end, uint32_t nb,
                                                     uint32_t mx, uint32_t lane) {
    for (uint32_t s = s_begin; s < s_end; s++) {
        const uint32_t n = ext.units_of(s);
        if (n <= (uint32_t)kWave) continue;
        const uint4 *list = units + ext.first_of(s);
        for (uint32_t at = kWave; at < n; at += 4u * kWave) {
            uint4 u[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t t = at + (uint32_t)i * kWave + lane;
                u[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
                if (t < n) u[i] = list[t];
            }
            if (PLAIN) {
#pragma unroll
                for (int i = 0; i < 4; i++) kmer_unit_plain<BITS>(cnt, spare, u[i], nb);
            } else {
                mx = kmer_count_units<BITS>(cnt, spare, u, nb, mx, [](int) {});
            }
        }
    }
    return mx;
}

// W waves per item (1, 2 or 4; the host chooses once per load).  Heads in flight per wave and batch: 16 lists for one
// wave, 8 or 4 where the item's lists are shared out, so that the registers of a wave shrink as the waves per CU grow.
template <int W>
constexpr int kmer_vote_batch() { return W == 1 ? 16 : (W == 2 ? 8 : 4); }
// ... and the waves per SIMD the registers must leave room for: 11 workgroups of 2 waves are 22 waves on 4 SIMDs; 4
// waves per item get 7 (7 workgroups: at 8 per SIMD the kernel spills); one wave: 1, no demand
template <int W>
constexpr int kmer_vote_waves_per_simd() { return W == 1 ? 1 : (W == 2 ? 6 : 7); }

// One item of the full-width vote (the header comment), by the whole workgroup: bmf_vote_kernel_lists calls it with
// its block number, bmf_vote_kernel_lists_over with the items the cells form handed over.
template <int BITS, int W>
__device__ __forceinline__ void kmer_vote_item(uint32_t *lds_cnt, const DevParams &P, const uint4 *__restrict__ units,
                                               const uint64_t *__restrict__ kmer_extents, const uint32_t *__restrict__ list_n,
                                               uint32_t *__restrict__ out_counts, uint32_t *__restrict__ out_buckets,
                                               const uint32_t item) {
    static_assert(W == 1 || W == 2 || W == 4, "waves per item");
    constexpr uint32_t kPer = 32u / BITS, kField = (1u << BITS) - 1u;
    constexpr uint32_t kTop = BITS == 4 ? 0x88888888u : 0x80808080u, kLow = ~kTop;
    constexpr int K = kmer_vote_batch<W>();
    const uint32_t tid = threadIdx.x;
    // the wave's number within the item (scalar) and the lane within the wave
    const uint32_t wave = W == 1 ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / (uint32_t)kWave));
    const uint32_t lane = W == 1 ? tid : tid % (uint32_t)kWave;
    // The wave's share of the item's lists: the lists s = wave + j W, j = 0 .. n_mine - 1, of which the first np_mine
    // are plain (s < n_plain: the item's first S - F lists in sample order, as with one wave).  Lane j holds the extent
    // of the wave's list j.  A wave with no list (S <= wave) loads and adds nothing.
    const uint32_t n_plain = P.S > P.F ? P.S - P.F : 0u;           // lists 0 .. n_plain - 1 of the item are the plain ones
    const uint32_t n_mine = W == 1 ? P.S : (P.S > wave ? (P.S - wave + (uint32_t)W - 1u) / (uint32_t)W : 0u);
    const uint32_t np_mine = W == 1 ? n_plain : (n_plain > wave ? (n_plain - wave + (uint32_t)W - 1u) / (uint32_t)W : 0u);
    // list_n and the extents are both addressed by `item` alone, so both loads are issued before the branch on list_n:
    // one level of global-load latency ahead of the units, not two.  The extents of a rejected window are stale (an
    // earlier batch's) or were never written: loaded, since the buffer is there for every window, and not used
    uint64_t extent = 0;
    if (lane < n_mine) extent = kmer_extents[(size_t)item * (P.list_len >> 1) + wave + lane * (uint32_t)W];
    if (list_n[item >> 1] == 0) {              // window rejected by the sample kernel (the whole workgroup leaves)
        if (tid == 0) out_counts[item] = 0;
        return;
    }
    const uint32_t n_dw = (P.nb + kPer - 1u) / kPer, n_q = (n_dw + 3u) >> 2;   // counter dwords, 16-byte groups of them
    uint32_t *stage = lds_cnt + n_q * 4u + wave * (uint32_t)kWave;   // the wave's [0..63] ids at the maximum
    uint32_t *xch = lds_cnt + n_q * 4u + (uint32_t)(W * kWave);      // W > 1: [w] wave w's maximum, [W + w] its matches
    const uint32_t spare = n_q * 4u + tid;     // the lane's dword of the staging area, where its padding ids add: 0 from a
                                               // returning unit, garbage from a plain one.  Harmless: every add precedes
                                               // the scan, which overwrites stage[0 .. total - 1] before those are read

    // (the extents arrive while the counters are zeroed)
    for (uint32_t i = tid; i < n_q; i += (uint32_t)(W * kWave)) reinterpret_cast<uint4 *>(lds_cnt)[i] = make_uint4(0, 0, 0, 0);
    kmer_item_sync<W>();                       // W > 1: the wave's adds land in dwords another wave zeroed

    const uint64_t first = kmer_extent_first(extent);               // a lane >= n_mine holds extent 0: no units
    const uint32_t n_units = kmer_extent_units(extent);
    const KmerListExtents ext{(uint32_t)first, (uint32_t)(first >> 32), n_units};
    const bool tails = __ballot(n_units > (uint32_t)kWave) != 0;   // heavy k-mers; one with no indexed q-gram holds all NB ids
    bool fenced = n_plain == 0;                                    // no plain list: the kernel is the all-returning one
    uint32_t mx = 0;
    for (uint32_t s0 = 0; s0 < n_mine; s0 += (uint32_t)K) {
        // the first 64 units of up to K lists, all issued before the first is counted.  No `s0 + i < n_mine` test:
        // S <= 64 (the library refuses more), so s0 + i <= 63 names a lane, and a lane >= n_mine holds n_units 0:
        // nothing is loaded
        uint4 u[K];
#pragma unroll
        for (int i = 0; i < K; i++) {
            const uint32_t n = ext.units_of((s0 + i) & 63u);
            u[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            if (lane < n) u[i] = units[ext.first_of((s0 + i) & 63u) + lane];
        }
        const uint32_t np = np_mine > s0 ? min(np_mine - s0, (uint32_t)K) : 0u;   // the plain ones among these K come first
#pragma unroll
        for (int i = 0; i < K; i++)
            if ((uint32_t)i < np) kmer_unit_plain<BITS>(lds_cnt, spare, u[i], P.nb);
        if (np == (uint32_t)K) continue;
        if (!fenced) {
            // the wave's last plain head is issued: its plain lists' tails, then the fence of invariant 2, once
            fenced = true;
            if (tails) kmer_count_tails<BITS, true>(lds_cnt, spare, units, ext, 0u, np_mine, P.nb, 0u, lane);
            kmer_item_sync<W>();
        }
        mx = kmer_count_units<BITS>(lds_cnt, spare, u, P.nb, mx, [](int) {}, np);
    }
    if constexpr (W > 1) {
        // a wave whose lists are all plain, or that has none, has not met the fence in the loop: the others wait there
        if (!fenced) {
            if (tails) kmer_count_tails<BITS, true>(lds_cnt, spare, units, ext, 0u, np_mine, P.nb, 0u, lane);
            kmer_item_sync<W>();
        }
    }
    if (tails) mx = kmer_count_tails<BITS, false>(lds_cnt, spare, units, ext, np_mine, n_mine, P.nb, mx, lane);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, kWave));
    if constexpr (W > 1) {
        // the item's maximum is the highest of the waves': through xch, so that all of them leave here or none does
        if (lane == 0) xch[wave] = mx;
        kmer_item_sync<W>();                    // and every add of every wave precedes the scan
#pragma unroll
        for (int w = 0; w < W; w++) mx = max(mx, xch[w]);
        mx = (uint32_t)__builtin_amdgcn_readfirstlane((int)mx);
    }
    // fewest misses = S - mx; nothing below F misses: every level of the reference's filter is empty
    if (mx + P.F <= P.S) {
        if (tid == 0) out_counts[item] = 0;
        return;                                 // (the counters die with the workgroup)
    }
    if constexpr (W == 1) kmer_item_sync<W>();
    // the buckets whose counter is mx, in ascending order: lane l of round r holds counter dwords 4 (64 r + l) .. + 3.
    // Wave w scans the rounds w R .. (w + 1) R - 1, R = ceil(rounds / W): contiguous, so the waves' ids, one wave after
    // the other, are in ascending order
    uint32_t q_begin = 0, q_end = n_q;
    if constexpr (W > 1) {
        const uint32_t per_wave = (((n_q + (uint32_t)kWave - 1u) / (uint32_t)kWave + (uint32_t)W - 1u) / (uint32_t)W) * (uint32_t)kWave;
        q_begin = min(wave * per_wave, n_q);
        q_end = min(q_begin + per_wave, n_q);
    }
    const uint32_t want = mx * (0xFFFFFFFFu / kField);        // mx in every field
    uint32_t total = 0;
    for (uint32_t q0 = q_begin; q0 < q_end; q0 += kWave) {
        const uint32_t qi = q0 + lane;
        uint4 v = make_uint4(~want, ~want, ~want, ~want);
        if (qi < q_end) v = reinterpret_cast<const uint4 *>(lds_cnt)[qi];
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
        if (total > P.max_cand) break;          // cleared whatever follows (wave-uniform; W > 1: whatever the others found)
    }
    uint32_t base = 0, all = total;             // ids of the waves before this one, of all waves
    if constexpr (W > 1) {
        if (lane == 0) xch[W + wave] = total;
        kmer_item_sync<W>();
        all = 0;
#pragma unroll
        for (int w = 0; w < W; w++) {
            const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)xch[W + w]);
            if ((uint32_t)w < wave) base += t;
            all += t;
        }
    }
    if (all > P.max_cand) {                     // q_gram_mapper.h:471-476
        if (tid == 0) out_counts[item] = 0;
        return;
    }
    if constexpr (W == 1) kmer_item_sync<W>();
    // all <= max_candidates <= 64: every id of every wave is staged
    if (lane < total) out_buckets[(size_t)item * P.max_cand + base + lane] = stage[lane];
    if (tid == 0) out_counts[item] = all;
}

template <int BITS, int W = 1>
__global__ __launch_bounds__(kWave * W) __attribute__((amdgpu_waves_per_eu(kmer_vote_waves_per_simd<W>()))) void bmf_vote_kernel_lists(DevParams P, const uint4 *__restrict__ units,
                                                                  const uint64_t *__restrict__ kmer_extents,
                                                                  const uint32_t *__restrict__ list_n,
                                                                  uint32_t *__restrict__ out_counts,
                                                                  uint32_t *__restrict__ out_buckets) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cnt[];
    kmer_vote_item<BITS, W>(lds_cnt, P, units, kmer_extents, list_n, out_counts, out_buckets, blockIdx.x);
}

// ---- the cells form ----
//
// A bucket qualifies with h >= t = S - F + 1 hits.  Buckets are grouped into cells of C = 2^CELL consecutive ids and
// every id of every list is counted into its cell first:
//   - a cell's sum is the sum of h(b) over its buckets, so it is at least the highest h(b) among them;
//   - a cell whose sum is below t therefore holds no qualifying bucket;
//   - every qualifying bucket lies in a cell whose sum is at least t.
// The ids of a list are distinct, so a cell's sum is at most C S <= 8 * 31 = 248: byte fields hold it (the host takes
// the form only for 1 <= t, S <= 31).  The cell counters take ceil(NB / C) bytes, half or a quarter of the 4-bit
// counters, every add is a plain ds_add_u32, and nothing depends on the order of the adds.  Only an item that keeps
// 1 .. kCellsKeep cells counts hits per bucket, in kCellsKeep * C byte counters, over a second walk of its units that
// adds the ids of the kept cells alone; an item that keeps more goes to the full-width kernel through the overflow list.
constexpr uint32_t kCellsKeep = 8;       // T: cells an item may keep; T * C >= max_candidates + 1 is decided here for C = 8
constexpr uint32_t kOverHead = 4;        // the overflow list: [0] the count (reset on the stream in every run), items from [4]

// LDS bytes per workgroup of bmf_vote_kernel_cells: the cell counters rounded up to whole 16-byte stores, a dword per
// lane of each wave (its padding ids add there; its kept cells are staged in the first kCellsKeep), the byte counters of
// the kept cells' buckets (64 bytes) and the exchange words (a dword per wave, 16 bytes)
inline uint32_t kmer_cells_counter_bytes(uint32_t nb, uint32_t cell) { return ((((nb + (1u << cell) - 1u) >> cell) + 15u) / 16u) * 16u; }
inline uint32_t kmer_cells_lds_bytes(uint32_t nb, uint32_t cell, uint32_t waves) {
    return kmer_cells_counter_bytes(nb, cell) + waves * 64u * 4u + kCellsKeep * 8u + 16u;
}

// The eight ids of one unit into their cells.  A padding id adds as well, where nobody reads: at the lane's dword of the
// staging area, or, where its dword lies inside the counters, in a field that is no cell (the scan masks it) or in the
// last cell's (NB > 65 535 - C: that cell is kept whatever it holds, see the scan).  Precondition, as for
// kmer_unit_plain: the only id >= NB in a list is kPadId.  A lane that holds no unit (all ones) takes no part.
template <int CELL>
__device__ __forceinline__ void kmer_unit_cells(uint32_t *cnt, uint32_t spare, const uint4 &u) {
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
    if ((w[0] & 0xFFFFu) != kPadId) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t cell = (j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xFFFFu) >> CELL;
            atomicAdd(&cnt[min(cell >> 2, spare)], 1u << ((cell & 3u) * 8u));
        }
    }
}

// The ids of one unit that lie in the kept cell whose first bucket is `base`, into that cell's C byte counters at
// `small`.  A list ascends, so a unit meets [base, base + C) only if its first id lies below base + C and its last one
// (a padding id is the highest) at or above base: two compares turn most units away.  A padding id counts in the field
// of bucket 65 535, which is no bucket (only where the last cell is kept and NB > 65 535 - C); at most 7 S + 8 of them
// meet a field the caller never reads as a bucket's, the top one of its dword.
template <int CELL>
__device__ __forceinline__ void kmer_unit_exact(uint32_t *small, uint32_t base, const uint4 &u) {
    constexpr uint32_t C = 1u << CELL;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
    if ((w[0] & 0xFFFFu) < base + C && (w[3] >> 16) >= base && (w[0] & 0xFFFFu) != kPadId) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t d = (j & 1 ? w[j >> 1] >> 16 : w[j >> 1] & 0xFFFFu) - base;
            if (d < C) atomicAdd(&small[d >> 2], 1u << ((d & 3u) * 8u));
        }
    }
}

// Waves per SIMD the registers of the cells kernel must leave room for; the LDS no longer limits the residency.
//   W = 1   6: 74 VGPRs, 24 items per CU (7 per SIMD spills 4 registers)
//   W = 2   6: 73 VGPRs with the heads kept for the exact phase, 12 items per CU.  Loading them again instead needs 43
//           VGPRs, 8 waves per SIMD, 16 items per CU -- and was measured SLOWER (vote 5.73 ms against 5.44 ms at the
//           headline shape, profiles/r20/README.md): the second pass over the units costs more than the residency buys.
//           (Keeping them at 7 per SIMD spills 4 registers.)
//   W = 4   8: 50 VGPRs, 8 items per CU
template <int W>
constexpr int kmer_cells_waves_per_simd() { return W == 4 ? 8 : 6; }

template <int CELL, int W>
__global__ __launch_bounds__(kWave * W) __attribute__((amdgpu_waves_per_eu(kmer_cells_waves_per_simd<W>()))) void bmf_vote_kernel_cells(DevParams P, const uint4 *__restrict__ units,
                                                                  const uint64_t *__restrict__ kmer_extents,
                                                                  const uint32_t *__restrict__ list_n,
                                                                  uint32_t *__restrict__ out_counts,
                                                                  uint32_t *__restrict__ out_buckets,
                                                                  uint32_t *__restrict__ over) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cnt[];
    static_assert(W == 1 || W == 2 || W == 4, "waves per item");
    static_assert(CELL == 2 || CELL == 3, "cells of 4 or 8 buckets");
    constexpr uint32_t C = 1u << CELL;
    constexpr int K = kmer_vote_batch<W>();
    const uint32_t tid = threadIdx.x, item = blockIdx.x;
    const uint32_t wave = W == 1 ? 0u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid / (uint32_t)kWave));
    const uint32_t lane = W == 1 ? tid : tid % (uint32_t)kWave;
    // the wave's share of the item's lists, as in kmer_vote_item: s = wave + j W, lane j holds the extent of list j
    const uint32_t n_mine = W == 1 ? P.S : (P.S > wave ? (P.S - wave + (uint32_t)W - 1u) / (uint32_t)W : 0u);
    uint64_t extent = 0;
    if (lane < n_mine) extent = kmer_extents[(size_t)item * (P.list_len >> 1) + wave + lane * (uint32_t)W];
    if (list_n[item >> 1] == 0) {              // window rejected by the sample kernel (the whole workgroup leaves)
        if (tid == 0) out_counts[item] = 0;
        return;
    }
    const uint32_t n_cells = (P.nb + C - 1u) >> CELL, n_dw = (n_cells + 3u) >> 2, n_q = (n_dw + 3u) >> 2;
    uint32_t *stage = lds_cnt + n_q * 4u;                            // [64 w + i]: wave w's i-th kept cell, i < kCellsKeep
    uint32_t *small = stage + (uint32_t)(W * kWave);                 // [2 j ..]: the C byte counters of kept cell j (C = 4: [j])
    uint32_t *xch = small + kCellsKeep * 2u;                         // [w]: cells wave w keeps
    const uint32_t spare = n_q * 4u + tid;     // the lane's dword of the staging area, where its padding ids add

    for (uint32_t i = tid; i < n_q; i += (uint32_t)(W * kWave)) reinterpret_cast<uint4 *>(lds_cnt)[i] = make_uint4(0, 0, 0, 0);
    if (tid < kCellsKeep * 2u) small[tid] = 0;
    kmer_item_sync<W>();

    const uint64_t first = kmer_extent_first(extent);
    const uint32_t n_units = kmer_extent_units(extent);
    const KmerListExtents ext{(uint32_t)first, (uint32_t)(first >> 32), n_units};
    const bool tails = __ballot(n_units > (uint32_t)kWave) != 0;
    auto heads = [&](uint32_t s0, uint4 (&u)[K]) {
#pragma unroll
        for (int i = 0; i < K; i++) {
            const uint32_t n = ext.units_of((s0 + i) & 63u);
            u[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            if (lane < n) u[i] = units[ext.first_of((s0 + i) & 63u) + lane];
        }
    };
    // what lies beyond the first 64 units of the wave's lists, four wave loads at a time
    auto walk_tails = [&](auto &&unit) {
        for (uint32_t s = 0; s < n_mine; s++) {
            const uint32_t n = ext.units_of(s);
            if (n <= (uint32_t)kWave) continue;
            const uint4 *list = units + ext.first_of(s);
            for (uint32_t at = kWave; at < n; at += 4u * kWave) {
                uint4 v[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t t = at + (uint32_t)i * kWave + lane;
                    v[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
                    if (t < n) v[i] = list[t];
                }
#pragma unroll
                for (int i = 0; i < 4; i++) unit(v[i]);
            }
        }
    };

    // ---- cell phase: every id of every list ----
    uint4 u[K];                                // the heads of the last batch stay: the exact phase reads them again
    uint32_t s0 = 0;
    do {                                       // (a wave with no list loads nothing: its u is all ones)
        heads(s0, u);
#pragma unroll
        for (int i = 0; i < K; i++) kmer_unit_cells<CELL>(lds_cnt, spare, u[i]);
        s0 += (uint32_t)K;
    } while (s0 < n_mine);
    if (tails) walk_tails([&](const uint4 &v) { kmer_unit_cells<CELL>(lds_cnt, spare, v); });
    kmer_item_sync<W>();                       // every add of every wave precedes the scan

    // ---- scan: the cells whose sum is at least t, in ascending order ----
    // Field x of a dword, x <= 248, against t, 1 <= t <= 31: x >= 128 has its top bit set; else (x & 127) + (128 - t)
    // stays below 256 and has its top bit set iff x >= t.
    // The padding id's cell, where it is a cell at all (NB > 65 535 - C: the last one, the top field of the last
    // dword), also counted up to 7 padding ids per list and may have wrapped: it is kept whatever it holds, and the
    // exact phase decides.
    const uint32_t t_min = P.S - P.F + 1u;
    const uint32_t add_c = (128u - t_min) * 0x01010101u;
    const uint32_t pad_dw = (kPadId >> CELL) < n_cells ? (kPadId >> CELL) >> 2 : 0xFFFFFFFFu;
    uint32_t q_begin = 0, q_end = n_q;
    if constexpr (W > 1) {
        const uint32_t per_wave = (((n_q + (uint32_t)kWave - 1u) / (uint32_t)kWave + (uint32_t)W - 1u) / (uint32_t)W) * (uint32_t)kWave;
        q_begin = min(wave * per_wave, n_q);
        q_end = min(q_begin + per_wave, n_q);
    }
    uint32_t kept = 0;
    for (uint32_t q0 = q_begin; q0 < q_end; q0 += kWave) {
        const uint32_t qi = q0 + lane;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (qi < q_end) v = reinterpret_cast<const uint4 *>(lds_cnt)[qi];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t ge[4], pc = 0;
#pragma unroll
        for (int x = 0; x < 4; x++) {
            const uint32_t dw = qi * 4u + (uint32_t)x;
            ge[x] = (((w[x] & 0x7F7F7F7Fu) + add_c) | w[x]) & 0x80808080u;
            if (dw == pad_dw) ge[x] |= 0x80000000u;
            const uint32_t left = dw * 4u < n_cells ? n_cells - dw * 4u : 0u;   // fields past the last cell are no cells
            if (left < 4u) ge[x] &= (1u << (left * 8u)) - 1u;
            if (qi >= q_end) ge[x] = 0;
            pc += __popc(ge[x]);
        }
        if (__ballot(pc != 0) == 0) continue;
        uint32_t incl = pc;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o, kWave);
            if (lane >= (uint32_t)o) incl += t;
        }
        uint32_t pos = kept + incl - pc;
        kept += __shfl(incl, kWave - 1, kWave);
#pragma unroll
        for (int x = 0; x < 4; x++) {
            uint32_t bits = ge[x];
            while (bits) {
                if (pos < kCellsKeep) stage[wave * (uint32_t)kWave + pos] = (qi * 4u + (uint32_t)x) * 4u + (uint32_t)__builtin_ctz(bits) / 8u;
                pos++;
                bits &= bits - 1u;
            }
        }
        if (kept > kCellsKeep) break;           // overflow whatever follows (wave-uniform)
    }
    uint32_t all = kept;
    if constexpr (W > 1) {
        if (lane == 0) xch[wave] = kept;
        kmer_item_sync<W>();                    // the kept cells of every wave are staged
        all = 0;
#pragma unroll
        for (int w = 0; w < W; w++) all += (uint32_t)__builtin_amdgcn_readfirstlane((int)xch[w]);
    } else {
        kmer_item_sync<W>();
    }
    if (all == 0) {                             // no cell reaches t: no bucket does (all waves leave, or none)
        if (tid == 0) out_counts[item] = 0;
        return;
    }
    if (all > kCellsKeep) {                     // the full-width kernel counts this item (bmf_vote_kernel_lists_over)
        if (tid == 0) over[kOverHead + atomicAdd(&over[0], 1u)] = item;
        return;
    }

    // ---- exact phase: hits per bucket of the kept cells ----
    // Two or four waves: where one batch held the wave's whole share (S <= 16 with two waves) its heads are still in
    // u.  One wave: 16 heads are 64 registers, which would halve the waves per SIMD; it loads them again.
    const bool held = W > 1 && n_mine <= (uint32_t)K;
    uint32_t j = 0;
#pragma unroll 1
    for (int w = 0; w < W; w++) {
        const uint32_t n_w = W == 1 ? kept : (uint32_t)__builtin_amdgcn_readfirstlane((int)xch[w]);
#pragma unroll 1
        for (uint32_t i = 0; i < n_w; i++, j++) {
            const uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)stage[(uint32_t)w * (uint32_t)kWave + i]) << CELL;
            uint32_t *small_j = small + j * (C / 4u);
            if (held) {
#pragma unroll
                for (int x = 0; x < K; x++) kmer_unit_exact<CELL>(small_j, base, u[x]);
            } else {
                for (uint32_t s0 = 0; s0 < n_mine; s0 += (uint32_t)K) {   // again from the L2
                    uint4 v[K];
                    heads(s0, v);
#pragma unroll
                    for (int x = 0; x < K; x++) kmer_unit_exact<CELL>(small_j, base, v[x]);
                }
            }
            if (tails) walk_tails([&](const uint4 &v) { kmer_unit_exact<CELL>(small_j, base, v); });
        }
    }
    kmer_item_sync<W>();                        // every add of every wave precedes the reading of the byte counters
    if (wave != 0) return;
    // Lane l holds byte counter l: bucket l % C of kept cell l / C.  The kept cells ascend through the waves' staging
    // areas, so the buckets ascend with the lane.
    uint32_t bucket = 0xFFFFFFFFu, hits = 0;
    if (lane < all * C) {
        uint32_t jj = lane >> CELL, w_of = 0;
        if constexpr (W > 1) {
#pragma unroll
            for (int w = 0; w < W - 1; w++) {
                const uint32_t n_w = xch[w];
                if (w_of == (uint32_t)w && jj >= n_w) {
                    jj -= n_w;
                    w_of++;
                }
            }
        }
        bucket = (stage[w_of * (uint32_t)kWave + jj] << CELL) + (lane & (C - 1u));
        hits = (small[lane >> 2] >> ((lane & 3u) * 8u)) & 0xFFu;
    }
    const bool is_bucket = bucket < P.nb;       // (the last cell may reach past NB; the padding id's field is there)
    uint32_t mx = is_bucket ? hits : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, kWave));
    // fewest misses = S - mx; nothing below F misses: every level of the reference's filter is empty
    if (mx + P.F <= P.S) {
        if (lane == 0) out_counts[item] = 0;
        return;
    }
    const uint64_t at_max = __ballot(is_bucket && hits == mx);
    const uint32_t count = (uint32_t)__popcll(at_max);
    if (count > P.max_cand) {                   // q_gram_mapper.h:471-476
        if (lane == 0) out_counts[item] = 0;
        return;
    }
    if ((at_max >> lane) & 1ull) out_buckets[(size_t)item * P.max_cand + (uint32_t)__popcll(at_max & ((1ull << lane) - 1ull))] = bucket;
    if (lane == 0) out_counts[item] = count;
}

// The items the cells kernel could not decide (more than kCellsKeep cells kept: a k-mer with no indexed q-gram, dense
// rows, repeats), counted by the full-width vote.  A fixed grid of resident workgroups walks over[kOverHead ..
// kOverHead + over[0]); outputs are addressed by item, so the order of the list changes nothing.
// (the loop over items takes a few registers more than one item does: a wave per SIMD fewer than bmf_vote_kernel_lists,
// so that nothing spills -- a wave that needs scratch is slow to start, and this kernel is launched in every run)
template <int W>
constexpr int kmer_over_waves_per_simd() { return W == 1 ? 1 : (W == 2 ? 5 : 6); }

template <int BITS, int W>
__global__ __launch_bounds__(kWave * W) __attribute__((amdgpu_waves_per_eu(kmer_over_waves_per_simd<W>()))) void bmf_vote_kernel_lists_over(DevParams P, const uint4 *__restrict__ units,
                                                                  const uint64_t *__restrict__ kmer_extents,
                                                                  const uint32_t *__restrict__ list_n,
                                                                  uint32_t *__restrict__ out_counts,
                                                                  uint32_t *__restrict__ out_buckets,
                                                                  const uint32_t *__restrict__ over) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_cnt[];
    const uint32_t n_over = over[0];
    for (uint32_t i = blockIdx.x; i < n_over; i += gridDim.x) {
        kmer_vote_item<BITS, W>(lds_cnt, P, units, kmer_extents, list_n, out_counts, out_buckets, over[kOverHead + i]);
        kmer_item_sync<W>();                    // the next item's zeroing behind this item's last reads
    }
}

}  // namespace bmf

