// bmv_annotate.hip.h -- the annotation pass of the verifier (bmv_annotate, include/bmv.h): one linear walk per alignment
// over text and query that turns the aligner's M/I/D CIGAR into forward-strand =/X/I/D entries, NM, the forward POS and
// the reference bases under every X and D column (MD's payload).  A post-pass of its own: no aligning kernel is touched.
//
// Shape: a wave per alignment, 64 alignment columns of an M entry per step.  The walk runs in FORWARD-strand order from
// the start: for text_rc != 0 the CIGAR is taken from its last entry to its first, the query from its last base to its
// first with complemented ranks, and the text window as it lies in the genome from pos = text_len - begin - R on -- the
// same comparisons the aligner made (rank(text) ^ 3 == rank(query)  <=>  rank(text) == rank(query) ^ 3), already in
// output order, so nothing is reversed afterwards.  Per step one ballot of "ranks differ"; run starts are the bits of
// x ^ (x << 1); a lane that starts a run finds its length with a count of trailing zeros and its output slot with a
// population count; the step's last run stays open (one packed entry in a uniform register) and is merged with the first
// run of the next step when the ops agree.  An I or D entry closes the open run, so `=` runs on both sides of an
// insertion stay two entries.  No LDS, no scratch: the only state is the open run and four counters.
//
// Output sizes depend on the data: the kernel runs twice, WRITE = false counting entries and bases (and writing nm, pos,
// ref_len), then -- after two exclusive sums (bm_scan.hip.h) -- WRITE = true storing them at their offsets.
#pragma once

#include "bm_dna4.hip.h"

namespace bmv {

constexpr uint32_t kAnnotateWaves = 4;          // alignments per 256-thread block
constexpr uint32_t kOpI = 1u, kOpD = 2u, kOpEq = 7u, kOpX = 8u;

struct AnnotateJob {
    const uint8_t *genome;
    const uint8_t *reads;
    const uint64_t *text_start;     // per alignment of the batch
    const uint32_t *text_len;
    const uint8_t *text_rc;
    const uint64_t *query_start;
    const uint32_t *query_len;
    const uint32_t *begin;
    const uint64_t *cigar_offset;   // count + 1
    const uint32_t *cigar;          // M / I / D, validated on the host
    uint32_t count;
    uint32_t *nm, *pos, *ref_len;   // written by the count pass
    uint32_t *n_xcigar, *n_ref;     // counts, written by the count pass
    const uint64_t *xcigar_offset;  // their exclusive sums, read by the write pass
    const uint64_t *ref_offset;
    uint32_t *xcigar;
    uint8_t *ref_bases;
};

__device__ __forceinline__ uint32_t annotate_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool WRITE>
__global__ __launch_bounds__(64 * kAnnotateWaves) void bmv_annotate_kernel(AnnotateJob J) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kAnnotateWaves + (threadIdx.x >> 6)));
    if (a >= J.count) return;
    const uint64_t cig_at = J.cigar_offset[a];
    const uint32_t ne = (uint32_t)(J.cigar_offset[a + 1] - cig_at);
    const uint32_t *cig = J.cigar + cig_at;
    const bool rc = J.text_rc[a] != 0;
    const uint32_t m = J.query_len[a];
    uint32_t pos;
    if (!WRITE) {
        uint32_t r = 0;                                         // reference bases consumed: M and D lengths
        for (uint32_t k = lane; k < ne; k += 64u) {
            const uint32_t e = cig[k];
            r += (e & 15u) != kOpI ? e >> 4 : 0u;
        }
        r = annotate_wave_sum(r);
        pos = ne == 0u ? 0u : (rc ? J.text_len[a] - J.begin[a] - r : J.begin[a]);
        if (lane == 0) {
            J.pos[a] = pos;
            J.ref_len[a] = r;
        }
    } else {
        pos = J.pos[a];
    }
    const uint8_t *T = J.genome + J.text_start[a];
    const uint8_t *Q = J.reads + J.query_start[a];
    uint32_t *out = WRITE ? J.xcigar + J.xcigar_offset[a] : nullptr;
    uint8_t *ref = WRITE ? J.ref_bases + J.ref_offset[a] : nullptr;
    constexpr uint32_t kLetters = 0x54474341u;                  // "ACGT", rank r in byte r

    uint32_t ti = pos, qi = 0;                                  // the next text / query base, forward strand
    uint32_t open = 0;                                          // the run not yet written, packed; 0 = none (lengths are > 0)
    uint32_t n_out = 0, n_ref = 0, nm = 0;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t k = 0; k < ne; k++) {
        const uint32_t e = cig[rc ? ne - 1u - k : k], op = e & 15u, len = e >> 4;
        if (op != 0u) {                                         // I or D: closes the open run and is the open run now
            if (open) {
                if (WRITE && lane == 0) out[n_out] = open;
                n_out++;
            }
            open = e;
            nm += len;
            if (op == kOpI) {
                qi += len;
            } else {
                if (WRITE)
                    for (uint32_t x = lane; x < len; x += 64u)
                        ref[n_ref + x] = (uint8_t)(kLetters >> (8u * bmdna::dna4_code(T[ti + x])));
                n_ref += len;
                ti += len;
            }
            continue;
        }
        // an M entry, 64 columns a step; the bytes of the next step are on their way while this one is worked on.
        // packed per lane: bit 0 ranks differ, bits 1-2 the text's rank
        auto fetch = [&](uint32_t c) -> uint32_t {
            if (c + lane >= len) return 0u;
            const uint32_t tr = bmdna::dna4_code(T[ti + c + lane]);
            const uint32_t qx = qi + c + lane;
            const uint32_t qr = rc ? bmdna::dna4_code(Q[m - 1u - qx]) ^ 3u : bmdna::dna4_code(Q[qx]);
            return (tr != qr ? 1u : 0u) | (tr << 1);
        };
        uint32_t cur = fetch(0u);
        for (uint32_t c = 0; c < len; c += 64u) {
            const uint32_t nxt = c + 64u < len ? fetch(c + 64u) : 0u;
            const uint32_t cnt = len - c < 64u ? len - c : 64u;
            const uint64_t valid = cnt == 64u ? ~0ull : (1ull << cnt) - 1ull;
            const uint64_t x = __ballot((cur & 1u) != 0u);      // (lanes beyond cnt hold 0)
            const uint64_t starts = ((x ^ (x << 1)) | 1ull) & valid;
            const uint32_t runs = (uint32_t)__popcll(starts);
            const uint32_t op0 = (x & 1ull) ? kOpX : kOpEq;
            uint32_t base = n_out, carry = 0;
            if (open) {
                if ((open & 15u) == op0) {
                    carry = open >> 4;                          // the first run continues the open one
                } else {
                    if (WRITE && lane == 0) out[base] = open;
                    base++;
                }
            }
            if (WRITE) {
                const uint32_t rank = (uint32_t)__popcll(starts & below);
                if (((starts >> lane) & 1ull) && rank + 1u < runs) {        // every run but the step's last is complete
                    const uint64_t next = starts & ~((2ull << lane) - 1ull);
                    const uint32_t run_len = (uint32_t)__builtin_ctzll(next) - lane + (rank == 0u ? carry : 0u);
                    out[base + rank] = (run_len << 4) | ((cur & 1u) ? kOpX : kOpEq);
                }
                if (cur & 1u) ref[n_ref + (uint32_t)__popcll(x & below)] = (uint8_t)(kLetters >> (8u * (cur >> 1)));
            }
            const uint32_t last = 63u - (uint32_t)__builtin_clzll(starts);
            open = ((cnt - last + (runs == 1u ? carry : 0u)) << 4) | (((x >> last) & 1ull) ? kOpX : kOpEq);
            n_out = base + runs - 1u;
            const uint32_t nx = (uint32_t)__popcll(x);
            n_ref += nx;
            nm += nx;
            cur = nxt;
        }
        ti += len;
        qi += len;
    }
    if (open) {
        if (WRITE && lane == 0) out[n_out] = open;
        n_out++;
    }
    if (!WRITE && lane == 0) {
        J.nm[a] = nm;
        J.n_xcigar[a] = n_out;
        J.n_ref[a] = n_ref;
    }
}

// instantiated in bmv_annotate.hip
extern template __global__ void bmv_annotate_kernel<false>(AnnotateJob);
extern template __global__ void bmv_annotate_kernel<true>(AnnotateJob);

}  // namespace bmv
