// bmq_kernels.hip.h -- the mapping statistics of a BAM record stream on gfx950 (include/bmq.h states the rule).
//
// The state is 35 u64 tallies and eight u64 tables, row-major as the ABI hands them out.  The three large tables are indexed by
// READ CYCLE: a million records of one length hit the same few thousand cells, so the counters of the cycles below a window Cw
// live in LDS while a workgroup works and reach the u64 tables once, at its end.  Nothing depends on the order of the records.
//
//   records  one record per lane, grid-stride: the classes and the per-record tallies (one ballot and popcount per tally, kept
//            per wave across the loop, one 64-bit atomic per wave and non-zero tally at the end), MAPQ and RL (LDS u32, flushed
//            once) and IS (global: the sizes spread).
//   bases    one record per wave, the waves grid-stride.  BC, QC, the g and n of GC and the quality sums: the wave takes 256
//            bases a trip, lane l loads the l-th word of the qualities and (l < 32) of the packed sequence, and in step j of 4
//            every lane takes base 64 j + l out of the words by a shuffle, so the 64 adds of one instruction go to 64
//            consecutive cycles -- 64 different banks.  MC, ID and the op tallies: 64 ops a trip, query starts from
//            bmscan::wave_inclusive as bmp's walk_wave has them; an op of fewer than kWideSpan bases is counted by its lane, a
//            longer one by all lanes over its bases.  The walk is this file's own: it needs the query index of every base and
//            no reference position.
//   The LDS of `bases` is u32 [column][cycle] (75 columns: 5 of BC, 64 of QC, 6 of MC; consecutive lanes on consecutive banks),
//   then GC and ID.  A cell counts at most the ops of the records one workgroup takes in one launch: the host keeps that below
//   2^32 (kWaveRecords).  Cycles from Cw on go to the u64 tables directly; with Cw == 0 every cell does.
// No scratch; no kernel waits for another workgroup.
#pragma once

#include "bmp_walk.hip.h"

namespace bmq {

constexpr uint32_t kRecThreads = 256;                    // records
constexpr uint32_t kBaseThreads = 1024, kBaseWaves = kBaseThreads / 64;   // bases
constexpr uint32_t kTallies = 35, kColumns = 75, kBc = 0, kQc = 5, kMc = 69;   // BMQ_N_TALLIES; the columns of BC, QC, MC in LDS
constexpr uint32_t kGcRows = 101, kIdCells = 512, kMaxLdsCycles = 512;        // BMQ_MAX_LDS_CYCLES
constexpr uint32_t kWideSpan = 16;                       // bases of an op from which the wave shares them
// records a wave of `bases` takes in one launch at most: a workgroup's LDS cell then counts at most 16 x 2048 x 65 535 ops
constexpr uint32_t kWaveRecords = 2048;
constexpr uint32_t kRecFlags = 21;                       // the tallies that are one bit per record

struct state {
    unsigned long long *tally, *mapq, *rl, *is, *gc, *id, *bc, *qc, *mc;
    uint32_t C, I, Cw;                                   // Cw <= min(C, kMaxLdsCycles)
};

inline size_t lds_words(uint32_t Cw) { return Cw ? (size_t)kColumns * Cw + kGcRows + kIdCells : 0; }

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// which tally the k-th flag of `records` is
__device__ __forceinline__ constexpr uint32_t flag_tally(uint32_t k) { return k < 18 ? k : k == 18 ? 20u : k == 19 ? 21u : 33u; }

__global__ __launch_bounds__(kRecThreads) void records_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                              const uint8_t *__restrict__ skip, state st) {
    __shared__ uint32_t s_mapq[256], s_rl[kMaxLdsCycles];
    const uint32_t lane = threadIdx.x & 63u;
    if (st.Cw) {
        for (uint32_t k = threadIdx.x; k < 256; k += kRecThreads) s_mapq[k] = 0;
        for (uint32_t k = threadIdx.x; k < st.Cw; k += kRecThreads) s_rl[k] = 0;
        __syncthreads();
    }
    uint32_t count[kRecFlags];                           // per wave: the same in every lane
#pragma unroll
    for (uint32_t k = 0; k < kRecFlags; k++) count[k] = 0;
    unsigned long long bases = 0, bases_mapped = 0;      // per lane
    const uint64_t stride = (uint64_t)gridDim.x * kRecThreads;
    for (uint64_t first = (uint64_t)blockIdx.x * kRecThreads + (threadIdx.x - lane); first < n; first += stride) {   // the same trips in every lane of a wave
        const uint64_t i = first + lane;
        bool f[kRecFlags];
#pragma unroll
        for (uint32_t k = 0; k < kRecFlags; k++) f[k] = false;
        if (i < n && !(skip && skip[i])) {
            const uint8_t *r = in + rec_offset[i];
            const int32_t ref = (int32_t)bmp::load32(r + 4), next_ref = (int32_t)bmp::load32(r + 24), tlen = (int32_t)bmp::load32(r + 32);
            const uint32_t l_name = r[12], mapq = r[13], n_cigar = bmp::load16(r + 16), flag = bmp::load16(r + 18), l_seq = bmp::load32(r + 20);
            const uint8_t *cigar = r + 36 + l_name;
            const bool primary = !(flag & 0x900u), mapped = !(flag & 0x4u), paired = primary && (flag & 0x1u);
            const bool placeholder = n_cigar == 2 && bmp::load32(cigar) == (l_seq << 4 | 4u) && (bmp::load32(cigar + 4) & 15u) == 3u;
            const bool both = paired && mapped && !(flag & 0x8u), other_ref = both && next_ref != ref;
            const bool in_is = both && next_ref == ref && tlen > 0;
            f[0] = true, f[1] = primary, f[2] = flag & 0x100u, f[3] = flag & 0x800u, f[4] = flag & 0x400u, f[5] = flag & 0x200u;
            f[6] = mapped, f[7] = primary && mapped, f[8] = paired, f[9] = paired && (flag & 0x40u), f[10] = paired && (flag & 0x80u);
            f[11] = paired && (flag & 0x2u) && mapped, f[12] = both, f[13] = paired && mapped && (flag & 0x8u);
            f[14] = other_ref, f[15] = other_ref && mapq >= 5, f[16] = mapped && (flag & 0x10u), f[17] = mapped && mapq == 0;
            f[18] = mapped && n_cigar > 0 && l_seq > 0 && !placeholder, f[19] = mapped && placeholder, f[20] = in_is;
            if (primary) bases += l_seq;
            if (primary && mapped) bases_mapped += l_seq;
            if (mapped) {
                if (st.Cw) atomicAdd(&s_mapq[mapq], 1u);
                else atomicAdd(&st.mapq[mapq], 1ull);
            }
            if (primary) {
                const uint32_t row = l_seq < st.C ? l_seq : st.C;
                if (row < st.Cw) atomicAdd(&s_rl[row], 1u);
                else atomicAdd(&st.rl[row], 1ull);
            }
            if (in_is) {
                const uint32_t row = (uint32_t)tlen < st.I ? (uint32_t)tlen : st.I, way = flag & 0x30u;
                atomicAdd(&st.is[3ull * row + (way == 0x20u ? 0u : way == 0x10u ? 1u : 2u)], 1ull);   // no result used: no return
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kRecFlags; k++) count[k] += (uint32_t)__popcll((unsigned long long)__ballot(f[k]));
    }
    const unsigned long long all = wave_sum64(bases), all_mapped = wave_sum64(bases_mapped);
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kRecFlags; k++)
            if (count[k]) atomicAdd(&st.tally[flag_tally(k)], (unsigned long long)count[k]);
        if (all) atomicAdd(&st.tally[18], all);
        if (all_mapped) atomicAdd(&st.tally[19], all_mapped);
    }
    if (st.Cw) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < 256; k += kRecThreads)
            if (const uint32_t v = s_mapq[k]) atomicAdd(&st.mapq[k], (unsigned long long)v);
        for (uint32_t k = threadIdx.x; k < st.Cw; k += kRecThreads)
            if (const uint32_t v = s_rl[k]) atomicAdd(&st.rl[k], (unsigned long long)v);
    }
}

// one more in the cell of column `col` (of the 75) at cycle c < C
__device__ __forceinline__ void bump(uint32_t *lds, const state &st, uint32_t col, uint32_t c) {
    if (c < st.Cw) atomicAdd(&lds[col * st.Cw + c], 1u);
    else if (col < kQc) atomicAdd(&st.bc[5ull * c + col], 1ull);
    else if (col < kMc) atomicAdd(&st.qc[64ull * c + (col - kQc)], 1ull);
    else atomicAdd(&st.mc[6ull * c + (col - kMc)], 1ull);
}

__global__ __launch_bounds__(kBaseThreads) void bases_kernel(const uint8_t *__restrict__ in, const uint64_t *__restrict__ rec_offset, uint32_t n,
                                                             const uint8_t *__restrict__ skip, state st) {
    extern __shared__ uint32_t lds[];                    // lds_words(Cw): [75][Cw], GC, ID
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, Cw = st.Cw, n_lds = Cw ? kColumns * Cw + kGcRows + kIdCells : 0u;
    uint32_t *const s_gc = lds + kColumns * Cw, *const s_id = s_gc + kGcRows;
    for (uint32_t k = threadIdx.x; k < n_lds; k += kBaseThreads) lds[k] = 0;
    __syncthreads();
    unsigned long long a_m = 0, a_eq = 0, a_x = 0, a_ins = 0, a_del = 0, a_soft = 0, a_ni = 0, a_nd = 0, a_qsum = 0, a_qn = 0, a_beyond = 0;   // per lane
    uint32_t no_acgt = 0;                                // per wave
    const uint64_t stride = (uint64_t)gridDim.x * kBaseWaves;
    for (uint64_t i = (uint64_t)blockIdx.x * kBaseWaves + wave; i < n; i += stride) {   // everything about the record is the same in all lanes
        if (skip && skip[i]) continue;
        const uint8_t *r = in + rec_offset[i];
        const uint32_t l_name = r[12], n_cigar = bmp::load16(r + 16), flag = bmp::load16(r + 18), l_seq = bmp::load32(r + 20);
        const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar, *qual = seq + ((uint64_t)l_seq + 1) / 2;
        const bool primary = !(flag & 0x900u), reverse = flag & 0x10u;
        const bool placeholder = n_cigar == 2 && bmp::load32(cigar) == (l_seq << 4 | 4u) && (bmp::load32(cigar + 4) & 15u) == 3u;
        const bool aligned = !(flag & 0x4u) && n_cigar > 0 && l_seq > 0 && !placeholder;
        if (primary && l_seq > 0) {
            const uint32_t seq_bytes = (uint32_t)(((uint64_t)l_seq + 1) / 2);
            uint64_t n_letters = 0, n_gc = 0;
            for (uint64_t b0 = 0; b0 < l_seq; b0 += 256) {
                // a word may reach up to 3 bytes behind the last quality (the stream's buffer has 16 bytes of room behind its
                // end) or behind the sequence (the qualities lie there)
                const uint32_t qw = b0 + 4u * lane < l_seq ? bmp::load32(qual + b0 + 4u * lane) : 0u;
                const uint32_t sw = lane < 32 && b0 / 2 + 4u * lane < seq_bytes ? bmp::load32(seq + b0 / 2 + 4u * lane) : 0u;
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t xq = __shfl(qw, (int)(16u * j + (lane >> 2)), 64), xs = __shfl(sw, (int)(8u * j + (lane >> 3)), 64);
                    const uint64_t at = b0 + 64u * j + lane;             // b0 is even: the parity of `at` is the lane's
                    const bool live = at < l_seq;
                    const uint32_t q = (xq >> (8u * (lane & 3u))) & 255u, byte = (xs >> (8u * ((lane >> 1) & 3u))) & 255u;
                    const uint32_t code = (lane & 1u) ? byte & 15u : byte >> 4;
                    uint32_t letter = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
                    n_letters += (uint32_t)__popcll((unsigned long long)__ballot(live && letter < 4));
                    n_gc += (uint32_t)__popcll((unsigned long long)__ballot(live && (letter == 1 || letter == 2)));
                    if (!live) continue;
                    if (reverse && letter < 4) letter = 3 - letter;
                    const uint64_t c = reverse ? l_seq - 1 - at : at;
                    if (c < st.C) bump(lds, st, kBc + letter, (uint32_t)c);
                    else a_beyond++;
                    if (q != bmp::kQualNone) {
                        a_qsum += q, a_qn++;
                        if (c < st.C) bump(lds, st, kQc + (q < 63 ? q : 63u), (uint32_t)c);
                    }
                }
            }
            if (n_letters == 0) no_acgt++;
            else if (lane == 0) {
                const uint32_t row = (uint32_t)((200 * n_gc + n_letters) / (2 * n_letters));
                if (Cw) atomicAdd(&s_gc[row], 1u);
                else atomicAdd(&st.gc[row], 1ull);
            }
        }
        if (aligned) {
            uint32_t qc = 0;                             // the query bases of an aligned record are its l_seq (host check): below 2^32
            for (uint32_t c0 = 0; c0 < n_cigar; c0 += 64) {
                const uint32_t k = c0 + lane;
                uint32_t op = 15, len = 0;
                if (k < n_cigar) {
                    const uint32_t w = bmp::load32(cigar + 4ull * k);
                    op = w & 15u, len = w >> 4;
                }
                const uint32_t col = op == 7 ? 0u : op == 8 ? 1u : op == 0 ? 2u : op == 1 ? 3u : op == 4 ? 4u : 6u;   // 6: holds no base
                const uint32_t span = col < 6 ? len : 0u;
                const uint32_t q_incl = bmscan::wave_inclusive<uint32_t>(span, lane), q0 = qc + q_incl - span;
                if (op == 0) a_m += len;
                if (op == 7) a_eq += len;
                if (op == 8) a_x += len;
                if (op == 1) a_ins += len, a_ni += len > 0;
                if (op == 2) a_del += len, a_nd += len > 0;
                if (op == 4) a_soft += len;
                if ((op == 1 || op == 2) && len) {
                    const uint32_t cell = 2u * (len < 255 ? len : 255u) + (op == 2);
                    if (Cw) atomicAdd(&s_id[cell], 1u);
                    else atomicAdd(&st.id[cell], 1ull);
                    if (op == 2 && q0 > 0) {             // a deletion counts once, at the base before it
                        const uint32_t c = reverse ? l_seq - q0 : q0 - 1;
                        if (c < st.C) bump(lds, st, kMc + 5, c);
                    }
                }
                if (span && span < kWideSpan)
                    for (uint32_t p = 0; p < span; p++) {
                        const uint32_t at = q0 + p, c = reverse ? l_seq - 1 - at : at;   // at < l_seq (host check)
                        if (c < st.C) bump(lds, st, kMc + col, c);
                    }
                uint64_t wide = __ballot(span >= kWideSpan);
                while (wide) {                           // a long op by all lanes: consecutive cycles in one instruction
                    const int src = __ffsll((unsigned long long)wide) - 1;
                    wide &= wide - 1;
                    const uint32_t from = __shfl(q0, src, 64), count = __shfl(span, src, 64), w_col = __shfl(col, src, 64);
                    for (uint32_t p = lane; p < count; p += 64) {
                        const uint32_t at = from + p, c = reverse ? l_seq - 1 - at : at;
                        if (c < st.C) bump(lds, st, kMc + w_col, c);
                    }
                }
                qc += __shfl(q_incl, 63, 64);
            }
        }
    }
    const unsigned long long sums[11] = {wave_sum64(a_m),   wave_sum64(a_eq), wave_sum64(a_x),  wave_sum64(a_ins),  wave_sum64(a_del),   wave_sum64(a_soft),
                                         wave_sum64(a_ni),  wave_sum64(a_nd), wave_sum64(a_qsum), wave_sum64(a_qn), wave_sum64(a_beyond)};
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < 11; k++)
            if (sums[k]) atomicAdd(&st.tally[22 + k], sums[k]);   // tallies 22 .. 32 in this order
        if (no_acgt) atomicAdd(&st.tally[34], (unsigned long long)no_acgt);
    }
    if (Cw) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < kColumns * Cw; k += kBaseThreads) {   // consecutive lanes: consecutive cycles of one column
            const uint32_t v = lds[k];
            if (!v) continue;
            const uint32_t col = k / Cw, c = k - col * Cw;
            if (col < kQc) atomicAdd(&st.bc[5ull * c + col], (unsigned long long)v);
            else if (col < kMc) atomicAdd(&st.qc[64ull * c + (col - kQc)], (unsigned long long)v);
            else atomicAdd(&st.mc[6ull * c + (col - kMc)], (unsigned long long)v);
        }
        for (uint32_t k = threadIdx.x; k < kGcRows; k += kBaseThreads)
            if (const uint32_t v = s_gc[k]) atomicAdd(&st.gc[k], (unsigned long long)v);
        for (uint32_t k = threadIdx.x; k < kIdCells; k += kBaseThreads)
            if (const uint32_t v = s_id[k]) atomicAdd(&st.id[k], (unsigned long long)v);
    }
}

}  // namespace bmq
