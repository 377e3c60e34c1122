// bmv_realign.hip -- the kernels of bmv_realign (bmv_realign.hip.h: the shape), in a translation unit of their own like
// bmv_pair.hip: the aligning kernels' device code is not recompiled beside them.
#include "bmv_realign.hip.h"

namespace bmv {

__device__ __forceinline__ int32_t realign_canon(int32_t v) { return v < kFloor ? kAbsent : v; }

// Cross-lane moves on the VALU (DPP), not through the LDS pipe, which a wave per row step would otherwise saturate.
// The value of the lane to the left; lane 0 receives `first`.
__device__ __forceinline__ int32_t realign_from_left(int32_t v, int32_t first) {
    return __builtin_amdgcn_update_dpp(first, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}
// One step of a prefix maximum: lanes the move does not reach keep their value.
template <int CTRL, int ROWS>
__device__ __forceinline__ int32_t realign_max_step(int32_t v) {
    const int32_t t = __builtin_amdgcn_update_dpp(INT32_MIN, v, CTRL, ROWS, 0xf, false);
    return t > v ? t : v;
}
// Inclusive prefix maximum over the wave: within rows of 16 lanes by row_shr 1, 2, 4, 8, then lane 15 of rows 0 and 2 into
// rows 1 and 3 (row_bcast:15), then lane 31 into rows 2 and 3 (row_bcast:31).
__device__ __forceinline__ int32_t realign_prefix_max(int32_t v) {
    v = realign_max_step<0x111, 0xf>(v);
    v = realign_max_step<0x112, 0xf>(v);
    v = realign_max_step<0x114, 0xf>(v);
    v = realign_max_step<0x118, 0xf>(v);
    v = realign_max_step<0x142, 0xa>(v);
    v = realign_max_step<0x143, 0xc>(v);
    return v;
}

__global__ __launch_bounds__(64) void bmv_realign_forward_kernel(RealignJob J) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t a = J.first + blockIdx.x;
    const uint64_t cig_at = J.cigar_offset[a];
    const uint32_t ne = (uint32_t)(J.cigar_offset[a + 1] - cig_at);
    const uint32_t *cig = J.cigar + cig_at;
    const bool rc = J.text_rc[a] != 0;
    const int m = (int)J.query_len[a], n = (int)J.text_len[a];
    const uint8_t *G = J.genome + J.text_start[a];
    const uint8_t *Q = J.reads + J.query_start[a];
    // the rank of T[x0 + lane], T the text as the aligner saw it; 0 outside it
    auto fetch_text = [&](int x0) -> uint32_t {
        const int x = x0 + lane;
        if (x < 0 || x >= n) return 0u;
        return rc ? bmdna::dna4_code(G[n - 1 - x]) ^ 3u : bmdna::dna4_code(G[x]);
    };
    auto fetch_query = [&](int x0) -> uint32_t {
        const int x = x0 + lane;
        return x < m ? bmdna::dna4_code(Q[x]) : 0u;
    };

    if (J.pass[a]) {                                            // the given path's affine score; begin and entries as given
        int32_t score = 0;
        int ti = (int)J.begin[a], qi = 0;
        for (uint32_t k = 0; k < ne; k++) {
            const uint32_t e = cig[k], op = e & 15u;
            const int len = (int)(e >> 4);
            if (op != 0u) {
                score -= J.open + len * J.ext;
                if (op == 1u) qi += len; else ti += len;
                continue;
            }
            for (int c = 0; c < len; c += 64) {
                const bool in = c + lane < len;
                const bool differ = in && fetch_text(ti + c) != fetch_query(qi + c);
                const int cnt = len - c < 64 ? len - c : 64;
                const int nx = (int)__popcll(__ballot(differ));
                score += (cnt - nx) * J.match - nx * J.mismatch;
            }
            ti += len;
            qi += len;
        }
        if (lane == 0) {
            J.score[a] = score;
            J.out_begin[a] = J.begin[a];
            J.nops[a] = ne;
        }
        return;
    }

    const int w = (int)J.band;
    uint8_t *codes = J.codes + J.row_at[a] * 64u;
    int base = (int)J.begin[a] - w;                             // column of lane 0
    uint32_t k = 0, op = 0;
    int rem = 0, run = 0;                                       // run: the D run that follows the row before
    if ((cig[0] & 15u) == 2u) {
        run = (int)(cig[0] >> 4);
        k = 1;
    }
    int32_t H, Ins = kAbsent;
    {
        const int j = base + lane;
        H = j >= 0 && j <= n && lane <= run + 2 * w ? 0 : kAbsent;
    }
    int tb = base - 1;                                          // the text column in lane 0 of tcur
    uint32_t tcur = fetch_text(tb), tnext = fetch_text(tb + 64), tahead = fetch_text(tb + 128);
    uint32_t qcur = fetch_query(0), qnext = fetch_query(64);
    for (int i = 1; i <= m; i++) {
        if (rem == 0) {
            const uint32_t e = cig[k++];
            op = e & 15u;
            rem = (int)(e >> 4);
        }
        rem--;
        const int shift = run + (op == 0u ? 1 : 0);
        run = 0;
        if (rem == 0 && k < ne && (cig[k] & 15u) == 2u) {
            run = (int)(cig[k] >> 4);
            k++;
        }
        base += shift;
        // s(i, j): the text base of column j - 1 against query base i - 1
        int o0 = base - 1 - tb;
        if (o0 >= 64) {
            tcur = tnext;
            tnext = tahead;
            tb += 64;
            tahead = fetch_text(tb + 128);
            o0 -= 64;
        }
        const int o = o0 + lane;
        const uint32_t both = (uint32_t)__shfl((int)(tcur | (tnext << 8)), o & 63, 64);
        const uint32_t tr = o < 64 ? both & 0xFFu : both >> 8;
        const int qi = i - 1;
        if (qi != 0 && (qi & 63) == 0) {
            qcur = qnext;
            qnext = fetch_query(qi + 64);
        }
        const uint32_t qr = (uint32_t)__builtin_amdgcn_readlane((int)qcur, qi & 63);
        const int32_t s = tr == qr ? J.match : -J.mismatch;
        // the row before, at this lane's column and at the one to its left
        const int up = lane + shift, dg = up - 1;
        const int32_t h_up_raw = __shfl(H, up & 63, 64), ins_up_raw = __shfl(Ins, up & 63, 64);
        // (the diagonal one is the upper one of the lane to the left; lane 0's is lane shift - 1 of the row before)
        const int32_t h_dg_raw = realign_from_left(h_up_raw, shift >= 1 ? __builtin_amdgcn_readlane(H, shift - 1) : kAbsent);
        const int32_t h_up = up <= 63 ? h_up_raw : kAbsent, ins_up = up <= 63 ? ins_up_raw : kAbsent;
        const int32_t h_dg = dg >= 0 && dg <= 63 ? h_dg_raw : kAbsent;
        const int j = base + lane;
        const bool valid = j >= 0 && j <= n && lane <= run + 2 * w;
        const int32_t diag = h_dg + s;
        const int32_t ins_open = h_up - J.open - J.ext, ins_ext = ins_up - J.ext;
        const bool ins_extends = ins_ext > ins_open;            // a tie opens: the shorter gap
        const int32_t ins = valid ? realign_canon(ins_extends ? ins_ext : ins_open) : kAbsent;
        const bool from_ins = ins > diag;                       // a tie takes the diagonal
        const int32_t h1 = valid ? realign_canon(from_ins ? ins : diag) : kAbsent;
        // Del by a prefix maximum over the lanes to the left
        const int32_t x = realign_prefix_max(h1 + lane * J.ext);    // (an absent one stays below kFloor)
        const int32_t before = realign_from_left(x, kAbsent);
        const int32_t del = valid ? realign_canon(realign_canon(before) - J.open - lane * J.ext) : kAbsent;
        const bool from_del = del > h1;
        const int32_t h = from_del ? del : h1;
        const int32_t h_left = realign_from_left(h, kAbsent), del_left = realign_from_left(del, kAbsent);
        const bool del_extends = del_left - J.ext > h_left - J.open - J.ext;
        uint32_t code = (from_del ? 2u : from_ins ? 1u : 0u) | (ins_extends ? 4u : 0u) | (del_extends ? 8u : 0u);
        if (lane == 0) code |= ((uint32_t)shift & 15u) << 4;
        if (lane == 1) code |= ((uint32_t)shift >> 4) << 4;
        codes[(uint64_t)(i - 1) * 64u + (uint32_t)lane] = (uint8_t)code;
        H = h;
        Ins = ins;
    }
    // the maximum of row m, at the last column that attains it
    int32_t best = H;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int32_t y = __shfl_xor(best, d, 64);
        best = y > best ? y : best;
    }
    const uint64_t at = __ballot(H == best);
    if (lane == 0) {
        J.score[a] = best;
        J.end_lane[a] = 63u - (uint32_t)__builtin_clzll(at);
    }
}

// The traceback of the realigned alignments of a piece: reversed run-length entries, their count, the begin column.
__global__ __launch_bounds__(64) void bmv_realign_trace_kernel(RealignJob J) {
    __shared__ uint4 rows[256];                                 // 64 rows of 64 codes
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = J.first + blockIdx.x;
    if (J.pass[a]) return;
    const uint32_t m = J.query_len[a];
    const uint8_t *codes = J.codes + J.row_at[a] * 64u;
    uint32_t *out = J.ops_rev + J.ops_at[a];
    const uint8_t *row_bytes = reinterpret_cast<const uint8_t *>(rows);
    uint32_t i = m, c = J.end_lane[a], state = 0;               // 0 H, 1 Ins, 2 Del
    uint32_t lo = m + 1u;                                       // rows lo .. lo + 63 are in LDS; none yet
    uint32_t open_op = 0, open_len = 0, n_out = 0;
    auto emit = [&](uint32_t op) {
        if (open_len != 0u && op == open_op) {
            open_len++;
            return;
        }
        if (open_len != 0u) {
            if (lane == 0) out[n_out] = (open_len << 4) | open_op;
            n_out++;
        }
        open_op = op;
        open_len = 1;
    };
    while (i != 0u) {                                           // (row 0 is reached in state H: Ins and Del are absent there)
        if (i < lo) {
            lo = ((i - 1u) & ~63u) + 1u;
            const uint32_t n_rows = m - lo + 1u < 64u ? m - lo + 1u : 64u;
            const uint4 *src = reinterpret_cast<const uint4 *>(codes + (uint64_t)(lo - 1u) * 64u);
            __syncthreads();
#pragma unroll
            for (uint32_t r = 0; r < 4u; r++) {
                const uint32_t idx = r * 64u + lane;
                if (idx < n_rows * 4u) rows[idx] = src[idx];
            }
            __syncthreads();
        }
        const uint8_t *row = row_bytes + (i - lo) * 64u;
        const uint32_t code = (uint32_t)__builtin_amdgcn_readfirstlane((int)row[c]);
        const uint32_t shift = (uint32_t)__builtin_amdgcn_readfirstlane((int)((row[0] >> 4) | ((row[1] >> 4) << 4)));
        if (state == 0u) {
            const uint32_t from = code & 3u;
            if (from == 0u) {
                emit(0u);
                c = c + shift - 1u;
                i--;
            } else {
                state = from;
            }
        } else if (state == 1u) {
            emit(1u);
            state = (code & 4u) ? 1u : 0u;
            c += shift;
            i--;
        } else {
            emit(2u);
            state = (code & 8u) ? 2u : 0u;
            c--;
        }
    }
    if (open_len != 0u) {
        if (lane == 0) out[n_out] = (open_len << 4) | open_op;
        n_out++;
    }
    if (lane == 0) {
        J.nops[a] = n_out;
        J.out_begin[a] = (uint32_t)((int)J.begin[a] - (int)J.band + (int)c);
    }
}

// The entries of a piece at their packed offsets: a realigned alignment's reversed into reading order, a passed-through one's
// copied as they came.  Eight threads an alignment, as bmv_gather_kernel.
__global__ void bmv_realign_gather_kernel(RealignJob J) {
    const uint32_t slot = blockIdx.x * (blockDim.x / 8u) + threadIdx.x / 8u, t = threadIdx.x % 8u;
    if (slot >= J.count) return;
    const uint32_t a = J.first + slot;
    const uint32_t cnt = J.nops[a];
    uint32_t *dst = J.out_cigar + J.out_offset[slot];
    if (J.pass[a]) {
        const uint32_t *src = J.cigar + J.cigar_offset[a];
        for (uint32_t x = t; x < cnt; x += 8u) dst[x] = src[x];
    } else {
        const uint32_t *src = J.ops_rev + J.ops_at[a];
        for (uint32_t x = t; x < cnt; x += 8u) dst[x] = src[cnt - 1u - x];
    }
}

}  // namespace bmv
