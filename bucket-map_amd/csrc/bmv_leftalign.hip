// bmv_leftalign.hip -- the kernels of bmv_leftalign (bmv_leftalign.hip.h: the shape), in a translation unit of their own
// like bmv_realign.hip: the aligning kernels' device code is not recompiled beside them.
#include "bmv_leftalign.hip.h"

namespace bmv {

__device__ __forceinline__ uint32_t leftalign_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__global__ __launch_bounds__(64 * kLeftAlignWaves) void bmv_leftalign_kernel(LeftAlignJob J) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = leftalign_uniform(blockIdx.x * kLeftAlignWaves + (threadIdx.x >> 6));
    if (slot >= J.count) return;
    const uint32_t a = J.first + slot;
    const uint64_t cig_at = J.cigar_offset[a];
    const uint32_t ne = (uint32_t)(J.cigar_offset[a + 1] - cig_at);
    if (ne == 0u) {                                             // begin as given, no entries, zeros
        if (lane == 0) {
            J.out_begin[a] = J.begin[a];
            J.nops[a] = 0u;
            J.dropped[a] = 0u;
            J.merges[a] = 0u;
            J.compared[a] = 0ull;
            J.changed[a] = 0;
        }
        return;
    }
    const uint32_t *cig = J.cigar + cig_at;
    const bool rc = J.text_rc[a] != 0;
    const uint32_t m = J.query_len[a];
    // reference bases consumed (M and D lengths) and the gap entries: the forward pos, and the slot's size
    uint32_t ref_len = 0, cap = 0;
    for (uint32_t k = lane; k < ne; k += 64u) {
        const uint32_t e = cig[k];
        ref_len += (e & 15u) != 1u ? e >> 4 : 0u;
        cap += (e & 15u) != 0u ? 2u : 1u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ref_len += __shfl_xor(ref_len, o, 64);
        cap += __shfl_xor(cap, o, 64);
    }
    ref_len = leftalign_uniform(ref_len);
    cap = leftalign_uniform(cap);
    const uint8_t *W = J.genome + J.text_start[a];
    const uint8_t *Q = J.reads + J.query_start[a];
    uint32_t *st = J.stack + J.slot_at[a];

    uint32_t pos = rc ? J.text_len[a] - J.begin[a] - ref_len : J.begin[a];
    uint32_t p = pos, q = 0;                                    // the cursors, forward strand
    uint32_t top = 0, sp = 0;                                   // the stack: its top entry (0 = empty), the entries below it
    uint32_t dropped = 0, merges = 0, moved = 0;
    uint64_t compared = 0;
    // (every input entry pushes at most one entry, a gap one more for the M columns it passed: sp stays below cap)
    auto push = [&](uint32_t e) {
        if (top != 0u) {
            if (lane == 0 && sp < cap) st[sp] = top;
            sp++;
        }
        top = e;
    };
    auto pop = [&]() {
        uint32_t v = 0;
        if (sp != 0u) {
            sp--;
            if (lane == 0) v = st[sp];
        }
        top = leftalign_uniform(v);
    };
    auto append_m = [&](uint32_t len) {
        if (len == 0u) return;
        if (top != 0u && (top & 15u) == 0u)
            top += len << 4;
        else
            push(len << 4);
    };

    uint32_t chunk = 0;
    for (uint32_t k = 0; k < ne; k++) {
        if ((k & 63u) == 0u) {
            const uint32_t x = k + lane;
            chunk = x < ne ? cig[rc ? ne - 1u - x : x] : 0u;
        }
        const uint32_t e = (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)(k & 63u));
        const uint32_t op = e & 15u;
        uint32_t len = e >> 4;
        if (op == 0u) {
            append_m(len);
            p += len;
            q += len;
            continue;
        }
        const bool is_d = op == 2u;
        const uint32_t p_after = p + (is_d ? len : 0u), q_after = q + (is_d ? 0u : len);
        uint32_t pend = 0;
        bool keep = true;
        for (;;) {
            if (top == 0u) {                                    // (1) the start of the alignment
                if (is_d) {
                    pos += len;
                    dropped += len;
                    keep = false;
                }
                break;
            }
            const uint32_t top_op = top & 15u;
            if (top_op == 0u) {                                 // (2) an M run of run columns in front of the gap
                uint32_t run = top >> 4;
                bool stopped = false;
                while (run != 0u) {
                    const uint32_t c = run < 64u ? run : 64u;
                    bool same = false;
                    if (lane < c) {
                        if (is_d) {
                            const uint32_t x = p - 1u - lane;
                            same = bmdna::dna4_code(W[x]) == bmdna::dna4_code(W[x + len]);
                        } else {
                            const uint32_t x = q - 1u - lane;
                            same = rc ? bmdna::dna4_code(Q[m - 1u - x]) == bmdna::dna4_code(Q[m - 1u - x - len])
                                      : bmdna::dna4_code(Q[x]) == bmdna::dna4_code(Q[x + len]);
                        }
                    }
                    const uint64_t differ = ~__ballot(same);    // (lanes from c on differ)
                    const uint32_t s = differ == 0ull ? 64u : (uint32_t)__builtin_ctzll(differ);
                    compared += s + (s < c ? 1u : 0u);
                    p -= s;
                    q -= s;
                    pend += s;
                    run -= s;
                    if (s < c) {
                        stopped = true;
                        break;
                    }
                }
                if (stopped) {
                    top = run << 4;
                    break;
                }
                pop();
            } else if (top_op == op) {                          // (3) a gap of the same op: one gap, which moves on
                const uint32_t more = top >> 4;
                len += more;
                if (is_d) p -= more; else q -= more;
                merges++;
                pop();
            } else {                                            // (4) a gap of the other op
                break;
            }
        }
        if (keep) push((len << 4) | op);
        append_m(pend);
        moved |= pend;
        p = p_after;
        q = q_after;
    }
    if (top != 0u && (top & 15u) == 2u) {                       // the alignment does not end with D
        dropped += top >> 4;
        pop();
    }
    if (top != 0u) {
        if (lane == 0 && sp < cap) st[sp] = top;
        sp++;
    }
    if (lane == 0) {
        J.out_begin[a] = rc ? J.text_len[a] - pos - (ref_len - dropped) : pos;
        J.nops[a] = sp < cap ? sp : cap;
        J.dropped[a] = dropped;
        J.merges[a] = merges;
        J.compared[a] = compared;
        J.changed[a] = (moved | dropped) != 0u ? 1 : 0;
    }
}

// The entries of a piece at their packed offsets: a forward-strand alignment's stack as it stands, a reverse-strand one's from
// its top down -- the aligner's order.  Eight threads an alignment, as bmv_realign_gather_kernel.
__global__ void bmv_leftalign_gather_kernel(LeftAlignJob J) {
    const uint32_t slot = blockIdx.x * (blockDim.x / 8u) + threadIdx.x / 8u, t = threadIdx.x % 8u;
    if (slot >= J.count) return;
    const uint32_t a = J.first + slot;
    const uint32_t cnt = J.nops[a];
    const bool rc = J.text_rc[a] != 0;
    const uint32_t *src = J.stack + J.slot_at[a];
    uint32_t *dst = J.out_cigar + J.out_offset[slot];
    for (uint32_t x = t; x < cnt; x += 8u) dst[x] = src[rc ? cnt - 1u - x : x];
}

}  // namespace bmv
