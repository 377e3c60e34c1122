// left_align.h -- bmv_leftalign's contract (include/bmv.h) restated for the host: every I and D entry of a known M/I/D path
// moved to its leftmost equivalent place on the forward strand, over a genome laid out as the verifier's.  A straight
// restatement of the rule: the walk, the stack, one column tested at a time.  alignment_verifier::left_align's default: a
// verifier without a pass of its own (the oracle-backed test tools) gets `bucketmap_align --left-align` through it; the
// product normalises on the device.
#pragma once

#include "bm_common.h"

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace bm {

// Normalised alignments of a batch, packed as bmv_leftaligned returns them (the shape of align's results, plus the flags),
// and what bmv_last_leftalign_stats counts.
struct left_alignment {
    std::vector<uint32_t> begin, cigar, dropped;
    std::vector<uint8_t> changed;
    std::vector<uint64_t> cigar_offset;
    uint64_t compared = 0, merges = 0;
};

namespace leftalign {

inline void left_align_on_host(const uint8_t *genome, const uint8_t *reads, const uint64_t *text_start, const uint32_t *text_len,
                               const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                               const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n_alignments, left_alignment &out) {
    out.begin.assign(begin, begin + n_alignments);
    out.dropped.assign(n_alignments, 0);
    out.changed.assign(n_alignments, 0);
    out.cigar.clear();
    out.cigar_offset.assign(static_cast<size_t>(n_alignments) + 1, 0);
    out.compared = out.merges = 0;
    std::vector<uint32_t> stack;
    for (uint32_t a = 0; a < n_alignments; a++) {
        const uint64_t c0 = cigar_offset[a], c1 = cigar_offset[a + 1];
        if (c0 == c1) {
            out.cigar_offset[a + 1] = out.cigar.size();
            continue;
        }
        uint64_t by_op[3] = {0, 0, 0};
        for (uint64_t x = c0; x < c1; x++) by_op[cigar[x] & 15u] += cigar[x] >> 4;
        for (const uint64_t sum : by_op)
            if (sum >= (1ull << 28))
                throw std::runtime_error("left_align: alignment " + std::to_string(a) + ": the lengths of one op sum to " +
                                         std::to_string(sum) + ", a merged entry would not fit 28 bits");
        const bool rc = text_rc[a] != 0;
        const int64_t m = query_len[a], r_len = static_cast<int64_t>(by_op[0] + by_op[2]);
        const uint8_t *w = genome + text_start[a], *qr = reads + query_start[a];
        // ranks of the window as it lies in the genome and of the query along the forward strand (both sides of every
        // comparison are complemented or neither is, so nothing is complemented)
        auto wf = [&](int64_t x) { return dna4_rank(w[x]); };
        auto qf = [&](int64_t x) { return dna4_rank(qr[rc ? m - 1 - x : x]); };
        int64_t pos = rc ? static_cast<int64_t>(text_len[a]) - begin[a] - r_len : begin[a];
        int64_t p = pos, q = 0;
        uint32_t dropped = 0;
        bool moved = false;
        stack.clear();
        auto append_m = [&](uint32_t len) {
            if (len == 0) return;
            if (!stack.empty() && (stack.back() & 15u) == 0u)
                stack.back() += len << 4;
            else
                stack.push_back(len << 4);
        };
        for (uint64_t k = 0; k < c1 - c0; k++) {
            const uint32_t e = cigar[rc ? c1 - 1 - k : c0 + k], op = e & 15u;
            uint32_t len = e >> 4;
            if (op == 0u) {
                append_m(len);
                p += len;
                q += len;
                continue;
            }
            const int64_t p_after = p + (op == 2u ? len : 0), q_after = q + (op == 1u ? len : 0);
            uint32_t pend = 0;
            bool push = true;
            for (;;) {
                if (stack.empty()) {                            // (1)
                    if (op == 2u) {
                        pos += len;
                        dropped += len;
                        push = false;
                    }
                    break;
                }
                const uint32_t top_op = stack.back() & 15u, top_len = stack.back() >> 4;
                if (top_op == 0u) {                             // (2)
                    uint32_t s = 0;
                    while (s < top_len) {
                        out.compared++;
                        const int64_t t = s + 1;
                        const bool same = op == 2u ? wf(p - t) == wf(p - t + len) : qf(q - t) == qf(q - t + len);
                        if (!same) break;
                        s++;
                    }
                    p -= s;
                    q -= s;
                    pend += s;
                    if (s < top_len) {
                        stack.back() = (top_len - s) << 4;
                        break;
                    }
                    stack.pop_back();
                } else if (top_op == op) {                      // (3)
                    stack.pop_back();
                    len += top_len;
                    (op == 2u ? p : q) -= top_len;
                    out.merges++;
                } else {                                        // (4)
                    break;
                }
            }
            if (push) stack.push_back(len << 4 | op);
            append_m(pend);
            moved = moved || pend != 0;
            p = p_after;
            q = q_after;
        }
        if (!stack.empty() && (stack.back() & 15u) == 2u) {
            dropped += stack.back() >> 4;
            stack.pop_back();
        }
        out.begin[a] = static_cast<uint32_t>(rc ? static_cast<int64_t>(text_len[a]) - pos - (r_len - dropped) : pos);
        out.dropped[a] = dropped;
        out.changed[a] = moved || dropped != 0;
        if (rc)
            out.cigar.insert(out.cigar.end(), stack.rbegin(), stack.rend());
        else
            out.cigar.insert(out.cigar.end(), stack.begin(), stack.end());
        out.cigar_offset[a + 1] = out.cigar.size();
    }
}

}  // namespace leftalign

}  // namespace bm
