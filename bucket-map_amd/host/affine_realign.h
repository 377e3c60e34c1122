// affine_realign.h -- bmv_realign's contract (include/bmv.h) restated for the host: the affine-gap alignment inside the band
// that follows a known edit path, as a straight three-matrix dynamic programme over the band's cells, over a genome laid out
// as the verifier's.  alignment_verifier::realign's default: a verifier without a realignment pass of its own (the
// oracle-backed test tools) gets `bucketmap_align --affine` through it; the product realigns on the device.
#pragma once

#include "bm_common.h"

#include <algorithm>
#include <cstdint>
#include <vector>

namespace bm {

// Realigned alignments of a batch, packed as bmv_realigned returns them (the shape of align's results, plus the flag).
struct realignment {
    std::vector<int32_t> score;
    std::vector<uint32_t> begin, cigar;
    std::vector<uint8_t> realigned;
    std::vector<uint64_t> cigar_offset;
};

struct affine_scores {
    uint32_t match = 1, mismatch = 4, gap_open = 6, gap_extend = 1, band = 16;
};

namespace affine {

constexpr int64_t kAbsent = INT64_MIN / 4;

inline int64_t minus(int64_t v, int64_t d) { return v == kAbsent ? kAbsent : v - d; }

inline void realign_on_host(const uint8_t *genome, const uint8_t *reads, const uint64_t *text_start, const uint32_t *text_len,
                            const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                            const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n_alignments, const affine_scores &sc,
                            realignment &out) {
    out.score.assign(n_alignments, 0);
    out.begin.assign(n_alignments, 0);
    out.realigned.assign(n_alignments, 0);
    out.cigar.clear();
    out.cigar_offset.assign(static_cast<size_t>(n_alignments) + 1, 0);
    const int64_t A = sc.match, B = sc.mismatch, O = sc.gap_open, E = sc.gap_extend, w = sc.band;
    for (uint32_t a = 0; a < n_alignments; a++) {
        const uint64_t c0 = cigar_offset[a], c1 = cigar_offset[a + 1];
        const int64_t m = query_len[a], n = text_len[a];
        const bool rc = text_rc[a] != 0;
        const uint8_t *g = genome + text_start[a], *q = reads + query_start[a];
        auto text = [&](int64_t x) -> uint8_t { return rc ? 3u - dna4_rank(g[n - 1 - x]) : dna4_rank(g[x]); };
        out.begin[a] = begin[a];
        // p(i), q(i) of the given path, and its affine score
        std::vector<int64_t> p(static_cast<size_t>(m) + 1, 0), qq(static_cast<size_t>(m) + 1, 0);
        int64_t i = 0, j = begin[a], given = 0, longest_d = 0;
        p[0] = qq[0] = j;
        for (uint64_t x = c0; x < c1; x++) {
            const uint32_t op = cigar[x] & 15u;
            const int64_t len = cigar[x] >> 4;
            if (op == 2u) {
                j += len;
                qq[i] = j;
                given -= O + len * E;
                longest_d = std::max(longest_d, len);
            } else {
                if (op == 1u) given -= O + len * E;
                for (int64_t s = 0; s < len; s++) {
                    if (op == 0u) {
                        given += text(j) == dna4_rank(q[i]) ? A : -B;
                        j++;
                    }
                    i++;
                    p[i] = qq[i] = j;
                }
            }
        }
        if (c0 == c1 || longest_d > 63 - 2 * w) {               // passed through
            out.score[a] = static_cast<int32_t>(c0 == c1 ? 0 : given);
            out.cigar.insert(out.cigar.end(), cigar + c0, cigar + c1);
            out.cigar_offset[a + 1] = out.cigar.size();
            continue;
        }
        out.realigned[a] = 1;
        // the three matrices, a row at a time; per cell the choices the traceback needs
        std::vector<int64_t> lo(static_cast<size_t>(m) + 1), hi(static_cast<size_t>(m) + 1);
        for (int64_t r = 0; r <= m; r++) {
            lo[r] = std::max<int64_t>(0, p[r] - w);
            hi[r] = std::min<int64_t>(n, qq[r] + w);
        }
        std::vector<std::vector<uint8_t>> code(static_cast<size_t>(m) + 1);   // bits 0-1: H from diagonal / Ins / Del; 2: Ins extends; 3: Del extends
        std::vector<int64_t> h_prev, ins_prev, h_cur, ins_cur, del_cur;
        h_prev.assign(static_cast<size_t>(hi[0] - lo[0] + 1), 0);
        ins_prev.assign(h_prev.size(), kAbsent);
        for (int64_t r = 1; r <= m; r++) {
            const size_t width = static_cast<size_t>(hi[r] - lo[r] + 1);
            h_cur.assign(width, kAbsent);
            ins_cur.assign(width, kAbsent);
            del_cur.assign(width, kAbsent);
            code[r].assign(width, 0);
            auto above = [&](const std::vector<int64_t> &row, int64_t col) {
                return col < lo[r - 1] || col > hi[r - 1] ? kAbsent : row[static_cast<size_t>(col - lo[r - 1])];
            };
            for (int64_t col = lo[r]; col <= hi[r]; col++) {
                const size_t at = static_cast<size_t>(col - lo[r]);
                uint8_t cd = 0;
                const int64_t ins_open = minus(above(h_prev, col), O + E), ins_ext = minus(above(ins_prev, col), E);
                ins_cur[at] = std::max(ins_open, ins_ext);
                if (ins_ext > ins_open) cd |= 4u;
                const int64_t del_open = at ? minus(h_cur[at - 1], O + E) : kAbsent, del_ext = at ? minus(del_cur[at - 1], E) : kAbsent;
                del_cur[at] = std::max(del_open, del_ext);
                if (del_ext > del_open) cd |= 8u;
                int64_t diag = col >= 1 ? above(h_prev, col - 1) : kAbsent;
                if (diag != kAbsent) diag += text(col - 1) == dna4_rank(q[r - 1]) ? A : -B;
                int64_t best = diag;
                if (ins_cur[at] > best) best = ins_cur[at], cd |= 1u;
                if (del_cur[at] > best) best = del_cur[at], cd = static_cast<uint8_t>((cd & ~3u) | 2u);
                h_cur[at] = best;
                code[r][at] = cd;
            }
            h_prev.swap(h_cur);
            ins_prev.swap(ins_cur);
        }
        int64_t best = kAbsent, col = lo[m];
        for (int64_t x = lo[m]; x <= hi[m]; x++) {
            const int64_t v = h_prev[static_cast<size_t>(x - lo[m])];
            if (v != kAbsent && v >= best) best = v, col = x;
        }
        out.score[a] = static_cast<int32_t>(best);
        std::vector<uint32_t> rev;                              // entries from the end
        auto emit = [&](uint32_t op) {
            if (!rev.empty() && (rev.back() & 15u) == op)
                rev.back() += 16u;
            else
                rev.push_back(16u | op);
        };
        int64_t r = m;
        int state = 0;
        while (r > 0) {
            const uint8_t cd = code[r][static_cast<size_t>(col - lo[r])];
            if (state == 0) {
                if ((cd & 3u) == 0u) {
                    emit(0u);
                    r--;
                    col--;
                } else {
                    state = cd & 3u;
                }
            } else if (state == 1) {
                emit(1u);
                state = (cd & 4u) ? 1 : 0;
                r--;
            } else {
                emit(2u);
                state = (cd & 8u) ? 2 : 0;
                col--;
            }
        }
        out.begin[a] = static_cast<uint32_t>(col);
        out.cigar.insert(out.cigar.end(), rev.rbegin(), rev.rend());
        out.cigar_offset[a + 1] = out.cigar.size();
    }
}

}  // namespace affine

}  // namespace bm
