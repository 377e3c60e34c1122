// pair_mapq.h -- `bucketmap_align --paired`: the pick over the candidates of two mates as bmv_pair defines it (include/bmv.h),
// restated for the host (alignment_verifier::paired's default selects with it), and the MAPQ and X0 of the two records.  A
// definition by choice, not by measurement, like best_mapq.h; the Python restatements are
// bucket_map_amd.verify.select_pairs and bucket_map_amd.verify.pair_mapq.
//
// The pick.  An alignment is known when its edits are not kBestBeyond.  Forward: R = text_start + end, L = R - query_len;
// reverse: L = text_start + text_len - end, R = L + query_len (signed 64-bit).  A combination of a known alignment of each
// mate is proper when both lie on one contig and on different strands and, with f the forward and r the reverse one,
// L(f) <= L(r), R(f) <= R(r) and min_frag <= R(r) - L(f) <= max_frag.  The pick minimises (edits[i] + edits[j], i, j); s1 is
// its sum and s2 the smallest sum over the proper combinations that differ from it in the locus (best_mapq.h's) of either
// mate.  Without a proper combination each mate keeps its own winner: the lowest known index with the smallest edits.
//
// MAPQ.  A pair that is not proper: each mate gets what best_mapq gives its own winner.  A proper pair, with M the sum of the
// two mates' margins:
//   q_pair     60 when there is no s2; 0 when s2 == s1; else min(60, (s2 - s1) * 60 / (M + 1))
//   q_single   best_mapq's value when the pick is the group's own winner, else 0
//   MAPQ       max(q_pair, q_single)
// X0 counts the distinct loci of the mate's own group at the pick's edits, its own included.
#pragma once

#include "best_mapq.h"

namespace bm {

constexpr uint64_t kPairNone = UINT64_MAX;      // BMV_PAIR_NONE

struct pair_pick {
    uint32_t pick[2], winner[2];    // batch indices, kBestBeyond when the group has no known alignment
    bool proper;
    uint64_t s1, s2;
};

// a0 .. a1 - 1 are the first mate's alignments, a1 .. a2 - 1 the second's; contig may be null (one contig)
inline pair_pick select_pair(const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc, const uint32_t *query_len,
                             const uint32_t *edits, const uint32_t *end, const uint32_t *contig, uint32_t a0, uint32_t a1, uint32_t a2,
                             int64_t min_frag, int64_t max_frag) {
    auto known = [&](uint32_t a) { return edits[a] != kBestBeyond; };
    auto rc = [&](uint32_t a) { return text_rc[a] != 0; };
    auto left = [&](uint32_t a) {
        return rc(a) ? static_cast<int64_t>(text_start[a]) + text_len[a] - end[a] : static_cast<int64_t>(text_start[a]) + end[a] - query_len[a];
    };
    auto right = [&](uint32_t a) { return left(a) + query_len[a]; };
    auto locus = [&](uint32_t a) { return std::make_pair(rc(a), rc(a) ? left(a) : right(a)); };
    auto own = [&](uint32_t lo, uint32_t hi) {
        uint32_t w = kBestBeyond;
        for (uint32_t a = lo; a < hi; a++)
            if (known(a) && (w == kBestBeyond || edits[a] < edits[w])) w = a;
        return w;
    };
    auto proper = [&](uint32_t i, uint32_t j) {
        if (!known(i) || !known(j) || rc(i) == rc(j) || (contig && contig[i] != contig[j])) return false;
        const uint32_t f = rc(i) ? j : i, r = rc(i) ? i : j;
        const int64_t frag = right(r) - left(f);
        return left(f) <= left(r) && right(f) <= right(r) && frag >= min_frag && frag <= max_frag;
    };
    pair_pick out{{own(a0, a1), own(a1, a2)}, {0, 0}, false, kPairNone, kPairNone};
    out.winner[0] = out.pick[0];
    out.winner[1] = out.pick[1];
    for (uint32_t i = a0; i < a1; i++)
        for (uint32_t j = a1; j < a2; j++) {
            if (!proper(i, j)) continue;
            const uint64_t s = static_cast<uint64_t>(edits[i]) + edits[j];
            if (out.proper && s >= out.s1) continue;            // (i, then j, ascending: the first of a sum stays)
            out.proper = true;
            out.s1 = s;
            out.pick[0] = i;
            out.pick[1] = j;
        }
    if (!out.proper) return out;
    const auto home_i = locus(out.pick[0]), home_j = locus(out.pick[1]);
    for (uint32_t i = a0; i < a1; i++)
        for (uint32_t j = a1; j < a2; j++)
            if (proper(i, j) && (locus(i) != home_i || locus(j) != home_j))
                out.s2 = std::min(out.s2, static_cast<uint64_t>(edits[i]) + edits[j]);
    return out;
}

inline unsigned int pair_quality(uint64_t s1, uint64_t s2, uint64_t margins) {
    if (s2 == kPairNone) return 60u;
    if (s2 == s1) return 0u;
    return static_cast<unsigned int>(std::min<uint64_t>(60u, (s2 - s1) * 60u / (margins + 1u)));
}

// One mate of a PROPER pair.  The arrays are the mate's own group's slices (size entries); pick and winner index into them;
// q_pair is pair_quality's value for the pair.
inline best_quality pair_mate_mapq(unsigned int q_pair, uint32_t pick, uint32_t winner, const uint32_t *edits, const uint32_t *end,
                                   const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc, uint32_t size,
                                   uint32_t margin) {
    auto locus = [&](uint32_t a) {
        const bool rc = text_rc[a] != 0;
        return std::make_pair(rc, rc ? text_start[a] + text_len[a] - end[a] : text_start[a] + end[a]);
    };
    const unsigned int q_single = pick == winner ? best_mapq(winner, edits, end, text_start, text_len, text_rc, size, margin).mapq : 0u;
    std::vector<std::pair<bool, uint64_t>> loci;                // distinct loci at the pick's edits
    for (uint32_t a = 0; a < size; a++)
        if (edits[a] == edits[pick] && std::find(loci.begin(), loci.end(), locus(a)) == loci.end()) loci.push_back(locus(a));
    return {std::max(q_pair, q_single), static_cast<unsigned int>(loci.size())};
}

}  // namespace bm
