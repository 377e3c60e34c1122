// best_mapq.h -- the MAPQ and the X0 tag of `bucketmap_align --best`, from what alignment_verifier::best (bmv_align_best,
// include/bmv.h) returns for one read's group of candidates.  A definition by choice, not by measurement; the
// Python restatement is bucket_map_amd.verify.best_mapq.
//
// The winner has e1 edits and the group's margin is M.  Of the other alignments of the group those with edits != kBeyond
// (within e1 + M) count, except the ones at the winner's own locus: the same strand and the same genome coordinate of the
// alignment's end -- text_start + end on the forward strand, text_start + text_len - end on the reverse.  Overlapping windows
// of neighbouring buckets find one alignment twice.  With e2 the smallest edits among the rest:
//   none               MAPQ 60
//   e2 == e1           MAPQ 0
//   otherwise          MAPQ (e2 - e1) * 60 / (M + 1), integer division
// X0 counts the distinct loci at e1 edits, the winner's own included.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace bm {

struct best_quality {
    unsigned int mapq, x0;
};

constexpr uint32_t kBestBeyond = UINT32_MAX;    // BMV_BEYOND

// The arrays are the group's own slices (size entries); winner is an index into them.
inline best_quality best_mapq(uint32_t winner, const uint32_t *edits, const uint32_t *end, const uint64_t *text_start,
                              const uint32_t *text_len, const uint8_t *text_rc, uint32_t size, uint32_t margin) {
    auto locus = [&](uint32_t a) {
        const bool rc = text_rc[a] != 0;
        return std::make_pair(rc, rc ? text_start[a] + text_len[a] - end[a] : text_start[a] + end[a]);
    };
    const uint32_t e1 = edits[winner];
    const auto home = locus(winner);
    uint32_t e2 = kBestBeyond;
    std::vector<std::pair<bool, uint64_t>> at_e1;               // distinct loci at e1 besides the winner's
    for (uint32_t a = 0; a < size; a++) {
        if (a == winner || edits[a] == kBestBeyond || locus(a) == home) continue;
        e2 = std::min(e2, edits[a]);
        if (edits[a] == e1 && std::find(at_e1.begin(), at_e1.end(), locus(a)) == at_e1.end()) at_e1.push_back(locus(a));
    }
    const unsigned int x0 = 1u + static_cast<unsigned int>(at_e1.size());
    if (e2 == kBestBeyond) return {60u, x0};
    if (e2 == e1) return {0u, x0};
    return {static_cast<unsigned int>(std::min<uint64_t>(60u, static_cast<uint64_t>(e2 - e1) * 60u / (static_cast<uint64_t>(margin) + 1u))), x0};
}

}  // namespace bm
