// split_pick.h -- the host side of `bucketmap_align --split`: bmv_split's pick (include/bmv.h) restated over arrays, the MAPQ
// of a chosen segment, and the SA:Z tag that ties a read's records together.  The product picks on the device
// (alignment_verifier::split, bmv_split); select_segments is the contract for users of the host layer and for the tests.  The
// Python restatements are bucket_map_amd.verify.select_segments, split_mapq and sa_entry.
//
// MAPQ, a definition by choice like best_mapq.h's, from a segment's clipping score s1 and the greatest clipping
// score s2 among the candidates that compete for the same half of the read and are no copy of the segment:
//   no competitor      MAPQ 60
//   s2 >= s1           MAPQ 0
//   otherwise          MAPQ (s1 - s2) * 60 / s1, integer division in 64 bits
#pragma once

#include <algorithm>
#include <charconv>
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

namespace bm {

constexpr int64_t kSplitNone = INT64_MIN;       // BMV_SPLIT_NONE
constexpr uint32_t kSplitBeyond = UINT32_MAX;   // BMV_BEYOND
constexpr uint32_t kSplitMaxSegments = 16;      // BMV_SPLIT_MAX_SEGMENTS

// What alignment_verifier::split returns for a batch: bmv_segments' arrays.
struct split_result {
    std::vector<int64_t> score, g_lo, g_hi, s2;     // s2: n_groups * max_segments
    std::vector<uint32_t> q_lo, q_hi, n_seg, seg;   // seg: n_groups * max_segments
};

struct split_params {
    uint32_t match = 1, penalty = 2;            // the clipping scores (--clip-scores)
    uint32_t min_score = 40, max_overlap_permille = 500, max_segments = 8;
};

namespace split_pick {

struct overlap {
    bool dup, conflict;
    uint64_t ovl_q;
};

// dup, conflict and ovl_q of alignments a and b (contig: null for one contig)
inline overlap compare(uint32_t a, uint32_t b, const uint32_t *q_lo, const uint32_t *q_hi, const int64_t *g_lo, const int64_t *g_hi,
                       const uint8_t *text_rc, const uint32_t *contig, uint32_t max_overlap_permille) {
    const uint32_t ql = std::max(q_lo[a], q_lo[b]), qh = std::min(q_hi[a], q_hi[b]);
    const int64_t gl = std::max(g_lo[a], g_lo[b]), gh = std::min(g_hi[a], g_hi[b]);
    const uint64_t ovl_q = qh > ql ? qh - ql : 0u;
    const bool same = (!contig || contig[a] == contig[b]) && (text_rc[a] != 0) == (text_rc[b] != 0);
    const bool dup = same && gh > gl && ovl_q > 0;
    const uint64_t shorter = std::min<uint64_t>(q_hi[a] - q_lo[a], q_hi[b] - q_lo[b]);
    return {dup, dup || ovl_q * 1000u > static_cast<uint64_t>(max_overlap_permille) * shorter, ovl_q};
}

}  // namespace split_pick

// bmv_split's pick over n alignments in n_groups groups: out.n_seg, out.seg and out.s2 as bmv_segments returns them (the five
// arrays per alignment are the caller's).
inline void select_segments(const int64_t *score, const uint32_t *q_lo, const uint32_t *q_hi, const int64_t *g_lo, const int64_t *g_hi,
                            const uint8_t *text_rc, const uint32_t *contig, const uint32_t *group_offset, uint32_t n_groups,
                            uint32_t min_score, uint32_t max_overlap_permille, uint32_t max_segments, split_result &out) {
    const size_t slots = static_cast<size_t>(n_groups) * max_segments;
    out.n_seg.assign(n_groups, 0);
    out.seg.assign(slots, kSplitBeyond);
    out.s2.assign(slots, kSplitNone);
    auto cmp = [&](uint32_t a, uint32_t b) { return split_pick::compare(a, b, q_lo, q_hi, g_lo, g_hi, text_rc, contig, max_overlap_permille); };
    for (uint32_t g = 0; g < n_groups; g++) {
        uint32_t *chosen = out.seg.data() + static_cast<size_t>(g) * max_segments;
        int64_t *s2 = out.s2.data() + static_cast<size_t>(g) * max_segments;
        uint32_t nc = 0;
        auto is_chosen = [&](uint32_t a) { return std::find(chosen, chosen + nc, a) != chosen + nc; };
        while (nc < max_segments) {
            uint32_t top = kSplitBeyond;
            for (uint32_t a = group_offset[g]; a < group_offset[g + 1]; a++) {
                if (score[a] < static_cast<int64_t>(min_score) || is_chosen(a)) continue;
                bool free = true;
                for (uint32_t k = 0; k < nc && free; k++) free = !cmp(a, chosen[k]).conflict;
                if (free && (top == kSplitBeyond || score[a] > score[top])) top = a;
            }
            if (top == kSplitBeyond) break;
            chosen[nc++] = top;
        }
        out.n_seg[g] = nc;
        for (uint32_t k = 0; k < nc; k++) {
            const uint32_t c = chosen[k];
            for (uint32_t a = group_offset[g]; a < group_offset[g + 1]; a++) {
                if (score[a] <= 0 || is_chosen(a)) continue;
                const split_pick::overlap o = cmp(a, c);
                if (!o.dup && 2u * o.ovl_q >= static_cast<uint64_t>(q_hi[c] - q_lo[c])) s2[k] = std::max(s2[k], score[a]);
            }
        }
    }
}

inline unsigned int split_mapq(int64_t s1, int64_t s2) {
    if (s2 == kSplitNone) return 60u;
    if (s2 >= s1 || s1 <= 0) return 0u;         // (a chosen segment has s1 >= min_score >= 1)
    return static_cast<unsigned int>(static_cast<uint64_t>(s1 - s2) * 60u / static_cast<uint64_t>(s1));
}

// One entry of SAM's SA:Z tag, "rname,pos,strand,CIGAR,mapQ,NM;": pos 1-based, the written entries (S = X I D) with their = and
// X runs merged into M.
inline void append_sa_entry(std::string &out, std::string_view rname, uint64_t pos0, bool reverse, const uint32_t *entry, size_t n,
                            unsigned int mapq, uint32_t nm) {
    auto number = [&](uint64_t v) {
        char tmp[24];
        const auto r = std::to_chars(tmp, tmp + sizeof tmp, v);
        out.append(tmp, static_cast<size_t>(r.ptr - tmp));
    };
    out.append(rname);
    out += ',';
    number(pos0 + 1u);
    out += ',';
    out += reverse ? '-' : '+';
    out += ',';
    uint64_t run = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t op = entry[i] & 15u, len = entry[i] >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            run += len;
            continue;
        }
        if (run) {
            number(run);
            out += 'M';
            run = 0;
        }
        number(len);
        out += "MIDNSHP=X"[op];
    }
    if (run) {
        number(run);
        out += 'M';
    }
    out += ',';
    number(mapq);
    out += ',';
    number(nm);
    out += ';';
}

}  // namespace bm
