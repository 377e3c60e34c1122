// frag_range.h -- `bucketmap_align --frag-auto`: the range a proper pair may span, learned from a block of pairs.  The spans
// and their histogram as bmv_frag_spans defines them (include/bmv.h), restated for the host (alignment_verifier::paired_auto's
// default computes them with frag_span), and the range from a histogram.  A definition by choice, not by measurement
// (DESIGN 4.4), like best_mapq.h and pair_mapq.h; the Python restatements are bucket_map_amd.verify.frag_spans,
// frag_histogram and frag_range.
//
// The span.  known, L, R, locus, own winner and proper are pair_mapq.h's.  A group is settled when it has an own winner and
// every known alignment of the group lies at the winner's locus.  span[p] = R(r) - L(f) of the two own winners when both groups
// are settled and the winners are proper under [1, cap]; else 0: the pair is uninformative.  hist[s], 0 <= s <= cap, counts
// the pairs with span == s.
//
// The range.  n = the sum of hist[s] over s >= 1.  Learned iff n >= max(1, min_pairs); else the fallback comes back
// unchanged.  With v the informative spans in ascending order, Qk = v[floor(k n / 4)] for k = 1, 2, 3; IQR = Q3 - Q1;
// slack = max(3 IQR, ceil(Q2 / 4)); min_frag = max(1, Q1 - slack) in signed arithmetic, max_frag = Q3 + slack.  The ceil(Q2 / 4)
// floor keeps a library of identical fragments -- simulated data -- from getting a one-value range.  Mean and standard
// deviation are for the log line only.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "pair_mapq.h"

namespace bm {

struct frag_range_result {
    uint32_t min_frag, max_frag;    // the learned range, or the fallback
    bool learned;
    uint64_t n_informative;
    uint32_t q1, q2, q3;            // 0 when not learned
    double mean, sd;                // of the informative spans; 0 when there is none
};

// hist: n_bins = cap + 1 entries
inline frag_range_result frag_range(const uint64_t *hist, size_t n_bins, uint64_t min_pairs, uint32_t fallback_min, uint32_t fallback_max) {
    frag_range_result out{fallback_min, fallback_max, false, 0, 0, 0, 0, 0.0, 0.0};
    long double sum = 0, sq = 0;
    for (size_t s = 1; s < n_bins; s++) {
        out.n_informative += hist[s];
        sum += static_cast<long double>(hist[s]) * s;
        sq += static_cast<long double>(hist[s]) * s * s;
    }
    const uint64_t n = out.n_informative;
    if (n) {
        out.mean = static_cast<double>(sum / n);
        out.sd = std::sqrt(static_cast<double>(std::max<long double>(0, sq / n - (sum / n) * (sum / n))));
    }
    if (n < std::max<uint64_t>(1, min_pairs)) return out;
    // v[i] is the span s with (the count below s) <= i < (the count up to s)
    const uint64_t at[3] = {n / 4u, n / 4u * 2u + n % 4u * 2u / 4u, n / 4u * 3u + n % 4u * 3u / 4u};       // floor(k n / 4) without overflow
    uint32_t q[3] = {0, 0, 0};
    uint64_t below = 0;
    unsigned int k = 0;
    for (size_t s = 1; s < n_bins && k < 3u; s++) {
        below += hist[s];
        while (k < 3u && at[k] < below) q[k++] = static_cast<uint32_t>(s);
    }
    out.q1 = q[0];
    out.q2 = q[1];
    out.q3 = q[2];
    const int64_t iqr = static_cast<int64_t>(q[2]) - q[0];
    const int64_t slack = std::max<int64_t>(3 * iqr, (static_cast<int64_t>(q[1]) + 3) / 4);
    out.min_frag = static_cast<uint32_t>(std::max<int64_t>(1, static_cast<int64_t>(q[0]) - slack));
    out.max_frag = static_cast<uint32_t>(static_cast<int64_t>(q[2]) + slack);
    out.learned = true;
    return out;
}

// span[p] of the pair whose first mate owns the alignments a0 .. a1 - 1 and whose second a1 .. a2 - 1; contig may be null
inline uint32_t frag_span(const uint64_t *text_start, const uint32_t *text_len, const uint8_t *text_rc, const uint32_t *query_len,
                          const uint32_t *edits, const uint32_t *end, const uint32_t *contig, uint32_t a0, uint32_t a1, uint32_t a2,
                          uint32_t cap) {
    auto known = [&](uint32_t a) { return edits[a] != kBestBeyond; };
    auto rc = [&](uint32_t a) { return text_rc[a] != 0; };
    auto left = [&](uint32_t a) {
        return rc(a) ? static_cast<int64_t>(text_start[a]) + text_len[a] - end[a] : static_cast<int64_t>(text_start[a]) + end[a] - query_len[a];
    };
    auto right = [&](uint32_t a) { return left(a) + query_len[a]; };
    auto locus = [&](uint32_t a) { return std::make_pair(rc(a), rc(a) ? left(a) : right(a)); };
    auto settled_winner = [&](uint32_t lo, uint32_t hi) {       // the own winner of a settled group, else kBestBeyond
        uint32_t w = kBestBeyond;
        for (uint32_t a = lo; a < hi; a++)
            if (known(a) && (w == kBestBeyond || edits[a] < edits[w])) w = a;
        for (uint32_t a = lo; a < hi && w != kBestBeyond; a++)
            if (known(a) && locus(a) != locus(w)) w = kBestBeyond;
        return w;
    };
    const uint32_t i = settled_winner(a0, a1), j = settled_winner(a1, a2);
    if (i == kBestBeyond || j == kBestBeyond || rc(i) == rc(j) || (contig && contig[i] != contig[j])) return 0u;
    const uint32_t f = rc(i) ? j : i, r = rc(i) ? i : j;
    const int64_t frag = right(r) - left(f);
    if (!(left(f) <= left(r) && right(f) <= right(r) && frag >= 1 && frag <= static_cast<int64_t>(cap))) return 0u;
    return static_cast<uint32_t>(frag);
}

}  // namespace bm
