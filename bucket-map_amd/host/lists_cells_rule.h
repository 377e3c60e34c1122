// lists_cells_rule.h -- whether the lists vote counts cells of buckets first (csrc/bmf_kmer_lists.hip.h, "the cells
// form"), decided once per index load.  Plain C++, no HIP: build_kmer_lists (csrc/bmf_api.hip) and the stand-alone check
// (tests/cpp/lists_cells_check.cpp) read the same lines.
//
// The cells form pays where an item that cannot vote -- the wrong orientation of a read, a read that maps nowhere --
// leaves after the cell phase, that is where none of its cells reaches t = S - F + 1 by chance.  Model: the S lists of
// such an item are independent draws of density d = ids per list / NB, so the sum of a cell of C buckets is about
// Poisson(lambda), lambda = S C d, and the item keeps p = P(Poisson(lambda) >= t) * ceil(NB / C) cells on average.
// p <= 0.05 is a condition, not a tuned figure: at most one such item in twenty does both phases for nothing.
#pragma once

#include <stdint.h>

#include <cmath>

namespace bmf_rule {

constexpr double kCellsMaxKept = 0.05;

// P(Poisson(lambda) >= t), summed from the tail's own terms (1 - the head would cancel where the tail is tiny)
inline double poisson_tail(double lambda, uint32_t t) {
    if (t == 0) return 1.0;
    if (!(lambda > 0.0)) return 0.0;
    double term = std::exp(-lambda);             // the term of i = 0
    for (uint32_t i = 1; i <= t; i++) term *= lambda / (double)i;
    double sum = 0.0;
    for (uint32_t i = t; i < t + 4096u; i++) {
        sum += term;
        term *= lambda / (double)(i + 1u);
        if (term < sum * 1e-17 && (double)(i + 1u) > lambda) break;
    }
    return sum < 1.0 ? sum : 1.0;
}

// lambda and p of cells of 2^shift buckets; mean_units: 16-byte units (8 ids) of the list a sample meets, weighted by
// length as the load-time sample computes it.  The last unit of a list is filled up with 0 .. 7 padding ids, 3.5 on
// average, which are no buckets: a list of u units holds 8 u - 3.5 ids on average, and so does the weighted mean.
inline void cells_model(uint32_t nb, uint32_t S, uint32_t F, double mean_units, uint32_t shift, double *lambda, double *p) {
    const double ids = std::fmax(0.0, 8.0 * mean_units - 3.5);
    const double density = nb ? std::fmin(1.0, ids / (double)nb) : 1.0;
    const uint32_t C = 1u << shift;
    *lambda = (double)S * (double)C * density;
    *p = poisson_tail(*lambda, S - F + 1u) * (double)((nb + C - 1u) / C);
}

// Can the form serve at all?  A cell's sum is at most C S, which byte fields hold for S <= 31, and the scan's test
// needs 1 <= t (F <= S; with F > S every bucket qualifies with no hit at all, which the full-width kernel answers).
inline bool cells_possible(uint32_t S, uint32_t F) { return S >= 1u && S <= 31u && F <= S; }

// 0: the full-width kernel; 3: cells of 8 buckets; 2: cells of 4
inline int lists_cells(uint32_t nb, uint32_t S, uint32_t F, double mean_units, double *lambda_out = nullptr, double *p_out = nullptr) {
    if (lambda_out) *lambda_out = 0.0;
    if (p_out) *p_out = 0.0;
    if (!cells_possible(S, F)) return 0;
    for (uint32_t shift = 3; shift >= 2; shift--) {
        double lambda, p;
        cells_model(nb, S, F, mean_units, shift, &lambda, &p);
        if (lambda_out) *lambda_out = lambda;
        if (p_out) *p_out = p;
        if (p <= kCellsMaxKept) return (int)shift;
    }
    return 0;
}

// Waves per item of the cells kernel.  Its counters are small, so the LDS does not limit the residency and the rule of
// the full-width kernel (kmer_item_waves in csrc/bmf_api.hip) would always answer 1.  Several waves shorten the zeroing
// and the scan, which grow with the counter bytes, and two or four waves keep their heads in registers for the exact
// phase where one wave must load them again.  Measured on the MI355X (profiles/r20/README.md), vote kernel ms:
//    3.3 KB of counters (NB = 26 413, cells of 8)   two waves 5.45, one 5.61, four 5.88 (three runs each)
//    6.6 KB (NB = 26 413, cells of 4)               two waves 5.70 (three runs); one and four only in a build whose two
//                                                   and four waves loaded their heads again: 6.00 / 5.98 / 6.45
//    8.2 KB (NB = 65 304, cells of 8)               two waves 5.76; in that other build 6.11 / 5.58 / 6.40
//   16.3 KB (NB = 65 304, cells of 4)               in that other build 12.17 / 8.72 / 7.44
// So: two waves up to 12 KB of counters, four above.  The threshold lies between the two measured sizes on either side
// of it; nothing between them, below 3.3 KB or above 16.3 KB was measured, and one wave is never chosen (it can be
// forced).
inline int cells_item_waves(uint32_t nb, uint32_t shift) {
    const uint32_t counter_bytes = ((nb + (1u << shift) - 1u) >> shift);
    return counter_bytes <= 12u * 1024u ? 2 : 4;
}

}  // namespace bmf_rule
