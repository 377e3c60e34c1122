// overlap_clip.h -- bmv_overlap's contract (include/bmv.h) restated for the host, on top of sam_tags::annotate_on_host: the two
// mates of a pair soft-clipped at one cut so that no reference base lies under both.  Plain C++17, one alignment after the
// other: the reference the device is compared with (tests/cpp/overlap_check.cpp) and what the locator falls back to with a
// verifier that has no overlap pass of its own (the oracle-backed test tools); the product clips on the device.
//
// The rule, on an alignment's forward-strand columns 0 .. C-1 (its =/X/I/D entries):
//   base range [l, r)    all columns when match == penalty == 0, else bmv_clip's: the greatest sum of +match per = column and
//                        -penalty per X, I or D column, the smallest r, then the largest l
//   g(i)                 text_start + pos + the reference-consuming columns before i;  G0 = g(l), G1 = g(r)
//   a pair is cut when   both ranges are non-empty, the contigs agree, with `first` the mate of smaller (G0, index):
//                        G1(first) <= G1(second) and o = G1(first) - G0(second) > 0, and both columns below exist
//   m                    G0(second) + o / 2
//   first keeps [l, r')  r' - 1 the last = or X column of [l, r) with g < m
//   second keeps [l', r) l' the first = or X column of [l, r) with g >= m
// Since every M column of the aligner's CIGAR is an = or an X column, r' and l' follow from entry lengths alone.
#pragma once

#include "sam_tags.h"

#include <stdexcept>
#include <string>

namespace bm {

namespace overlap {

constexpr uint32_t kNoMate = 0xFFFFFFFFu;

struct span {
    uint64_t l = 0, r = 0;          // the range, in columns
    int64_t g0 = 0, g1 = 0;         // g(l), g(r)
};

// the reference- and query-consuming columns of entries[0, n) before column x
inline void columns_before(const uint32_t *entry, size_t n, uint64_t x, uint64_t &ref, uint64_t &qry) {
    uint64_t col = 0;
    ref = qry = 0;
    for (size_t k = 0; k < n && col < x; k++) {
        const uint32_t op = entry[k] & 15u;
        const uint64_t len = entry[k] >> 4, take = x - col < len ? x - col : len;
        if (op != 1u) ref += take;
        if (op != 2u) qry += take;
        col += len;
    }
}

// bmv_clip's range over =/X/I/D entries: one pass, the least prefix sum so far at its latest index, the best replaced only by
// a greater score
inline void best_range(const uint32_t *entry, size_t n, int64_t match, int64_t penalty, uint64_t &l, uint64_t &r) {
    int64_t p = 0, low = 0, best = 0;
    uint64_t col = 0, low_at = 0;
    l = r = 0;
    for (size_t k = 0; k < n; k++) {
        const uint32_t op = entry[k] & 15u, len = entry[k] >> 4;
        for (uint32_t x = 0; x < len; x++) {
            p += op == 7u ? match : -penalty;
            col++;
            if (p <= low) {
                low = p;
                low_at = col;
            }
            if (p - low > best) {
                best = p - low;
                l = low_at;
                r = col;
            }
        }
    }
}

// r' of a first (0: there is none) or l' of a second (UINT64_MAX: none) for the cut at `want` reference bases behind column 0
inline uint64_t edge(const uint32_t *entry, size_t n, const span &s, int64_t want, bool first) {
    int64_t col = 0, ref = 0;
    uint64_t found = first ? 0u : UINT64_MAX;
    const int64_t l = static_cast<int64_t>(s.l), r = static_cast<int64_t>(s.r);
    for (size_t k = 0; k < n && col < r; k++) {
        const uint32_t op = entry[k] & 15u;
        const int64_t len = entry[k] >> 4;
        if (op == 7u || op == 8u) {
            // column i of this entry has g - g(0) = ref + i - col:  g < m  <=>  i < col + want - ref
            const int64_t lo = col > l ? col : l, hi = col + len < r ? col + len : r, lim = col + want - ref;
            if (lo < hi) {
                if (first) {
                    const int64_t end = hi < lim ? hi : lim;
                    if (end > lo) found = static_cast<uint64_t>(end);
                } else if (found == UINT64_MAX) {
                    const int64_t at = lo > lim ? lo : lim;
                    if (at < hi) found = static_cast<uint64_t>(at);
                }
            }
        }
        col += len;
        if (op != 1u) ref += len;
    }
    return found;
}

}  // namespace overlap

// `genome`: the records back to back, as the verifier's own copy lies.  mate[a]: the batch index of a's mate or kNoMate;
// contig: per alignment, or null for one contig.  out: bmv_overlapped's arrays; cut[a]: the query bases the cut added to a's
// soft clips; pairs_cut and bases_cut: the pairs cut and the sum of cut.  Throws std::invalid_argument on what bmv_overlap
// refuses about mate and the scores.
inline void clip_overlap_on_host(const uint8_t *genome, const uint8_t *reads, const uint64_t *text_start, const uint32_t *text_len,
                                 const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                                 const uint64_t *cigar_offset, const uint32_t *cigar, const uint32_t *mate, const uint32_t *contig,
                                 uint32_t n, uint32_t match, uint32_t penalty, clipping &out, std::vector<uint32_t> &cut,
                                 uint64_t &pairs_cut, uint64_t &bases_cut) {
    using namespace overlap;
    const bool scored = match != 0u || penalty != 0u;
    if (scored && (match < 1u || match > 1024u || penalty < 1u || penalty > 1024u))
        throw std::invalid_argument("clip_overlap: match and penalty must be 0 and 0 or in 1..1024");
    for (uint32_t a = 0; a < n; a++) {
        if (mate[a] == kNoMate) continue;
        if (mate[a] >= n || mate[a] == a || mate[mate[a]] != a)
            throw std::invalid_argument("clip_overlap: alignment " + std::to_string(a) + " and its mate do not name each other");
    }
    annotation ann;
    sam_tags::annotate_on_host(genome, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar, n, ann);
    auto entries = [&](uint32_t a) { return ann.xcigar.data() + ann.xcigar_offset[a]; };
    auto n_entries = [&](uint32_t a) { return static_cast<size_t>(ann.xcigar_offset[a + 1] - ann.xcigar_offset[a]); };

    std::vector<span> base(n), kept;
    for (uint32_t a = 0; a < n; a++) {
        span &s = base[a];
        if (scored) {
            best_range(entries(a), n_entries(a), match, penalty, s.l, s.r);
        } else {
            for (size_t k = 0; k < n_entries(a); k++) s.r += entries(a)[k] >> 4;
        }
        uint64_t ref = 0, qry = 0;
        const int64_t g = static_cast<int64_t>(text_start[a]) + ann.pos[a];
        columns_before(entries(a), n_entries(a), s.l, ref, qry);
        s.g0 = g + static_cast<int64_t>(ref);
        columns_before(entries(a), n_entries(a), s.r, ref, qry);
        s.g1 = g + static_cast<int64_t>(ref);
    }
    kept = base;
    cut.assign(n, 0);
    pairs_cut = bases_cut = 0;
    for (uint32_t a = 0; a < n; a++) {
        const uint32_t b = mate[a];
        if (b == kNoMate || b < a) continue;
        if (base[a].l == base[a].r || base[b].l == base[b].r || (contig && contig[a] != contig[b])) continue;
        const bool a_first = base[a].g0 <= base[b].g0;            // (a < b: the index decides between equals)
        const uint32_t f = a_first ? a : b, s = a_first ? b : a;
        const int64_t o = base[f].g1 - base[s].g0;
        if (base[f].g1 > base[s].g1 || o <= 0) continue;
        const int64_t m = base[s].g0 + o / 2;
        const uint64_t r2 = edge(entries(f), n_entries(f), base[f], m - (static_cast<int64_t>(text_start[f]) + ann.pos[f]), true);
        const uint64_t l2 = edge(entries(s), n_entries(s), base[s], m - (static_cast<int64_t>(text_start[s]) + ann.pos[s]), false);
        if (r2 == 0u || l2 == UINT64_MAX) continue;
        uint64_t ref = 0, q_at = 0, q_end = 0;
        columns_before(entries(f), n_entries(f), r2, ref, q_at);
        columns_before(entries(f), n_entries(f), base[f].r, ref, q_end);
        cut[f] = static_cast<uint32_t>(q_end - q_at);
        columns_before(entries(s), n_entries(s), base[s].l, ref, q_at);
        columns_before(entries(s), n_entries(s), l2, ref, q_end);
        cut[s] = static_cast<uint32_t>(q_end - q_at);
        kept[f].r = r2;
        kept[s].l = l2;
        pairs_cut++;
        bases_cut += cut[f] + cut[s];
    }

    out.score.assign(n, 0);
    out.clip_left.assign(n, 0);
    out.clip_right.assign(n, 0);
    out.nm.assign(n, 0);
    out.pos.assign(n, 0);
    out.ref_len.assign(n, 0);
    out.xcigar.clear();
    out.ref_bases.clear();
    out.xcigar_offset.assign(static_cast<size_t>(n) + 1, 0);
    out.ref_offset.assign(static_cast<size_t>(n) + 1, 0);
    for (uint32_t a = 0; a < n; a++) {
        const uint64_t l = kept[a].l, r = kept[a].r;
        const size_t ne = n_entries(a);
        if (ne != 0 && l == r) {                                  // nothing kept: the whole query as one S entry
            out.clip_right[a] = query_len[a];
            if (query_len[a]) out.xcigar.push_back(query_len[a] << 4 | 4u);
        } else if (ne != 0) {
            uint64_t ref = 0, qry = 0, q_end = 0;
            columns_before(entries(a), ne, l, ref, qry);
            out.clip_left[a] = static_cast<uint32_t>(qry);
            out.pos[a] = ann.pos[a] + static_cast<uint32_t>(ref);
            columns_before(entries(a), ne, r, ref, q_end);
            out.clip_right[a] = query_len[a] - static_cast<uint32_t>(q_end);
            if (out.clip_left[a]) out.xcigar.push_back(out.clip_left[a] << 4 | 4u);
            const uint8_t *rb = ann.ref_bases.data() + ann.ref_offset[a];     // a letter per X and D column, in order
            uint64_t col = 0;
            for (size_t k = 0; k < ne && col < r; k++) {
                const uint32_t op = entries(a)[k] & 15u;
                const uint64_t len = entries(a)[k] >> 4, from = col < l ? (l - col < len ? l - col : len) : 0u,
                               to = r - col < len ? r - col : len;
                if (from < to) {
                    const uint32_t take = static_cast<uint32_t>(to - from);
                    out.xcigar.push_back(take << 4 | op);
                    if (op == 7u) out.score[a] += static_cast<int64_t>(match) * take;
                    else out.score[a] -= static_cast<int64_t>(penalty) * take, out.nm[a] += take;
                    if (op != 1u) out.ref_len[a] += take;
                    if (op == 8u || op == 2u) out.ref_bases.insert(out.ref_bases.end(), rb + from, rb + to);
                }
                if (op == 8u || op == 2u) rb += len;
                col += len;
            }
            if (out.clip_right[a]) out.xcigar.push_back(out.clip_right[a] << 4 | 4u);
        }
        out.xcigar_offset[a + 1] = out.xcigar.size();
        out.ref_offset[a + 1] = out.ref_bases.size();
    }
}

}  // namespace bm
