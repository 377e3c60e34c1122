// sam_tags.h -- what `bucketmap_align --annotate` and `--clip` put into a record beyond the reference's fields, from the
// verifier's annotation of an alignment (include/bmv.h, bmv_annotate; with soft clips: bmv_clip): the =/X/I/D/S CIGAR
// string, the MD tag, and the reverse complement of a folded read.  Text formatting only; the walk over text and query that produces the annotation runs on
// the device.
#pragma once

#include "bm_common.h"

#include <charconv>
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

namespace bm {

// Annotations of a batch, packed as bmv_annotations returns them: alignment a owns xcigar[xcigar_offset[a] ..
// xcigar_offset[a + 1]) (len << 4 | op, BAM op codes: I 1, D 2, = 7, X 8) and ref_bases[ref_offset[a] .. ref_offset[a + 1]).
struct annotation {
    std::vector<uint32_t> nm, pos, ref_len, xcigar;
    std::vector<uint64_t> xcigar_offset, ref_offset;
    std::vector<uint8_t> ref_bases;
};

// The same of the kept part of every alignment as bmv_clipped returns it: S entries (op 4) may stand first and last.
struct clipping : annotation {
    std::vector<int64_t> score;
    std::vector<uint32_t> clip_left, clip_right;
};

namespace sam_tags {

inline void number(std::string &out, uint64_t v) {
    char tmp[24];
    const auto r = std::to_chars(tmp, tmp + sizeof tmp, v);
    out.append(tmp, static_cast<size_t>(r.ptr - tmp));
}

// "2S5=1X3I2D4S": BAM's op letters
inline void append_cigar(std::string &out, const uint32_t *entry, size_t n) {
    for (size_t i = 0; i < n; i++) {
        number(out, entry[i] >> 4);
        out += "MIDNSHP=X"[entry[i] & 15u];
    }
}

// MD as samtools writes it: a running count of matching bases; before every X base and before every D entry the count
// (also when it is 0), then the reference base -- or '^' and the deleted bases --, and the count starts again; I adds
// nothing, and neither does S (clipped bases are not aligned); the count once more at the end.  ref_bases: the reference base
// of every X and D column, in CIGAR order.
inline void append_md(std::string &out, const uint32_t *entry, size_t n, const uint8_t *ref_bases) {
    uint64_t run = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t op = entry[i] & 15u, len = entry[i] >> 4;
        if (op == 7u) {
            run += len;
        } else if (op == 8u) {
            for (uint32_t x = 0; x < len; x++) {
                number(out, run);
                out += static_cast<char>(*ref_bases++);
                run = 0;
            }
        } else if (op == 2u) {
            number(out, run);
            out += '^';
            out.append(reinterpret_cast<const char *>(ref_bases), len);
            ref_bases += len;
            run = 0;
        }
    }
    number(out, run);
}

// The affine score of written =/X/I/D entries (S adds nothing): match per = column, -mismatch per X column, -(gap_open +
// L gap_extend) per I or D entry of length L.  bmv_realign's score of the same path; `--affine --left-align` writes it as
// AS:i, since a merge or a dropped D changes the score the realignment returned.
inline int64_t affine_score(const uint32_t *entry, size_t n, uint32_t match, uint32_t mismatch, uint32_t gap_open, uint32_t gap_extend) {
    int64_t score = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t op = entry[i] & 15u;
        const int64_t len = entry[i] >> 4;
        if (op == 7u) score += len * match;
        else if (op == 8u) score -= len * mismatch;
        else if (op == 1u || op == 2u) score -= gap_open + len * static_cast<int64_t>(gap_extend);
    }
    return score;
}

// bmv_annotate's contract (include/bmv.h) restated for the host, over a genome laid out as the verifier's: forward-strand pos,
// ref_len, =/X/I/D entries, NM and the reference letters under X and D columns of alignments given with their begin and M/I/D
// CIGAR.  The locator uses it with a verifier that has no annotation pass of its own (the oracle-backed test tools); the product
// annotates on the device.
inline void annotate_on_host(const uint8_t *genome, const uint8_t *reads, const uint64_t *text_start, const uint32_t *text_len,
                             const uint8_t *text_rc, const uint64_t *query_start, const uint32_t *query_len, const uint32_t *begin,
                             const uint64_t *cigar_offset, const uint32_t *cigar, uint32_t n, annotation &out) {
    out.nm.assign(n, 0);
    out.pos.assign(n, 0);
    out.ref_len.assign(n, 0);
    out.xcigar.clear();
    out.ref_bases.clear();
    out.xcigar_offset.assign(static_cast<size_t>(n) + 1, 0);
    out.ref_offset.assign(static_cast<size_t>(n) + 1, 0);
    for (uint32_t a = 0; a < n; a++) {
        const uint64_t c0 = cigar_offset[a], c1 = cigar_offset[a + 1];
        const size_t first = out.xcigar.size();
        auto push = [&](uint32_t op, uint32_t len) {
            if (out.xcigar.size() > first && (out.xcigar.back() & 15u) == op)
                out.xcigar.back() += len << 4;
            else
                out.xcigar.push_back(len << 4 | op);
        };
        if (c1 > c0) {
            uint32_t r_len = 0;
            for (uint64_t x = c0; x < c1; x++)
                if ((cigar[x] & 15u) != 1u) r_len += cigar[x] >> 4;
            const bool rc = text_rc[a] != 0;
            const uint32_t pos = rc ? text_len[a] - begin[a] - r_len : begin[a];
            const uint8_t *t = genome + text_start[a] + pos, *q = reads + query_start[a];
            int64_t qi = rc ? static_cast<int64_t>(query_len[a]) - 1 : 0;
            const int64_t step = rc ? -1 : 1;
            for (uint64_t k = 0; k < c1 - c0; k++) {
                const uint32_t e = cigar[rc ? c1 - 1 - k : c0 + k], op = e & 15u, len = e >> 4;
                if (op == 0u) {
                    for (uint32_t x = 0; x < len; x++, t++, qi += step) {
                        const uint8_t tb = dna4_rank(*t), qb = rc ? 3u - dna4_rank(q[qi]) : dna4_rank(q[qi]);
                        push(tb == qb ? 7u : 8u, 1u);
                        if (tb != qb) {
                            out.ref_bases.push_back(static_cast<uint8_t>(dna4_char(tb)));
                            out.nm[a]++;
                        }
                    }
                } else if (op == 1u) {
                    push(1u, len);
                    out.nm[a] += len;
                    qi += step * static_cast<int64_t>(len);
                } else {
                    push(2u, len);
                    out.nm[a] += len;
                    for (uint32_t x = 0; x < len; x++, t++) out.ref_bases.push_back(static_cast<uint8_t>(dna4_char(dna4_rank(*t))));
                }
            }
            out.pos[a] = pos;
            out.ref_len[a] = r_len;
        }
        out.xcigar_offset[a + 1] = out.xcigar.size();
        out.ref_offset[a + 1] = out.ref_bases.size();
    }
}

// reverse complement of a read that is folded to A C G T already (append_dna4's output)
inline void append_revcomp(std::string &out, std::string_view folded) {
    for (size_t i = folded.size(); i-- > 0;) out += "TGCA"[dna4_rank(static_cast<uint8_t>(folded[i]))];
}

}  // namespace sam_tags

}  // namespace bm
