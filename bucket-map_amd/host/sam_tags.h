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

// reverse complement of a read that is folded to A C G T already (append_dna4's output)
inline void append_revcomp(std::string &out, std::string_view folded) {
    for (size_t i = folded.size(); i-- > 0;) out += "TGCA"[dna4_rank(static_cast<uint8_t>(folded[i]))];
}

}  // namespace sam_tags

}  // namespace bm
