// bias.h -- the strand-bias and mapping-quality rule of include/bmb.h as plain C++17: what bmb_begin / bmb_add / bmb_annotate
// compute on the device, value for value, and the text --vcf-bias adds to a SNV line of the VCF.
//
// The rule (the two parameters, the five cells per position, MQ, the 2x2 table, FS from the two integer tables, the sixteen
// words of an annotation and what is left out) is stated in include/bmb.h; the counted records and the walk are those of
// include/bmp.h, which bases count is include/bmg.h's.  tests/bias_rule.py restates it a third time in Python.  The tables LF
// and E are arguments here: bmb_tables of libbmf.so makes them.  This copy is the annotator of every build without a device
// behind it (block_compressor's defaults in bgzf.h, so the oracle-backed test tools) and the reference the device is compared
// with.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace bm {

constexpr size_t kBiasStrandCells = 4;      // BMB_N_STRAND_CELLS: A C G T
constexpr size_t kBiasCallWords = 24;       // BMB_CALL_WORDS: a call of the genotype caller
constexpr size_t kBiasOutWords = 16;        // BMB_OUT_WORDS
constexpr size_t kBiasNLf = 65536, kBiasNE = 12001;
constexpr uint32_t kBiasFsCap = 6000, kBiasFsMaxN = 65535;
constexpr uint32_t kBiasAnnotated = 1, kBiasNoFs = 2;      // the flags of an annotation
constexpr size_t kBiasWFwd = 0, kBiasWRev = 4, kBiasWMq = 8, kBiasWFs = 9, kBiasWFlags = 10;

struct bias_params {                        // the order of bmb_begin's params; the defaults are the command line's
    uint32_t min_mapq = 0, min_bq = 13;
};

struct bias_tables {
    std::vector<uint32_t> lf;               // kBiasNLf
    std::vector<uint64_t> e;                // kBiasNE
};

// floor(sqrt(v))
inline uint64_t bias_isqrt(uint64_t v) {
    uint64_t r = 0;
    for (int b = 31; b >= 0; b--) {
        const uint64_t t = r | (uint64_t{1} << b);
        if (t * t <= v) r = t;
    }
    return r;
}

// FS of the table ((a, b), (c, d)) in centi-phred; false where the rule gives none
inline bool bias_fs(uint64_t a, uint64_t b, uint64_t c, uint64_t d, const bias_tables &t, uint32_t &fs) {
    const uint64_t r1 = a + b, r2 = c + d, c1 = a + c, c2 = b + d;
    fs = 0;
    if (r1 + r2 > kBiasFsMaxN || r1 == 0 || r2 == 0 || c1 == 0 || c2 == 0) return false;
    const uint64_t x_lo = c1 > r2 ? c1 - r2 : 0, x_hi = std::min(r1, c1);
    auto cost = [&](uint64_t x) { return static_cast<uint64_t>(t.lf[x]) + t.lf[r1 - x] + t.lf[c1 - x] + t.lf[r2 + x - c1]; };   // -w(x)
    uint64_t least = ~uint64_t{0};
    for (uint64_t x = x_lo; x <= x_hi; x++) least = std::min(least, cost(x));
    const uint64_t mine = cost(a);
    uint64_t s_all = 0, s_ext = 0;
    for (uint64_t x = x_lo; x <= x_hi; x++) {
        const uint64_t v = cost(x), k = v - least, e = k < kBiasNE ? t.e[k] : 0;
        s_all += e;
        if (v + 4 >= mine) s_ext += e;                  // w(x) <= w(a) + 4
    }
    const unsigned __int128 rhs = static_cast<unsigned __int128>(s_ext) << 40;
    uint32_t k = 0;
    while (k < kBiasFsCap && static_cast<unsigned __int128>(s_all) * t.e[k] > rhs) k++;
    fs = k;
    return true;
}

class bias_counter {
    std::vector<uint32_t> ref_len_;
    std::vector<uint64_t> base_;    // reference r: positions base_[r] .. base_[r + 1] - 1
    std::vector<uint64_t> strand_;  // kBiasStrandCells per position: fwd << 32 | rev
    std::vector<uint64_t> mapq_;    // one per position: n << 40 | S
    bias_params pr_;
    bool begun_ = false;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);   // little-endian hosts only, like the rest of the tool
        return v;
    }
    static uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }

public:
    void begin(const uint32_t *ref_len, size_t n_ref, const bias_params &pr) {
        if (n_ref == 0) throw std::runtime_error("--vcf-bias: no reference");
        uint64_t bases = 0;
        for (size_t r = 0; r < n_ref; r++) {
            if (ref_len[r] == 0) throw std::runtime_error("--vcf-bias: reference " + std::to_string(r) + " has the length 0");
            bases += ref_len[r];
        }
        if (bases > (uint64_t{1} << 32) - (uint64_t{1} << 20) || bases + n_ref > 0xFFFFFFFEull)
            throw std::runtime_error("--vcf-bias: " + std::to_string(bases) + " bases, at most 2^32 - 2^20 are counted in one go");
        pr_ = pr;
        ref_len_.assign(ref_len, ref_len + n_ref);
        base_.assign(n_ref + 1, 0);
        for (size_t r = 0; r < n_ref; r++) base_[r + 1] = base_[r] + ref_len[r];
        strand_.assign(base_[n_ref] * kBiasStrandCells, 0);
        mapq_.assign(base_[n_ref], 0);
        begun_ = true;
    }

    // whole records in[rec_offset[i], rec_offset[i + 1]); skip may be null
    void add(const uint8_t *in, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        if (!begun_) throw std::runtime_error("--vcf-bias: records before the references");
        // the checks first: a refused call changes nothing
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const uint64_t length = rec_offset[i + 1] - rec_offset[i];
            if (length < 36) throw std::runtime_error("--vcf-bias: a record of " + std::to_string(length) + " bytes");
            const int32_t ref = static_cast<int32_t>(u32(r + 4));
            const uint32_t l_name = r[12], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if (36ull + l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2 + l_seq > length)
                throw std::runtime_error("--vcf-bias: a record's fields lie beyond its end");
            uint64_t query = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = u32(r + 36 + l_name + 4ull * k), op = c & 15u;
                if (op > 8) throw std::runtime_error("--vcf-bias: a CIGAR op with the code " + std::to_string(op));
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
            }
            if (n_cigar && l_seq && query != l_seq)
                throw std::runtime_error("--vcf-bias: a CIGAR of " + std::to_string(query) + " query bases on a record of " + std::to_string(l_seq));
            if (ref >= 0 && static_cast<size_t>(ref) >= ref_len_.size() && !(flag & 4u))
                throw std::runtime_error("--vcf-bias: a record names reference " + std::to_string(ref) + ", there are " + std::to_string(ref_len_.size()));
        }
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const int32_t ref = static_cast<int32_t>(u32(r + 4)), pos = static_cast<int32_t>(u32(r + 8));
            const uint32_t l_name = r[12], mapq = r[13], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if ((flag & (0x4u | 0x100u | 0x200u | 0x400u)) || (skip && skip[i])) continue;
            if (ref < 0 || static_cast<size_t>(ref) >= ref_len_.size() || pos < 0 || static_cast<uint32_t>(pos) >= ref_len_[ref] || n_cigar == 0) continue;
            const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar, *qual = seq + (static_cast<uint64_t>(l_seq) + 1) / 2;
            if (l_seq == 0 || (n_cigar == 2 && u32(cigar) == (l_seq << 4 | 4u) && (u32(cigar + 4) & 15u) == 3)) continue;   // ... or the long-CIGAR placeholder
            if (mapq < pr_.min_mapq) continue;
            const uint64_t rlen = ref_len_[ref];
            const uint64_t s_add = (flag & 0x10u) ? uint64_t{1} : uint64_t{1} << 32, m_add = (uint64_t{1} << 40) + static_cast<uint64_t>(mapq) * mapq;
            uint64_t *s = strand_.data() + base_[ref] * kBiasStrandCells, *m = mapq_.data() + base_[ref];
            uint64_t rc = static_cast<uint64_t>(pos), qc = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t w = u32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
                const bool block = op == 0 || op == 7 || op == 8;
                if (block && len && rc < rlen) {
                    const uint64_t e = std::min<uint64_t>(rc + len, rlen);
                    for (uint64_t j = 0; j < e - rc; j++) {
                        const uint64_t at = qc + j;
                        const uint32_t q = qual[at], code = (seq[at >> 1] >> ((at & 1) ? 0 : 4)) & 15u;
                        if (q != 0xFF && q < pr_.min_bq) continue;
                        const uint32_t letter = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
                        if (letter == 4) continue;
                        s[(rc + j) * kBiasStrandCells + letter] += s_add;
                        m[rc + j] += m_add;
                    }
                }
                if (block || op == 2 || op == 3) rc += len;
                if (block || op == 1 || op == 4) qc += len;
            }
        }
    }

    // the annotations of the n_calls calls (kBiasCallWords each, in any order) from everything added so far: out receives
    // kBiasOutWords per call
    void annotate(const uint32_t *calls, size_t n_calls, const bias_tables &t, std::vector<uint32_t> &out) const {
        if (!begun_) throw std::runtime_error("--vcf-bias: annotations before the references");
        if (t.lf.size() != kBiasNLf || t.e.size() != kBiasNE) throw std::runtime_error("--vcf-bias: the tables have the wrong sizes");
        for (size_t i = 0; i < n_calls; i++) {
            const uint32_t *c = calls + kBiasCallWords * i;
            if (!(c[3] & 2u)) continue;
            if (c[0] >= ref_len_.size() || c[1] >= ref_len_[c[0]] || c[2] > 3 || c[4] > 3 || c[5] > 3)
                throw std::runtime_error("--vcf-bias: a call at base " + std::to_string(c[1]) + " of reference " + std::to_string(c[0]));
        }
        out.assign(n_calls * kBiasOutWords, 0);
        for (size_t i = 0; i < n_calls; i++) {
            const uint32_t *c = calls + kBiasCallWords * i;
            uint32_t *o = out.data() + kBiasOutWords * i;
            if (!(c[3] & 2u)) continue;
            const uint64_t slot = base_[c[0]] + c[1];
            uint64_t fwd[4], rev[4];
            for (size_t a = 0; a < 4; a++) {
                fwd[a] = strand_[slot * kBiasStrandCells + a] >> 32, rev[a] = strand_[slot * kBiasStrandCells + a] & 0xFFFFFFFFull;
                o[kBiasWFwd + a] = static_cast<uint32_t>(fwd[a]), o[kBiasWRev + a] = static_cast<uint32_t>(rev[a]);
            }
            const uint64_t n = mapq_[slot] >> 40, S = mapq_[slot] & ((uint64_t{1} << 40) - 1);
            o[kBiasWMq] = n ? static_cast<uint32_t>(bias_isqrt(10000 * S / n)) : 0;
            const uint32_t R = c[2];
            uint64_t cc = 0, dd = 0;
            if (c[4] != R) cc += fwd[c[4]], dd += rev[c[4]];
            if (c[5] != R && c[5] != c[4]) cc += fwd[c[5]], dd += rev[c[5]];
            uint32_t fs = 0;
            const bool has = bias_fs(fwd[R], rev[R], cc, dd, t, fs);
            o[kBiasWFs] = fs;
            o[kBiasWFlags] = kBiasAnnotated | (has ? 0u : kBiasNoFs);
            o[11] = static_cast<uint32_t>(n);
            o[12] = static_cast<uint32_t>(fwd[R]), o[13] = static_cast<uint32_t>(rev[R]), o[14] = static_cast<uint32_t>(cc), o[15] = static_cast<uint32_t>(dd);
        }
    }

    const std::vector<uint64_t> &strand_cells() const { return strand_; }
    const std::vector<uint64_t> &mapq_cells() const { return mapq_; }
};

// what --vcf-bias hands to the writer of the VCF: the annotations of the calls, in their order, and the two thresholds in
// phred (max_fs 1 .. 60; min_mq 0 .. 255, 0 is off)
struct vcf_bias {
    std::vector<uint32_t> notes;    // kBiasOutWords per call
    uint32_t max_fs = 60, min_mq = 0;
    const uint32_t *at(size_t call) const { return notes.data() + kBiasOutWords * call; }
    bool strand_bias(const uint32_t *b) const { return !(b[kBiasWFlags] & kBiasNoFs) && b[kBiasWFs] >= 100u * max_fs; }
    bool low_mq(const uint32_t *b) const { return b[kBiasWMq] < 100u * min_mq; }
};

struct bias_summary {
    uint64_t annotated = 0, strand_bias = 0, low_mq = 0, no_fs = 0;
};

inline bias_summary summarize_bias(const vcf_bias &v) {
    bias_summary s;
    for (size_t k = 0; k < v.notes.size() / kBiasOutWords; k++) {
        const uint32_t *b = v.at(k);
        if (!(b[kBiasWFlags] & kBiasAnnotated)) continue;
        s.annotated++;
        s.strand_bias += v.strand_bias(b), s.low_mq += v.low_mq(b), s.no_fs += (b[kBiasWFlags] & kBiasNoFs) != 0;
    }
    return s;
}

inline std::string bias_summary_line(const bias_summary &s) {
    return "Bias: " + std::to_string(s.annotated) + " variants annotated (" + std::to_string(s.strand_bias) + " StrandBias, " + std::to_string(s.low_mq) +
           " LowMQ, " + std::to_string(s.no_fs) + " without FS)";
}

// the lines --vcf-bias adds to the header: after the INFO lines, after the FILTER line, after FORMAT=AD
inline std::string bias_info_lines() {
    return "##INFO=<ID=FS,Number=1,Type=Float,Description=\"Phred-scaled p-value of Fisher's exact test of the strands of reference and alternative bases, at most 60\">\n"
           "##INFO=<ID=MQ,Number=1,Type=Float,Description=\"Root mean square of the mapping qualities of the counted bases\">\n";
}
inline std::string bias_filter_lines(const vcf_bias &v) {
    return "##FILTER=<ID=StrandBias,Description=\"FS at least " + std::to_string(v.max_fs) + "\">\n##FILTER=<ID=LowMQ,Description=\"MQ below " +
           std::to_string(v.min_mq) + "\">\n";
}
inline std::string bias_format_lines() {
    return "##FORMAT=<ID=ADF,Number=R,Type=Integer,Description=\"Counted bases of each allele on the forward strand\">\n"
           "##FORMAT=<ID=ADR,Number=R,Type=Integer,Description=\"Counted bases of each allele on the reverse strand\">\n";
}

// ";FS=ff.ff;MQ=mm.mm" of an annotation, FS left out where there is none
inline std::string bias_info(const uint32_t *b) {
    char text[64];
    std::string out;
    if (!(b[kBiasWFlags] & kBiasNoFs)) {
        std::snprintf(text, sizeof text, ";FS=%u.%02u", b[kBiasWFs] / 100, b[kBiasWFs] % 100);
        out += text;
    }
    std::snprintf(text, sizeof text, ";MQ=%u.%02u", b[kBiasWMq] / 100, b[kBiasWMq] % 100);
    return out + text;
}

}  // namespace bm
