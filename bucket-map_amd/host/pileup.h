// pileup.h -- the pileup rule of include/bmp.h as plain C++17: what bmp_begin / bmp_add / bmp_finish compute on the device,
// value for value.
//
// The rule (counted records, the eight counters per position, the reference alleles, sites and their kinds, the six sums per
// reference and what is left out) is stated in include/bmp.h; tests/pileup_rule.py restates it a third time in Python.  This
// copy is the counter of every build without a device behind it (block_compressor's defaults in bgzf.h, so the oracle-backed
// test tools) and the reference the device is compared with.  It also writes the file of --pileup.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace bm {

constexpr size_t kPileupCounters = 8;    // BMP_N_COUNTERS: A C G T N DEL INS LOWQ
constexpr size_t kPileupStats = 6;       // BMP_N_STATS: n_reads, n_low_mapq, n_left_out, n_bases, n_lowq, n_sites
constexpr size_t kPileupSiteWords = 12;  // BMP_SITE_WORDS: reference, position, allele, the counters, kind

struct pileup_thresholds {               // the order of bmp_begin's thresholds; the defaults are the command line's
    uint32_t min_mapq = 0, min_bq = 13, min_alt = 2, min_frac_ppm = 200000;
};

struct pileup_result {
    std::vector<uint32_t> sites;    // kPileupSiteWords per site
    std::vector<uint64_t> stats;    // kPileupStats per reference
    size_t n_sites() const { return sites.size() / kPileupSiteWords; }
};

class pileup_counter {
    std::vector<uint32_t> ref_len_;
    std::vector<uint64_t> base_;    // reference r: positions base_[r] .. base_[r + 1] - 1
    std::vector<uint32_t> cnt_;     // kPileupCounters per position
    std::vector<uint8_t> allele_;   // 0 .. 3, or 4 for none
    std::vector<uint64_t> stats_;
    pileup_thresholds th_;
    bool begun_ = false;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);   // little-endian hosts only, like the rest of the tool
        return v;
    }
    static uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }

public:
    // ref_bases[r]: ref_len[r] bytes
    void begin(const uint32_t *ref_len, size_t n_ref, const uint8_t *const *ref_bases, const pileup_thresholds &th) {
        if (n_ref == 0) throw std::runtime_error("--pileup: no reference");
        uint64_t bases = 0;
        for (size_t r = 0; r < n_ref; r++) {
            if (ref_len[r] == 0) throw std::runtime_error("--pileup: reference " + std::to_string(r) + " has the length 0");
            bases += ref_len[r];
        }
        if (bases > (uint64_t{1} << 32) - (uint64_t{1} << 20) || bases + n_ref > 0xFFFFFFFEull)
            throw std::runtime_error("--pileup: " + std::to_string(bases) + " bases, at most 2^32 - 2^20 are counted in one go");
        if (th.min_alt == 0) throw std::runtime_error("--pileup: min_alt is 0");
        if (th.min_frac_ppm > 1000000u) throw std::runtime_error("--pileup: a fraction of " + std::to_string(th.min_frac_ppm) + " ppm");
        for (size_t r = 0; r < n_ref; r++)
            if (!ref_bases[r]) throw std::runtime_error("--pileup: reference " + std::to_string(r) + " has no bases");
        th_ = th;
        ref_len_.assign(ref_len, ref_len + n_ref);
        base_.assign(n_ref + 1, 0);
        for (size_t r = 0; r < n_ref; r++) base_[r + 1] = base_[r] + ref_len[r];
        cnt_.assign(base_[n_ref] * kPileupCounters, 0);
        allele_.resize(base_[n_ref]);
        for (size_t r = 0; r < n_ref; r++)
            for (uint32_t p = 0; p < ref_len[r]; p++) {
                const uint8_t u = ref_bases[r][p] & 0xDFu;   // either case
                allele_[base_[r] + p] = u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
            }
        stats_.assign(n_ref * kPileupStats, 0);
        begun_ = true;
    }

    // whole records in[rec_offset[i], rec_offset[i + 1]); skip may be null
    void add(const uint8_t *in, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        if (!begun_) throw std::runtime_error("--pileup: records before the references");
        // the checks first: a refused call changes nothing
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const uint64_t length = rec_offset[i + 1] - rec_offset[i];
            if (length < 36) throw std::runtime_error("--pileup: a record of " + std::to_string(length) + " bytes");
            const int32_t ref = static_cast<int32_t>(u32(r + 4));
            const uint32_t l_name = r[12], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if (36ull + l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2 + l_seq > length)
                throw std::runtime_error("--pileup: a record's fields lie beyond its end");
            uint64_t query = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = u32(r + 36 + l_name + 4ull * k), op = c & 15u;
                if (op > 8) throw std::runtime_error("--pileup: a CIGAR op with the code " + std::to_string(op));
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
            }
            if (n_cigar && l_seq && query != l_seq)
                throw std::runtime_error("--pileup: a CIGAR of " + std::to_string(query) + " query bases on a record of " + std::to_string(l_seq));
            if (ref >= 0 && static_cast<size_t>(ref) >= ref_len_.size() && !(flag & 4u))
                throw std::runtime_error("--pileup: a record names reference " + std::to_string(ref) + ", there are " + std::to_string(ref_len_.size()));
        }
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const int32_t ref = static_cast<int32_t>(u32(r + 4)), pos = static_cast<int32_t>(u32(r + 8));
            const uint32_t l_name = r[12], mapq = r[13], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if ((flag & (0x4u | 0x100u | 0x200u | 0x400u)) || (skip && skip[i])) continue;
            if (ref < 0 || static_cast<size_t>(ref) >= ref_len_.size() || pos < 0 || static_cast<uint32_t>(pos) >= ref_len_[ref] || n_cigar == 0) continue;
            const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar, *qual = seq + (static_cast<uint64_t>(l_seq) + 1) / 2;
            uint64_t *st = stats_.data() + static_cast<size_t>(ref) * kPileupStats;
            if (l_seq == 0 || (n_cigar == 2 && u32(cigar) == (l_seq << 4 | 4u) && (u32(cigar + 4) & 15u) == 3)) {   // ... or the long-CIGAR placeholder
                st[2]++;
                continue;
            }
            if (mapq < th_.min_mapq) {
                st[1]++;
                continue;
            }
            st[0]++;
            const uint64_t rlen = ref_len_[ref];
            uint32_t *c = cnt_.data() + base_[ref] * kPileupCounters;
            uint64_t rc = static_cast<uint64_t>(pos), qc = 0;
            bool anchored = false;                       // an M, =, X or D of a length > 0 came before
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t w = u32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
                const bool block = op == 0 || op == 7 || op == 8;
                if ((block || op == 2) && len && rc < rlen) {
                    const uint64_t e = std::min<uint64_t>(rc + len, rlen);
                    for (uint64_t j = 0; j < e - rc; j++) {
                        uint32_t which = 5;              // DEL
                        if (block) {
                            const uint64_t at = qc + j;
                            const uint32_t q = qual[at], code = (seq[at >> 1] >> ((at & 1) ? 0 : 4)) & 15u;
                            which = q != 0xFF && q < th_.min_bq ? 7u : code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
                        }
                        c[(rc + j) * kPileupCounters + which]++;
                    }
                }
                if (op == 1 && len && anchored && rc >= 1 && rc - 1 < rlen) c[(rc - 1) * kPileupCounters + 6]++;
                if ((block || op == 2) && len) anchored = true;
                if (block || op == 2 || op == 3) rc += len;
                if (block || op == 1 || op == 4) qc += len;
            }
        }
    }

    // the sites and the sums of everything added; counts, where given, receives every position's eight counters, the
    // references back to back
    void finish(pileup_result &out, std::vector<uint32_t> *counts = nullptr) {
        if (!begun_) throw std::runtime_error("--pileup: a result before the references");
        out.sites.clear();
        for (size_t r = 0; r < ref_len_.size(); r++) {
            uint64_t *st = stats_.data() + r * kPileupStats;
            st[3] = st[4] = st[5] = 0;
            for (uint32_t p = 0; p < ref_len_[r]; p++) {
                const uint32_t *v = cnt_.data() + (base_[r] + p) * kPileupCounters;
                const uint32_t allele = allele_[base_[r] + p];
                const uint64_t five = static_cast<uint64_t>(v[0]) + v[1] + v[2] + v[3] + v[4], span = five + v[5];
                const uint64_t bar = static_cast<uint64_t>(th_.min_frac_ppm) * span;
                auto passes = [&](uint32_t x) { return x >= th_.min_alt && static_cast<uint64_t>(x) * 1000000u >= bar; };
                uint32_t alt = 0;
                for (uint32_t k = 0; k < 4; k++)
                    if (k != allele) alt = std::max(alt, v[k]);
                const uint32_t kind = (allele < 4 && passes(alt) ? 1u : 0u) | (passes(v[5]) ? 2u : 0u) | (passes(v[6]) ? 4u : 0u);
                st[3] += five;
                st[4] += v[7];
                if (kind) {
                    st[5]++;
                    out.sites.insert(out.sites.end(), {static_cast<uint32_t>(r), p, allele, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], kind});
                }
            }
        }
        out.stats = stats_;
        if (counts) *counts = cnt_;
    }
};

// --pileup FILE: the header line, then one line per site; pos is 1-based, ref the upper-case letter or '.', kind the letters
// of S, D, I that apply
inline void write_pileup_file(std::ostream &out, const pileup_result &res, const std::vector<std::string> &ref_ids) {
    std::string buf = "#rname\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\tlowq\tkind\n";
    for (size_t k = 0; k < res.n_sites(); k++) {
        const uint32_t *s = res.sites.data() + kPileupSiteWords * k;
        buf += ref_ids.at(s[0]);
        buf += '\t', buf += std::to_string(static_cast<uint64_t>(s[1]) + 1);
        buf += '\t', buf += s[2] < 4 ? "ACGT"[s[2]] : '.';
        for (size_t f = 3; f < 11; f++) buf += '\t', buf += std::to_string(s[f]);
        buf += '\t';
        if (s[11] & 1u) buf += 'S';
        if (s[11] & 2u) buf += 'D';
        if (s[11] & 4u) buf += 'I';
        buf += '\n';
        if (buf.size() > (1u << 20)) out.write(buf.data(), static_cast<std::streamsize>(buf.size())), buf.clear();
    }
    out.write(buf.data(), static_cast<std::streamsize>(buf.size()));
}

}  // namespace bm
