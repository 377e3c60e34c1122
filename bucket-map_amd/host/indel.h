// indel.h -- the indel rule of include/bmn.h in plain C++ (the header states it in full; this is the same rule, not the device's
// code), the summary line and the VCF lines of --vcf-indels.  The oracle-backed tools call with it; the product plugs bmn_* in
// behind block_compressor's indel_* virtuals and uses only the writer.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

namespace bm {

constexpr size_t kIndelEventWords = 4;      // BMN_EVENT_WORDS
constexpr size_t kIndelAlleleWords = 8;     // BMN_ALLELE_WORDS
constexpr size_t kIndelCallWords = 16;      // BMN_CALL_WORDS
constexpr size_t kIndelStats = 3;           // BMN_N_STATS: n_reads n_low_mapq n_left_out
constexpr uint32_t kIndelIns = 1u << 31, kIndelOther = 1u << 30, kIndelLenMask = (1u << 28) - 1, kIndelMaxIns = 32;
constexpr uint32_t kIndelGenotyped = 1, kIndelVariant = 2;   // the flags of a call

struct indel_params {                       // the order of bmn_begin's params; the defaults are the command line's
    uint32_t min_mapq = 0, min_alt = 2, min_frac_ppm = 200000, q_indel = 30, prior = 4000;
};

struct indel_result {
    std::vector<uint32_t> alleles;          // kIndelAlleleWords each, ascending by (slot, w1, seq)
    std::vector<uint32_t> calls;            // kIndelCallWords each, in (reference, anchor) order
    std::vector<uint64_t> stats;            // kIndelStats per reference
    uint64_t n_events = 0;
    size_t n_alleles() const { return alleles.size() / kIndelAlleleWords; }
    size_t n_calls() const { return calls.size() / kIndelCallWords; }
};

class indel_caller {
    using event = std::tuple<uint32_t, uint32_t, uint64_t>;   // slot, w1, seq: the order of the 128-bit key
    std::vector<uint32_t> ref_len_;
    std::vector<uint64_t> base_;    // reference r: slots base_[r] .. base_[r + 1] - 1
    std::vector<uint32_t> cover_;   // the +1 / -1 of the extents until finish, wrapping
    std::vector<uint64_t> stats_;
    std::vector<event> events_;
    indel_params pr_;
    bool begun_ = false;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);   // little-endian hosts only, like the rest of the tool
        return v;
    }
    static uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }
    static uint32_t sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(v); }

public:
    void begin(const uint32_t *ref_len, size_t n_ref, const indel_params &pr) {
        if (n_ref == 0) throw std::runtime_error("--vcf-indels: no reference");
        uint64_t bases = 0;
        for (size_t r = 0; r < n_ref; r++) {
            if (ref_len[r] == 0) throw std::runtime_error("--vcf-indels: reference " + std::to_string(r) + " has the length 0");
            bases += ref_len[r];
        }
        if (bases > (uint64_t{1} << 32) - (uint64_t{1} << 20) || bases + n_ref > 0xFFFFFFFEull)
            throw std::runtime_error("--vcf-indels: " + std::to_string(bases) + " bases, at most 2^32 - 2^20 are counted in one go");
        if (pr.min_alt == 0) throw std::runtime_error("--vcf-indels: min_alt is 0");
        if (pr.min_frac_ppm > 1000000) throw std::runtime_error("--vcf-indels: min_frac_ppm is above 1 000 000");
        if (pr.q_indel == 0 || pr.q_indel > 93) throw std::runtime_error("--vcf-indels: q_indel is " + std::to_string(pr.q_indel) + ", not 1 .. 93");
        pr_ = pr;
        ref_len_.assign(ref_len, ref_len + n_ref);
        base_.assign(n_ref + 1, 0);
        for (size_t r = 0; r < n_ref; r++) base_[r + 1] = base_[r] + ref_len[r];
        cover_.assign(base_[n_ref], 0);
        stats_.assign(n_ref * kIndelStats, 0);
        events_.clear();
        begun_ = true;
    }

    // whole records in[rec_offset[i], rec_offset[i + 1]); skip may be null
    void add(const uint8_t *in, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        if (!begun_) throw std::runtime_error("--vcf-indels: records before the references");
        // the checks first: a refused call changes nothing
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const uint64_t length = rec_offset[i + 1] - rec_offset[i];
            if (length < 36) throw std::runtime_error("--vcf-indels: a record of " + std::to_string(length) + " bytes");
            const int32_t ref = static_cast<int32_t>(u32(r + 4));
            const uint32_t l_name = r[12], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if (36ull + l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2 + l_seq > length)
                throw std::runtime_error("--vcf-indels: a record's fields lie beyond its end");
            uint64_t query = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = u32(r + 36 + l_name + 4ull * k), op = c & 15u;
                if (op > 8) throw std::runtime_error("--vcf-indels: a CIGAR op with the code " + std::to_string(op));
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
            }
            if (n_cigar && l_seq && query != l_seq)
                throw std::runtime_error("--vcf-indels: a CIGAR of " + std::to_string(query) + " query bases on a record of " + std::to_string(l_seq));
            if (ref >= 0 && static_cast<size_t>(ref) >= ref_len_.size() && !(flag & 4u))
                throw std::runtime_error("--vcf-indels: a record names reference " + std::to_string(ref) + ", there are " + std::to_string(ref_len_.size()));
        }
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const int32_t ref = static_cast<int32_t>(u32(r + 4)), pos = static_cast<int32_t>(u32(r + 8));
            const uint32_t l_name = r[12], mapq = r[13], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if ((flag & (0x4u | 0x100u | 0x200u | 0x400u)) || (skip && skip[i])) continue;
            if (ref < 0 || static_cast<size_t>(ref) >= ref_len_.size() || pos < 0 || static_cast<uint32_t>(pos) >= ref_len_[ref] || n_cigar == 0) continue;
            const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar;
            uint64_t *st = stats_.data() + static_cast<size_t>(ref) * kIndelStats;
            if (l_seq == 0 || (n_cigar == 2 && u32(cigar) == (l_seq << 4 | 4u) && (u32(cigar + 4) & 15u) == 3)) {   // ... or the long-CIGAR placeholder
                st[2]++;
                continue;
            }
            if (mapq < pr_.min_mapq) {
                st[1]++;
                continue;
            }
            st[0]++;
            const uint64_t rlen = ref_len_[ref];
            uint64_t end = static_cast<uint64_t>(pos);
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t w = u32(cigar + 4ull * k), op = w & 15u;
                if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) end += w >> 4;
            }
            const uint64_t endc = std::min(end, rlen);
            if (endc >= static_cast<uint64_t>(pos) + 2) {
                cover_[base_[ref] + pos] += 1u;
                cover_[base_[ref] + endc - 1] -= 1u;
            }
            uint64_t rc = static_cast<uint64_t>(pos), qc = 0;
            bool anchored = false;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t w = u32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
                const bool block = op == 0 || op == 7 || op == 8;
                if ((op == 1 || op == 2) && len && anchored && rc >= 1) {
                    const uint32_t slot = static_cast<uint32_t>(base_[ref] + rc - 1);
                    if (op == 2 && rc + len <= rlen) events_.emplace_back(slot, len, 0);
                    if (op == 1 && rc < endc) {
                        bool other = len > kIndelMaxIns;
                        uint64_t bits = 0;
                        for (uint32_t j = 0; !other && j < len; j++) {
                            const uint64_t at = qc + j;
                            const uint32_t code = (seq[at >> 1] >> ((at & 1) ? 0 : 4)) & 15u;
                            const uint32_t two = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
                            if (two == 4) other = true;
                            else bits |= static_cast<uint64_t>(two) << (2 * j);
                        }
                        events_.emplace_back(slot, len | kIndelIns | (other ? kIndelOther : 0u), other ? 0 : bits);
                    }
                }
                if ((block || op == 2) && len) anchored = true;
                if (block || op == 2 || op == 3) rc += len;
                if (block || op == 1 || op == 4) qc += len;
            }
        }
    }

    // the call of one anchor from its alleles (in allele order) and its cover; false: the anchor is no site
    static bool call_anchor(const uint32_t *alleles, size_t n, uint32_t D, const indel_params &pr, uint32_t *o) {
        uint64_t E = 0;
        uint32_t n_alt = 0;
        const uint32_t *alt = nullptr;
        for (size_t a = 0; a < n; a++) {
            const uint32_t *x = alleles + kIndelAlleleWords * a;
            E += x[5];
            if (!(x[2] & kIndelOther) && x[5] > n_alt) n_alt = x[5], alt = x;   // a tie keeps the first
        }
        if (!alt || D == 0 || n_alt < pr.min_alt || static_cast<uint64_t>(n_alt) * 1000000ull < static_cast<uint64_t>(pr.min_frac_ppm) * D) return false;
        const uint64_t n_ref = D > E ? D - E : 0;
        const uint64_t L[3] = {100ull * pr.q_indel * n_alt, 301ull * (n_ref + n_alt) + pr.prior, 100ull * pr.q_indel * n_ref + pr.prior};
        uint32_t g = 0;                                  // a tie goes to RR, then to RA
        if (L[1] < L[g]) g = 1;
        if (L[2] < L[g]) g = 2;
        const uint64_t second = std::min(L[(g + 1) % 3], L[(g + 2) % 3]);
        for (size_t k = 0; k < 5; k++) o[k] = alt[k];
        o[5] = kIndelGenotyped | (g ? kIndelVariant : 0u);
        o[6] = g;
        o[7] = static_cast<uint32_t>(std::min<uint64_t>(99, (second - L[g]) / 100));
        o[8] = sat32(L[0] - L[g]);
        o[9] = static_cast<uint32_t>(n_ref), o[10] = n_alt, o[11] = sat32(E - n_alt), o[12] = D;
        for (size_t k = 0; k < 3; k++) o[13 + k] = sat32(L[k] - L[g]);
        return true;
    }

    void finish(indel_result &out) {
        if (!begun_) throw std::runtime_error("--vcf-indels: the calls before the references");
        begun_ = false;
        for (size_t r = 0; r + 1 < base_.size(); r++) {  // every record's +1 and -1 lie on one reference
            uint32_t run = 0;
            for (uint64_t p = base_[r]; p < base_[r + 1]; p++) cover_[p] = run += cover_[p];
        }
        std::sort(events_.begin(), events_.end());
        out.alleles.clear(), out.calls.clear();
        out.stats = stats_;
        out.n_events = events_.size();
        for (size_t j = 0; j < events_.size();) {
            size_t to = j;
            while (to < events_.size() && events_[to] == events_[j]) to++;
            const uint32_t slot = std::get<0>(events_[j]);
            const size_t ref = static_cast<size_t>(std::upper_bound(base_.begin(), base_.end(), uint64_t{slot}) - base_.begin()) - 1;
            const uint64_t seq = std::get<2>(events_[j]);
            const uint32_t words[kIndelAlleleWords] = {static_cast<uint32_t>(ref), static_cast<uint32_t>(slot - base_[ref]), std::get<1>(events_[j]),
                                                       static_cast<uint32_t>(seq), static_cast<uint32_t>(seq >> 32), static_cast<uint32_t>(to - j), 0, 0};
            out.alleles.insert(out.alleles.end(), words, words + kIndelAlleleWords);
            j = to;
        }
        const size_t na = out.n_alleles();
        for (size_t a = 0; a < na;) {
            const uint32_t *x = out.alleles.data() + kIndelAlleleWords * a;
            size_t to = a;
            while (to < na && out.alleles[kIndelAlleleWords * to] == x[0] && out.alleles[kIndelAlleleWords * to + 1] == x[1]) to++;
            uint32_t call[kIndelCallWords];
            if (call_anchor(x, to - a, cover_[base_[x[0]] + x[1]], pr_, call)) out.calls.insert(out.calls.end(), call, call + kIndelCallWords);
            a = to;
        }
    }

    // cover at every position, the references back to back (after finish)
    const std::vector<uint32_t> &cover() const { return cover_; }
};

struct indel_summary {
    uint64_t variants = 0, het = 0, hom = 0, low_qual = 0, sites = 0, events = 0, other = 0;
};

// min_qual in phred: a variant call of qual < 100 min_qual is LowQual
inline indel_summary summarize_indels(const indel_result &res, uint32_t min_qual) {
    indel_summary s;
    s.sites = res.n_calls(), s.events = res.n_events;
    for (size_t a = 0; a < res.n_alleles(); a++)
        if (res.alleles[kIndelAlleleWords * a + 2] & kIndelOther) s.other += res.alleles[kIndelAlleleWords * a + 5];
    for (size_t k = 0; k < res.n_calls(); k++) {
        const uint32_t *c = res.calls.data() + kIndelCallWords * k;
        if (!(c[5] & kIndelVariant)) continue;
        s.variants++;
        (c[6] == 1 ? s.het : s.hom)++;
        if (c[8] < static_cast<uint64_t>(100) * min_qual) s.low_qual++;
    }
    return s;
}

inline std::string indel_summary_line(const indel_summary &s) {
    return "Indels: " + std::to_string(s.variants) + " variants (" + std::to_string(s.het) + " het, " + std::to_string(s.hom) + " hom, " +
           std::to_string(s.low_qual) + " below QUAL) at " + std::to_string(s.sites) + " sites from " + std::to_string(s.events) + " events (" +
           std::to_string(s.other) + " other)";
}

inline const char *indel_vcf_header() {
    return "##INFO=<ID=INDEL,Number=0,Type=Flag,Description=\"An insertion or deletion behind POS, from the CIGARs of the records\">\n";
}

// the tools' convention for a reference letter: upper case, and what is not A C G T reads as A
inline char indel_ref_letter(char b) {
    const char u = static_cast<char>(b & 0xDF);
    return u == 'A' || u == 'C' || u == 'G' || u == 'T' ? u : 'A';
}

// The VCF line of a VARIANT call appended to buf: POS is the anchor + 1, REF the anchor base (and the deleted bases), ALT the
// anchor base (and the inserted bases); QUAL, FILTER and the sample column as for SNVs (host/genotype.h).  ref_bases are the
// bases of the call's reference.
inline void append_indel_vcf_line(std::string &buf, const uint32_t *c, const std::string &ref_id, const std::string &ref_bases, uint32_t min_qual) {
    const uint32_t anchor = c[1], w1 = c[2], len = w1 & kIndelLenMask;
    if (anchor >= ref_bases.size() || (!(w1 & kIndelIns) && static_cast<uint64_t>(anchor) + len >= ref_bases.size()))
        throw std::runtime_error("--vcf-indels: a call beyond the end of " + ref_id);
    std::string ref(1, indel_ref_letter(ref_bases[anchor])), alt = ref;
    if (w1 & kIndelIns) {
        const uint64_t seq = static_cast<uint64_t>(c[3]) | static_cast<uint64_t>(c[4]) << 32;
        for (uint32_t j = 0; j < len; j++) alt += "ACGT"[(seq >> (2 * j)) & 3];
    } else
        for (uint32_t j = 1; j <= len; j++) ref += indel_ref_letter(ref_bases[anchor + j]);
    char qual[32];
    std::snprintf(qual, sizeof qual, "%u.%02u", c[8] / 100, c[8] % 100);
    buf += ref_id;
    buf += '\t', buf += std::to_string(static_cast<uint64_t>(anchor) + 1);
    buf += "\t.\t" + ref + "\t" + alt + "\t" + qual;
    buf += c[8] >= static_cast<uint64_t>(100) * min_qual ? "\tPASS" : "\tLowQual";
    buf += "\tINDEL;DP=" + std::to_string(c[12]) + "\tGT:DP:AD:GQ:PL\t";
    buf += c[6] == 1 ? "0/1:" : "1/1:";
    buf += std::to_string(c[12]) + ":" + std::to_string(c[9]) + "," + std::to_string(c[10]) + ":" + std::to_string(c[7]) + ":";
    buf += std::to_string(c[13] / 100) + "," + std::to_string(c[14] / 100) + "," + std::to_string(c[15] / 100) + "\n";
}

}  // namespace bm
