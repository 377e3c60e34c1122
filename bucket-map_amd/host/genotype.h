// genotype.h -- the genotype rule of include/bmg.h as plain C++17: what bmg_begin / bmg_add / bmg_call compute on the device,
// value for value, and the VCF file of --vcf.
//
// The rule (the five parameters, the four cells n << 32 | Q per position, the ten costs, the call's 24 words and what is left
// out) is stated in include/bmg.h; the counted records and the walk are those of include/bmp.h (host/pileup.h).
// tests/genotype_rule.py restates it a third time in Python.  This copy is the caller of every build without a device behind
// it (block_compressor's defaults in bgzf.h, so the oracle-backed test tools) and the reference the device is compared with.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "bias.h"
#include "phase.h"

namespace bm {

constexpr size_t kGenotypeCells = 4;        // BMG_N_CELLS: A C G T
constexpr size_t kGenotypeSiteWords = 12;   // BMG_SITE_WORDS: a site of the pileup
constexpr size_t kGenotypeCallWords = 24;   // BMG_CALL_WORDS
constexpr uint32_t kGenotyped = 1, kVariant = 2;   // the flags of a call

struct genotype_params {                    // the order of bmg_begin's params; the defaults are the command line's
    uint32_t min_mapq = 0, min_bq = 13, q_absent = 30, q_cap = 60, prior = 3000;
};

class genotype_counter {
    std::vector<uint32_t> ref_len_;
    std::vector<uint64_t> base_;    // reference r: positions base_[r] .. base_[r + 1] - 1
    std::vector<uint64_t> cell_;    // kGenotypeCells per position
    genotype_params pr_;
    bool begun_ = false;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);   // little-endian hosts only, like the rest of the tool
        return v;
    }
    static uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }
    static uint32_t sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(v); }

public:
    void begin(const uint32_t *ref_len, size_t n_ref, const genotype_params &pr) {
        if (n_ref == 0) throw std::runtime_error("--vcf: no reference");
        uint64_t bases = 0;
        for (size_t r = 0; r < n_ref; r++) {
            if (ref_len[r] == 0) throw std::runtime_error("--vcf: reference " + std::to_string(r) + " has the length 0");
            bases += ref_len[r];
        }
        if (bases > (uint64_t{1} << 32) - (uint64_t{1} << 20) || bases + n_ref > 0xFFFFFFFEull)
            throw std::runtime_error("--vcf: " + std::to_string(bases) + " bases, at most 2^32 - 2^20 are counted in one go");
        if (pr.q_cap == 0 || pr.q_cap > 93) throw std::runtime_error("--vcf: q_cap is " + std::to_string(pr.q_cap) + ", not 1 .. 93");
        if (pr.q_absent > pr.q_cap) throw std::runtime_error("--vcf: q_absent " + std::to_string(pr.q_absent) + " is above q_cap");
        pr_ = pr;
        ref_len_.assign(ref_len, ref_len + n_ref);
        base_.assign(n_ref + 1, 0);
        for (size_t r = 0; r < n_ref; r++) base_[r + 1] = base_[r] + ref_len[r];
        cell_.assign(base_[n_ref] * kGenotypeCells, 0);
        begun_ = true;
    }

    // whole records in[rec_offset[i], rec_offset[i + 1]); skip may be null
    void add(const uint8_t *in, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        if (!begun_) throw std::runtime_error("--vcf: records before the references");
        // the checks first: a refused call changes nothing
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const uint64_t length = rec_offset[i + 1] - rec_offset[i];
            if (length < 36) throw std::runtime_error("--vcf: a record of " + std::to_string(length) + " bytes");
            const int32_t ref = static_cast<int32_t>(u32(r + 4));
            const uint32_t l_name = r[12], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if (36ull + l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2 + l_seq > length)
                throw std::runtime_error("--vcf: a record's fields lie beyond its end");
            uint64_t query = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = u32(r + 36 + l_name + 4ull * k), op = c & 15u;
                if (op > 8) throw std::runtime_error("--vcf: a CIGAR op with the code " + std::to_string(op));
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
            }
            if (n_cigar && l_seq && query != l_seq)
                throw std::runtime_error("--vcf: a CIGAR of " + std::to_string(query) + " query bases on a record of " + std::to_string(l_seq));
            if (ref >= 0 && static_cast<size_t>(ref) >= ref_len_.size() && !(flag & 4u))
                throw std::runtime_error("--vcf: a record names reference " + std::to_string(ref) + ", there are " + std::to_string(ref_len_.size()));
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
            uint64_t *c = cell_.data() + base_[ref] * kGenotypeCells;
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
                        const uint32_t q_eff = q == 0xFF ? pr_.q_absent : std::min(q, pr_.q_cap);
                        c[(rc + j) * kGenotypeCells + letter] += (uint64_t{1} << 32) + q_eff;
                    }
                }
                if (block || op == 2 || op == 3) rc += len;
                if (block || op == 1 || op == 4) qc += len;
            }
        }
    }

    // the calls of the n_sites sites (kGenotypeSiteWords each, in any order) from everything added so far: out receives
    // kGenotypeCallWords per site
    void call(const uint32_t *sites, size_t n_sites, std::vector<uint32_t> &out) const {
        if (!begun_) throw std::runtime_error("--vcf: calls before the references");
        for (size_t i = 0; i < n_sites; i++) {
            const uint32_t ref = sites[kGenotypeSiteWords * i], pos = sites[kGenotypeSiteWords * i + 1];
            if (ref >= ref_len_.size() || pos >= ref_len_[ref])
                throw std::runtime_error("--vcf: a site at base " + std::to_string(pos) + " of reference " + std::to_string(ref));
        }
        out.assign(n_sites * kGenotypeCallWords, 0);
        for (size_t i = 0; i < n_sites; i++) {
            const uint32_t *s = sites + kGenotypeSiteWords * i;
            uint32_t *o = out.data() + kGenotypeCallWords * i;
            const uint32_t R = s[2];
            const uint64_t *c = cell_.data() + (base_[s[0]] + s[1]) * kGenotypeCells;
            uint64_t n[4], M[4], T[4], all = 0, depth = 0;
            for (size_t a = 0; a < 4; a++) {
                n[a] = c[a] >> 32;
                const uint64_t Q = c[a] & 0xFFFFFFFFull;
                M[a] = 100 * Q + 477 * n[a];
                T[a] = 301 * n[a];
                all += M[a];
                depth += n[a];
                o[8 + a] = static_cast<uint32_t>(n[a]);
            }
            o[0] = s[0], o[1] = s[1], o[2] = R;
            if (!(s[11] & 1u) || R > 3 || depth == 0) continue;
            uint64_t L[10];
            uint32_t letters[10][2], k = 0, best = 0, k_rr = 0;
            for (uint32_t b = 0; b < 4; b++)
                for (uint32_t a = 0; a <= b; a++, k++) {
                    const uint64_t like = a == b ? all - M[a] : T[a] + T[b] + all - M[a] - M[b];
                    const uint32_t others = (a != R ? 1u : 0u) + (b != R && b != a ? 1u : 0u);
                    L[k] = like + static_cast<uint64_t>(pr_.prior) * others;
                    letters[k][0] = a, letters[k][1] = b;
                    if (a == R && b == R) k_rr = k;
                    if (L[k] < L[best]) best = k;        // the smallest k among equals
                }
            if (L[k_rr] == L[best]) best = k_rr;         // a tie goes to RR
            uint64_t second = ~uint64_t{0};
            for (uint32_t g = 0; g < 10; g++)
                if (g != best) second = std::min(second, L[g]);
            o[3] = kGenotyped | (best != k_rr ? kVariant : 0u);
            o[4] = letters[best][0], o[5] = letters[best][1];
            o[6] = static_cast<uint32_t>(std::min<uint64_t>(99, (second - L[best]) / 100));
            o[7] = sat32(L[k_rr] - L[best]);
            for (uint32_t g = 0; g < 10; g++) o[12 + g] = sat32(L[g] - L[best]);
            o[22] = sat32(depth);
        }
    }

    // every position's four cells, the references back to back
    const std::vector<uint64_t> &cells() const { return cell_; }
};

struct genotype_result {
    std::vector<uint32_t> calls;    // kGenotypeCallWords per site of the pileup, in its order
    uint64_t n_snv_sites = 0;       // the sites with the SNV kind bit
    size_t n_calls() const { return calls.size() / kGenotypeCallWords; }
};

struct genotype_summary {
    uint64_t variants = 0, het = 0, hom = 0, low_qual = 0;
};

// min_qual in phred: a variant call of qual < 100 min_qual is LowQual
inline genotype_summary summarize_genotypes(const genotype_result &res, uint32_t min_qual) {
    genotype_summary s;
    for (size_t k = 0; k < res.n_calls(); k++) {
        const uint32_t *c = res.calls.data() + kGenotypeCallWords * k;
        if (!(c[3] & kVariant)) continue;
        s.variants++;
        (c[4] != c[5] ? s.het : s.hom)++;
        if (c[7] < static_cast<uint64_t>(100) * min_qual) s.low_qual++;
    }
    return s;
}

// what --vcf-indels puts between the SNV lines: called before the line at (reference, POS) and, with (2^32 - 1, 2^64 - 1), after
// the last one; it appends the lines that belong before that place to buf
using vcf_between = std::function<void(std::string &buf, uint32_t ref, uint64_t pos)>;

// --vcf FILE: VCF 4.2, the header, then one line per VARIANT call in the order of the calls.  more_info, where given, is a
// further INFO line of the header.  bias, where given (--vcf-bias, host/bias.h), holds one annotation per call: the header gains
// six lines, a line FS and MQ in INFO, ADF and ADR after AD, and the filters StrandBias and LowMQ.  phase, where given
// (--vcf-phase, host/phase.h), knows the phase sites: the header gains FORMAT=PS after PL, and the line of a PHASED call reads
// g(haplotype 1)|g(haplotype 2) and ends its keys with :PS and its sample column with the 1-based POS of the block's root; every
// other line is the line without it.
inline void write_vcf_file(std::ostream &out, const genotype_result &res, const std::vector<std::string> &ref_ids, const std::vector<uint32_t> &ref_len,
                           const std::string &sample, uint32_t min_qual, const char *more_info = nullptr, const vcf_between *between = nullptr,
                           const char *const *gvcf = nullptr, const vcf_bias *bias = nullptr, const vcf_phase *phase = nullptr) {
    // gvcf, where given, makes it the header of --gvcf: three more lines, one for ALT, one for INFO and one for FORMAT
    std::string buf = gvcf ? "##fileformat=VCFv4.2\n##source=bucketmap --gvcf\n" : "##fileformat=VCFv4.2\n##source=bucketmap --vcf\n";
    for (size_t r = 0; r < ref_ids.size(); r++) buf += "##contig=<ID=" + ref_ids[r] + ",length=" + std::to_string(ref_len.at(r)) + ">\n";
    if (gvcf) buf += gvcf[0];
    buf += "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Counted bases A, C, G and T of sufficient base quality\">\n";
    if (more_info) buf += more_info;
    if (gvcf) buf += gvcf[1];
    if (bias) buf += bias_info_lines();
    buf += "##FILTER=<ID=LowQual,Description=\"QUAL below " + std::to_string(min_qual) + "\">\n";
    if (bias) buf += bias_filter_lines(*bias);
    buf += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n";
    buf += "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Counted bases A, C, G and T of sufficient base quality\">\n";
    buf += "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Counted bases of the reference and of each alternative allele\">\n";
    if (bias) buf += bias_format_lines();
    buf += "##FORMAT=<ID=GQ,Number=1,Type=Integer,Description=\"Genotype quality: the cost of the second-best genotype, at most 99\">\n";
    buf += "##FORMAT=<ID=PL,Number=G,Type=Integer,Description=\"Phred-scaled genotype costs with the prior, the best at 0\">\n";
    if (phase) buf += phase_format_line();
    if (gvcf) buf += gvcf[2];
    buf += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample + "\n";
    for (size_t k = 0; k < res.n_calls(); k++) {
        const uint32_t *c = res.calls.data() + kGenotypeCallWords * k;
        if (!(c[3] & kVariant)) continue;
        const uint32_t R = c[2];
        uint32_t allele[3] = {R, 0, 0}, n_alleles = 1;   // R, then the letters of g* other than R in A C G T order
        if (c[4] != R) allele[n_alleles++] = c[4];
        if (c[5] != R && c[5] != c[4]) allele[n_alleles++] = c[5];
        auto number_of = [&](uint32_t letter) {
            for (uint32_t j = 0; j < n_alleles; j++)
                if (allele[j] == letter) return j;
            return 0u;
        };
        char qual[32];
        std::snprintf(qual, sizeof qual, "%u.%02u", c[7] / 100, c[7] % 100);
        if (between) (*between)(buf, c[0], static_cast<uint64_t>(c[1]) + 1);
        buf += ref_ids.at(c[0]);
        buf += '\t', buf += std::to_string(static_cast<uint64_t>(c[1]) + 1);
        buf += "\t.\t", buf += "ACGT"[R];
        buf += '\t';
        for (uint32_t j = 1; j < n_alleles; j++) buf += j > 1 ? "," : "", buf += "ACGT"[allele[j]];
        buf += '\t', buf += qual;
        const uint32_t *note = bias ? bias->at(k) : nullptr;
        std::string filters = c[7] >= static_cast<uint64_t>(100) * min_qual ? "" : "LowQual";
        if (note && bias->strand_bias(note)) filters += filters.empty() ? "StrandBias" : ";StrandBias";
        if (note && bias->low_mq(note)) filters += filters.empty() ? "LowMQ" : ";LowMQ";
        buf += '\t', buf += filters.empty() ? "PASS" : filters;
        buf += "\tDP=" + std::to_string(c[22]);
        if (note) buf += bias_info(note);
        const uint32_t *linked = phase ? phase->phased(k) : nullptr;
        buf += note ? "\tGT:DP:AD:ADF:ADR:GQ:PL" : "\tGT:DP:AD:GQ:PL";
        buf += linked ? ":PS\t" : "\t";
        const uint32_t g0 = number_of(c[4]), g1 = number_of(c[5]);
        if (linked)                                      // haplotype 1 carries allele hap of the site: the call's first letter at hap 0
            buf += std::to_string(linked[kPhaseWHap] ? g1 : g0) + "|" + std::to_string(linked[kPhaseWHap] ? g0 : g1) + ":" + std::to_string(c[22]) + ":";
        else
            buf += std::to_string(std::min(g0, g1)) + "/" + std::to_string(std::max(g0, g1)) + ":" + std::to_string(c[22]) + ":";
        for (uint32_t j = 0; j < n_alleles; j++) buf += j ? "," : "", buf += std::to_string(c[8 + allele[j]]);
        if (note)
            for (size_t w : {kBiasWFwd, kBiasWRev}) {
                buf += ':';
                for (uint32_t j = 0; j < n_alleles; j++) buf += j ? "," : "", buf += std::to_string(note[w + allele[j]]);
            }
        buf += ":" + std::to_string(c[6]) + ":";
        for (uint32_t hi = 0; hi < n_alleles; hi++)      // VCF order: the genotype j/hi at hi (hi + 1) / 2 + j
            for (uint32_t lo = 0; lo <= hi; lo++) {
                const uint32_t a = std::min(allele[lo], allele[hi]), b = std::max(allele[lo], allele[hi]);
                buf += hi ? "," : "", buf += std::to_string(c[12 + b * (b + 1) / 2 + a] / 100);
            }
        if (linked) buf += ":" + std::to_string(static_cast<uint64_t>(linked[kPhaseWRootPos]) + 1);
        buf += '\n';
        if (buf.size() > (1u << 20)) out.write(buf.data(), static_cast<std::streamsize>(buf.size())), buf.clear();
    }
    if (between) (*between)(buf, 0xFFFFFFFFu, ~uint64_t{0});
    out.write(buf.data(), static_cast<std::streamsize>(buf.size()));
}

}  // namespace bm
