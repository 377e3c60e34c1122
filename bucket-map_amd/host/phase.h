// phase.h -- the read-backed phasing rule of include/bmk.h as plain C++17: what bmk_begin / bmk_add / bmk_finish compute on the
// device, value for value, and the text --vcf-phase adds to a het SNV line of the VCF.
//
// The rule (the five parameters, phase sites, observations, links, decisive links, parents, roots and haps, the eight words of
// a site and what is left out) is stated in include/bmk.h; the counted records and the walk are those of include/bmp.h.
// tests/phase_rule.py restates it a third time in Python.  This copy is the phaser of every build without a device behind it
// (block_compressor's defaults in bgzf.h, so the oracle-backed test tools) and the reference the device is compared with.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace bm {

constexpr size_t kPhaseCallWords = 24;      // BMK_CALL_WORDS: a call of the genotype caller
constexpr size_t kPhaseOutWords = 8;        // BMK_OUT_WORDS
constexpr size_t kPhaseStats = 4;           // BMK_N_STATS: H, phased sites, blocks of two sites or more, observations
constexpr uint32_t kPhaseMaxReach = 8;
constexpr uint32_t kPhasePhased = 1, kPhaseRoot = 2;
constexpr size_t kPhaseWCall = 0, kPhaseWRoot = 1, kPhaseWRootPos = 2, kPhaseWHap = 3, kPhaseWFlags = 4, kPhaseWD = 5, kPhaseWCis = 6, kPhaseWTrans = 7;

struct phase_params {                       // the order of bmk_begin's params; the defaults are the command line's
    uint32_t min_mapq = 0, min_bq = 13, min_links = 2, min_frac_ppm = 800000, reach = 4;
};

struct phase_result {
    std::vector<uint32_t> sites;            // kPhaseOutWords per phase site, in site order
    uint64_t stats[kPhaseStats] = {0, 0, 0, 0};
    size_t n_sites() const { return sites.size() / kPhaseOutWords; }
};

class phase_linker {
    struct site {
        uint32_t ref, pos, call, a0, a1;
    };
    std::vector<uint32_t> ref_len_;
    std::vector<uint64_t> base_;    // reference r: slots base_[r] .. base_[r + 1] - 1
    std::vector<uint64_t> slot_;    // ascending
    std::vector<site> site_;
    std::vector<uint32_t> link_;    // [site][reach][4]
    phase_params pr_;
    uint64_t observations_ = 0;
    bool begun_ = false, finished_ = false;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);   // little-endian hosts only, like the rest of the tool
        return v;
    }
    static uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }

public:
    // the phase sites among the calls (kPhaseCallWords each, ascending); returns H
    size_t begin(const uint32_t *ref_len, size_t n_ref, const phase_params &pr, const uint32_t *calls, size_t n_calls) {
        if (n_ref == 0) throw std::runtime_error("--vcf-phase: no reference");
        uint64_t bases = 0;
        for (size_t r = 0; r < n_ref; r++) {
            if (ref_len[r] == 0) throw std::runtime_error("--vcf-phase: reference " + std::to_string(r) + " has the length 0");
            bases += ref_len[r];
        }
        if (bases > (uint64_t{1} << 32) - (uint64_t{1} << 20) || bases + n_ref > 0xFFFFFFFEull)
            throw std::runtime_error("--vcf-phase: " + std::to_string(bases) + " bases, at most 2^32 - 2^20 in one go");
        if (pr.reach < 1 || pr.reach > kPhaseMaxReach) throw std::runtime_error("--vcf-phase: a reach of " + std::to_string(pr.reach) + ", it is 1 .. 8");
        if (pr.min_links == 0) throw std::runtime_error("--vcf-phase: min_links is 0");
        if (pr.min_frac_ppm < 500001 || pr.min_frac_ppm > 1000000) throw std::runtime_error("--vcf-phase: min_frac_ppm is " + std::to_string(pr.min_frac_ppm));
        std::vector<uint64_t> base(n_ref + 1, 0);
        for (size_t r = 0; r < n_ref; r++) base[r + 1] = base[r] + ref_len[r];
        std::vector<uint64_t> slot;
        std::vector<site> sites;
        for (size_t i = 0; i < n_calls; i++) {
            const uint32_t *c = calls + kPhaseCallWords * i;
            if (!(c[3] & 2u) || c[4] == c[5]) continue;
            if (c[0] >= n_ref || c[1] >= ref_len[c[0]] || c[4] > 3 || c[5] > 3)
                throw std::runtime_error("--vcf-phase: a call at base " + std::to_string(c[1]) + " of reference " + std::to_string(c[0]));
            const uint64_t at = base[c[0]] + c[1];
            if (!slot.empty() && at <= slot.back()) throw std::runtime_error("--vcf-phase: the calls do not ascend at call " + std::to_string(i));
            if (slot.size() == (uint64_t{1} << 31) - 1 || i > 0xFFFFFFFFull)   // this one would be the 2^31st: H is at most 2^31 - 1
                throw std::runtime_error("--vcf-phase: 2^31 phase sites or more");
            slot.push_back(at);
            sites.push_back(site{c[0], c[1], static_cast<uint32_t>(i), c[4], c[5]});
        }
        pr_ = pr;
        ref_len_.assign(ref_len, ref_len + n_ref);
        base_.swap(base), slot_.swap(slot), site_.swap(sites);
        link_.assign(slot_.size() * pr.reach * 4, 0);
        observations_ = 0;
        begun_ = true, finished_ = false;
        return slot_.size();
    }

    // whole records in[rec_offset[i], rec_offset[i + 1]); skip may be null
    void add(const uint8_t *in, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        if (!begun_ || finished_) throw std::runtime_error("--vcf-phase: records outside begin and finish");
        // the checks first: a refused call changes nothing
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const uint64_t length = rec_offset[i + 1] - rec_offset[i];
            if (length < 36) throw std::runtime_error("--vcf-phase: a record of " + std::to_string(length) + " bytes");
            const int32_t ref = static_cast<int32_t>(u32(r + 4));
            const uint32_t l_name = r[12], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if (36ull + l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2 + l_seq > length)
                throw std::runtime_error("--vcf-phase: a record's fields lie beyond its end");
            uint64_t query = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = u32(r + 36 + l_name + 4ull * k), op = c & 15u;
                if (op > 8) throw std::runtime_error("--vcf-phase: a CIGAR op with the code " + std::to_string(op));
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
            }
            if (n_cigar && l_seq && query != l_seq)
                throw std::runtime_error("--vcf-phase: a CIGAR of " + std::to_string(query) + " query bases on a record of " + std::to_string(l_seq));
            if (ref >= 0 && static_cast<size_t>(ref) >= ref_len_.size() && !(flag & 4u))
                throw std::runtime_error("--vcf-phase: a record names reference " + std::to_string(ref) + ", there are " + std::to_string(ref_len_.size()));
        }
        if (slot_.empty()) return;
        std::vector<std::pair<size_t, uint32_t>> seen;   // (site, allele) of one record, ascending
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const int32_t ref = static_cast<int32_t>(u32(r + 4)), pos = static_cast<int32_t>(u32(r + 8));
            const uint32_t l_name = r[12], mapq = r[13], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if ((flag & (0x4u | 0x100u | 0x200u | 0x400u)) || (skip && skip[i])) continue;
            if (ref < 0 || static_cast<size_t>(ref) >= ref_len_.size() || pos < 0 || static_cast<uint32_t>(pos) >= ref_len_[ref] || n_cigar == 0) continue;
            const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar, *qual = seq + (static_cast<uint64_t>(l_seq) + 1) / 2;
            if (l_seq == 0 || (n_cigar == 2 && u32(cigar) == (l_seq << 4 | 4u) && (u32(cigar + 4) & 15u) == 3)) continue;   // ... or the long-CIGAR placeholder
            if (mapq < pr_.min_mapq) continue;
            const uint64_t rlen = ref_len_[ref], base = base_[ref];
            size_t sc = static_cast<size_t>(std::lower_bound(slot_.begin(), slot_.end(), base + static_cast<uint64_t>(pos)) - slot_.begin());
            uint64_t rc = static_cast<uint64_t>(pos), qc = 0;
            seen.clear();
            for (uint32_t k = 0; k < n_cigar && rc < rlen && sc < slot_.size(); k++) {
                const uint32_t w = u32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
                const bool block = op == 0 || op == 7 || op == 8, takes_ref = block || op == 2 || op == 3;
                if (takes_ref && len) {
                    const uint64_t limit = base + std::min<uint64_t>(rc + len, rlen);
                    for (; sc < slot_.size() && slot_[sc] < limit; sc++) {
                        if (!block) continue;
                        const uint64_t at = qc + (slot_[sc] - base - rc);
                        const uint32_t q = qual[at], code = (seq[at >> 1] >> ((at & 1) ? 0 : 4)) & 15u;
                        if (q != 0xFF && q < pr_.min_bq) continue;
                        const uint32_t letter = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
                        if (letter == site_[sc].a0) seen.emplace_back(sc, 0u);
                        else if (letter == site_[sc].a1) seen.emplace_back(sc, 1u);
                    }
                }
                if (takes_ref) rc += len;
                if (block || op == 1 || op == 4) qc += len;
            }
            observations_ += seen.size();
            for (size_t y = 1; y < seen.size(); y++)
                for (size_t x = y; x-- > 0 && seen[y].first - seen[x].first <= pr_.reach;)
                    link_[(seen[x].first * pr_.reach + (seen[y].first - seen[x].first - 1)) * 4 + 2 * seen[x].second + seen[y].second]++;
        }
    }

    void finish(phase_result &out) {
        if (!begun_ || finished_) throw std::runtime_error("--vcf-phase: finish outside begin");
        finished_ = true;
        const size_t H = slot_.size();
        std::vector<size_t> parent(H);
        std::vector<uint32_t> flip(H, 0), d_of(H, 0), cis_of(H, 0), trans_of(H, 0);
        for (size_t j = 0; j < H; j++) {
            parent[j] = j;
            for (uint32_t d = 1; d <= pr_.reach && d <= j; d++) {
                const size_t i = j - d;
                if (site_[i].ref != site_[j].ref) break;
                const uint32_t *c = link_.data() + (i * pr_.reach + (d - 1)) * 4;
                const uint64_t cis = static_cast<uint64_t>(c[0]) + c[3], trans = static_cast<uint64_t>(c[1]) + c[2], big = std::max(cis, trans);
                if (big >= pr_.min_links && big * 1000000ull >= static_cast<uint64_t>(pr_.min_frac_ppm) * (cis + trans)) {
                    parent[j] = i, flip[j] = trans > cis, d_of[j] = d;
                    cis_of[j] = static_cast<uint32_t>(cis), trans_of[j] = static_cast<uint32_t>(trans);
                    break;
                }
            }
        }
        // a parent lies before its child: one pass in site order follows every path to its root
        std::vector<size_t> root(H), members(H, 0);
        std::vector<uint32_t> hap(H, 0);
        for (size_t j = 0; j < H; j++) {
            root[j] = parent[j] == j ? j : root[parent[j]];
            hap[j] = parent[j] == j ? 0u : hap[parent[j]] ^ flip[j];
            members[root[j]]++;
        }
        out.sites.assign(H * kPhaseOutWords, 0);
        out.stats[0] = H, out.stats[1] = out.stats[2] = 0, out.stats[3] = observations_;
        for (size_t j = 0; j < H; j++) {
            uint32_t *o = out.sites.data() + kPhaseOutWords * j;
            const bool phased = members[root[j]] >= 2, is_root = root[j] == j;
            o[kPhaseWCall] = site_[j].call, o[kPhaseWRoot] = static_cast<uint32_t>(root[j]), o[kPhaseWRootPos] = site_[root[j]].pos, o[kPhaseWHap] = hap[j];
            o[kPhaseWFlags] = (phased ? kPhasePhased : 0u) | (is_root ? kPhaseRoot : 0u);
            o[kPhaseWD] = d_of[j], o[kPhaseWCis] = cis_of[j], o[kPhaseWTrans] = trans_of[j];
            out.stats[1] += phased, out.stats[2] += phased && is_root;
        }
    }

    size_t n_sites() const { return slot_.size(); }
    const std::vector<uint32_t> &links() const { return link_; }
};

// what --vcf-phase hands to the writer of the VCF: per call the output words of its phase site, or null where it is none
struct vcf_phase {
    std::vector<uint32_t> sites;            // kPhaseOutWords per phase site
    std::vector<uint32_t> site_of_call;     // per call: its phase site + 1, 0 where it is none
    void index(size_t n_calls) {
        site_of_call.assign(n_calls, 0);
        for (size_t k = 0; k < sites.size() / kPhaseOutWords; k++) site_of_call.at(sites[kPhaseOutWords * k + kPhaseWCall]) = static_cast<uint32_t>(k + 1);
    }
    // the words of the call's phase site if it is PHASED, else null
    const uint32_t *phased(size_t call) const {
        if (call >= site_of_call.size() || site_of_call[call] == 0) return nullptr;
        const uint32_t *w = sites.data() + kPhaseOutWords * (site_of_call[call] - 1);
        return (w[kPhaseWFlags] & kPhasePhased) ? w : nullptr;
    }
};

struct phase_summary {
    uint64_t sites = 0, phased = 0, blocks = 0, longest = 0, observations = 0;
};

// calls: the calls the sites were chosen from (the position of a site is its call's)
inline phase_summary summarize_phase(const phase_result &res, const uint32_t *calls) {
    phase_summary s;
    s.sites = res.stats[0], s.phased = res.stats[1], s.blocks = res.stats[2], s.observations = res.stats[3];
    for (size_t k = 0; k < res.n_sites(); k++) {
        const uint32_t *w = res.sites.data() + kPhaseOutWords * k;
        if (!(w[kPhaseWFlags] & kPhasePhased)) continue;
        const uint64_t pos = calls[kPhaseCallWords * w[kPhaseWCall] + 1];
        s.longest = std::max<uint64_t>(s.longest, pos - w[kPhaseWRootPos] + 1);   // a root lies before its sites, on their reference
    }
    return s;
}

inline std::string phase_summary_line(const phase_summary &s) {
    return "Phase: " + std::to_string(s.phased) + " of " + std::to_string(s.sites) + " het SNVs phased in " + std::to_string(s.blocks) + " blocks (longest " +
           std::to_string(s.longest) + " bases, " + std::to_string(s.observations) + " observations)";
}

// the line --vcf-phase adds to the header, after FORMAT=PL
inline std::string phase_format_line() {
    return "##FORMAT=<ID=PS,Number=1,Type=Integer,Description=\"Phase set: POS of the first het SNV of the block of read-linked het SNVs this genotype is phased in\">\n";
}

}  // namespace bm
