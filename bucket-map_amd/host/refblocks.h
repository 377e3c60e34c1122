// refblocks.h -- the reference-block rule of include/bmr.h as plain C++17 over genotype_counter::cells(): what bmr_run computes
// on the device, value for value, and the gVCF file and the summary line of --gvcf.
//
// The rule (gq without the prior, the bands, IN / EXCLUDED / NO_ALLELE, the eight words of a block, the two words of the
// per-position view and what is left out) is stated in include/bmr.h; tests/refblocks_rule.py restates it a third time in
// Python.  This copy is the path of every build without a device behind it (block_compressor's default in bgzf.h, so the
// oracle-backed test tools) and the reference the device is compared with.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "genotype.h"
#include "indel.h"

namespace bm {

constexpr size_t kRefBlockWords = 8;        // BMR_BLOCK_WORDS
constexpr size_t kRefBlockMaxBands = 16;    // BMR_MAX_BANDS
constexpr uint32_t kRefBlockIn = 1u << 16, kRefBlockExcluded = 1u << 17, kRefBlockNoAllele = 1u << 18;

struct refblock_result {
    std::vector<uint32_t> blocks;           // kRefBlockWords each, in (reference, start) order
    uint64_t n_excluded = 0, n_no_allele = 0;   // positions under an excluded interval / with R = 4 and not excluded
    size_t n_blocks() const { return blocks.size() / kRefBlockWords; }
};

inline uint32_t refblock_letter(uint8_t b) {
    const uint8_t u = b & 0xDF;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// what bmr_run refuses, in its words
inline void refblock_check(const std::vector<uint32_t> &ref_len, const std::vector<uint32_t> &bands, const std::vector<uint32_t> &exclude) {
    if (bands.size() > kRefBlockMaxBands) throw std::runtime_error("--gvcf: " + std::to_string(bands.size()) + " band bounds, at most 16");
    for (size_t k = 0; k < bands.size(); k++) {
        if (bands[k] == 0 || bands[k] > 99) throw std::runtime_error("--gvcf: band bound " + std::to_string(bands[k]) + ", a bound is 1 .. 99");
        if (k && bands[k] <= bands[k - 1]) throw std::runtime_error("--gvcf: band bound " + std::to_string(bands[k]) + " is not above its predecessor");
    }
    if (exclude.size() % 3) throw std::runtime_error("--gvcf: an excluded interval is three numbers");
    for (size_t i = 0; i < exclude.size(); i += 3)
        if (exclude[i] >= ref_len.size() || exclude[i + 1] >= exclude[i + 2] || exclude[i + 2] > ref_len[exclude[i]])
            throw std::runtime_error("--gvcf: an excluded interval " + std::to_string(exclude[i + 1]) + " .. " + std::to_string(exclude[i + 2]) +
                                     " of reference " + std::to_string(exclude[i]));
}

// n_excluded and n_no_allele of res from its blocks: the intervals' union, and what neither they nor the blocks hold
inline void refblock_count_rest(refblock_result &res, const std::vector<uint32_t> &ref_len, const std::vector<uint32_t> &exclude) {
    std::vector<std::pair<uint64_t, uint64_t>> spans;    // (reference << 32 | start, reference << 32 | end)
    for (size_t i = 0; i < exclude.size(); i += 3)
        spans.emplace_back(static_cast<uint64_t>(exclude[i]) << 32 | exclude[i + 1], static_cast<uint64_t>(exclude[i]) << 32 | exclude[i + 2]);
    std::sort(spans.begin(), spans.end());
    uint64_t under = 0, reached = 0;
    for (const auto &sp : spans) {
        const uint64_t from = std::max(sp.first, reached);
        if (sp.second > from) under += sp.second - from, reached = sp.second;
    }
    uint64_t bases = 0, on = 0;
    for (uint32_t l : ref_len) bases += l;
    for (size_t k = 0; k < res.n_blocks(); k++) on += res.blocks[kRefBlockWords * k + 2] - res.blocks[kRefBlockWords * k + 1];
    res.n_excluded = under;
    res.n_no_allele = bases - on - under;
}

// gq of one position from its four cells and the reference allele R <= 3: the costs of bmg.h without the prior
inline uint32_t refblock_gq(const uint64_t *c, uint32_t R) {
    uint64_t M[4], T[4], all = 0;
    for (size_t a = 0; a < 4; a++) {
        const uint64_t n = c[a] >> 32, Q = c[a] & 0xFFFFFFFFull;
        M[a] = 100 * Q + 477 * n;
        T[a] = 301 * n;
        all += M[a];
    }
    uint64_t l_rr = 0, h = ~uint64_t{0};
    for (uint32_t b = 0; b < 4; b++)
        for (uint32_t a = 0; a <= b; a++) {
            const uint64_t like = a == b ? all - M[a] : T[a] + T[b] + all - M[a] - M[b];
            if (a == R && b == R) l_rr = like;
            else h = std::min(h, like);
        }
    return l_rr <= h ? static_cast<uint32_t>(std::min<uint64_t>(99, (h - l_rr) / 100)) : 0u;
}

// The per-position view (conf: two words per position, the references back to back; may be null) and the blocks of the cells
// (four per position, the references back to back).  exclude holds three words per interval.
inline void refblocks_of(const std::vector<uint64_t> &cells, const std::vector<uint32_t> &ref_len, const uint8_t *const *ref_bases,
                         const std::vector<uint32_t> &bands, const std::vector<uint32_t> &exclude, refblock_result &out, std::vector<uint32_t> *conf = nullptr) {
    refblock_check(ref_len, bands, exclude);
    uint64_t total = 0;
    for (uint32_t l : ref_len) total += l;
    if (cells.size() != total * kGenotypeCells) throw std::runtime_error("--gvcf: " + std::to_string(cells.size()) + " cells for " + std::to_string(total) + " bases");
    std::vector<uint64_t> first(ref_len.size() + 1, 0);
    for (size_t r = 0; r < ref_len.size(); r++) first[r + 1] = first[r] + ref_len[r];
    std::vector<uint8_t> excluded(total, 0);
    for (size_t i = 0; i < exclude.size(); i += 3) std::fill(excluded.begin() + first[exclude[i]] + exclude[i + 1], excluded.begin() + first[exclude[i]] + exclude[i + 2], 1);
    out.blocks.clear();
    if (conf) conf->assign(2 * total, 0);
    for (size_t r = 0; r < ref_len.size(); r++) {
        bool open = false;
        uint32_t cur[kRefBlockWords] = {};
        uint64_t sum = 0;
        auto close = [&](uint32_t end) {
            if (!open) return;
            cur[2] = end, cur[6] = static_cast<uint32_t>(sum), cur[7] = static_cast<uint32_t>(sum >> 32);
            out.blocks.insert(out.blocks.end(), cur, cur + kRefBlockWords);
            open = false;
        };
        for (uint32_t p = 0; p < ref_len[r]; p++) {
            const uint64_t *c = cells.data() + (first[r] + p) * kGenotypeCells;
            const uint64_t depth = (c[0] >> 32) + (c[1] >> 32) + (c[2] >> 32) + (c[3] >> 32);
            const uint32_t dp = depth > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(depth);
            const uint32_t R = refblock_letter(ref_bases[r][p]);
            uint32_t word = 0;
            if (excluded[first[r] + p]) word = kRefBlockExcluded;
            else if (R > 3) word = kRefBlockNoAllele;
            else {
                const uint32_t gq = refblock_gq(c, R);
                uint32_t band = 0;
                for (uint32_t bound : bands) band += bound <= gq;
                word = gq | band << 8 | kRefBlockIn;
                if (open && cur[3] != band) close(p);
                if (!open) {
                    open = true, sum = 0;
                    cur[0] = static_cast<uint32_t>(r), cur[1] = p, cur[3] = band, cur[4] = gq, cur[5] = dp;
                }
                cur[4] = std::min(cur[4], gq), cur[5] = std::min(cur[5], dp), sum += dp;
            }
            if (!(word & kRefBlockIn)) close(p);
            if (conf) (*conf)[2 * (first[r] + p)] = word, (*conf)[2 * (first[r] + p) + 1] = dp;
        }
        close(ref_len[r]);
    }
    refblock_count_rest(out, ref_len, exclude);
}

// The intervals no block may claim: the position of every SNV call that is written as a line, the anchor of every indel call
// that is written as a line and the deleted bases of a written deletion, clipped to the reference.  indel_calls may be null.
inline std::vector<uint32_t> refblock_excluded(const genotype_result &res, const std::vector<uint32_t> *indel_calls, const std::vector<uint32_t> &ref_len) {
    std::vector<uint32_t> ex;
    for (size_t k = 0; k < res.n_calls(); k++) {
        const uint32_t *c = res.calls.data() + kGenotypeCallWords * k;
        if (c[3] & kVariant) ex.insert(ex.end(), {c[0], c[1], c[1] + 1});
    }
    if (indel_calls)
        for (size_t k = 0; k + kIndelCallWords <= indel_calls->size(); k += kIndelCallWords) {
            const uint32_t *c = indel_calls->data() + k;
            if (!(c[5] & kIndelVariant)) continue;
            ex.insert(ex.end(), {c[0], c[1], c[1] + 1});
            const uint64_t end = std::min<uint64_t>(static_cast<uint64_t>(c[1]) + 1 + (c[2] & kIndelLenMask), ref_len.at(c[0]));
            if (!(c[2] & kIndelIns) && end > static_cast<uint64_t>(c[1]) + 1) ex.insert(ex.end(), {c[0], c[1] + 1, static_cast<uint32_t>(end)});
        }
    return ex;
}

inline const char *gvcf_alt_header() { return "##ALT=<ID=NON_REF,Description=\"Any allele other than the reference's: a block of positions without a variant call\">\n"; }
inline const char *gvcf_info_header() { return "##INFO=<ID=END,Number=1,Type=Integer,Description=\"The last position of the block\">\n"; }
inline const char *gvcf_format_header() {
    return "##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description=\"The smallest DP in the block; DP is the mean and GQ the smallest GQ\">\n";
}

// the line of one block: POS is start + 1, END the last position, DP the mean depth rounded down
inline void append_block_line(std::string &buf, const uint32_t *b, const std::string &ref_id, const uint8_t *ref_bases) {
    const uint8_t u = ref_bases[b[1]] & 0xDF;
    const uint64_t sum = static_cast<uint64_t>(b[6]) | static_cast<uint64_t>(b[7]) << 32;
    buf += ref_id;
    buf += '\t', buf += std::to_string(static_cast<uint64_t>(b[1]) + 1);
    buf += "\t.\t", buf += u == 'A' || u == 'C' || u == 'G' || u == 'T' ? static_cast<char>(u) : 'A';
    buf += "\t<NON_REF>\t.\t.\tEND=" + std::to_string(b[2]) + "\tGT:DP:GQ:MIN_DP\t0/0:" + std::to_string(sum / (b[2] - b[1])) + ":" + std::to_string(b[4]) + ":" +
           std::to_string(b[5]) + "\n";
}

inline std::string refblock_summary_line(const refblock_result &res, const std::vector<uint32_t> &ref_len) {
    uint64_t bases = 0, on = 0, band0 = 0;
    for (uint32_t l : ref_len) bases += l;
    for (size_t k = 0; k < res.n_blocks(); k++) {
        const uint32_t *b = res.blocks.data() + kRefBlockWords * k;
        on += b[2] - b[1];
        if (b[3] == 0) band0 += b[2] - b[1];
    }
    return "Blocks: " + std::to_string(res.n_blocks()) + " blocks on " + std::to_string(on) + " of " + std::to_string(bases) + " bases (" +
           std::to_string(band0) + " in band 0, " + std::to_string(res.n_excluded) + " under variant lines, " + std::to_string(res.n_no_allele) +
           " without a reference allele)";
}

}  // namespace bm
