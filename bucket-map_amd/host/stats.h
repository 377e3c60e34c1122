// stats.h -- the mapping statistics rule of include/bmq.h as plain C++17: what bmq_begin / bmq_add / bmq_finish count on the
// device, value for value, and the text file of --stats.
//
// The rule (the two parameters, the classes of a record, the 35 tallies, cycles, letters as sequenced, the eight tables and
// what is left out) is stated in include/bmq.h.  tests/stats_rule.py restates it a third time in Python.  This copy is the
// counter of every build without a device behind it (block_compressor's defaults in bgzf.h, so the oracle-backed test tools)
// and the reference the device is compared with.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace bm {

constexpr size_t kStatsTallies = 35;        // BMQ_N_TALLIES
constexpr size_t kStatsTables = 8;          // BMQ_N_TABLES: MAPQ RL IS GC ID BC QC MC
constexpr size_t kStatsWidth[kStatsTables] = {1, 1, 3, 1, 2, 5, 64, 6};
enum stats_table : size_t { kStatsMapq = 0, kStatsRl = 1, kStatsIs = 2, kStatsGc = 3, kStatsId = 4, kStatsBc = 5, kStatsQc = 6, kStatsMc = 7 };

struct stats_params {                       // the order of bmq_begin's params; the defaults are the command line's
    uint32_t max_cycle = 1024, max_insert = 8000;
};

inline size_t stats_rows(size_t table, const stats_params &pr) {
    const size_t rows[kStatsTables] = {256, size_t{pr.max_cycle} + 1, size_t{pr.max_insert} + 1, 101, 256, pr.max_cycle, pr.max_cycle, pr.max_cycle};
    return rows[table];
}

struct stats_result {
    stats_params params;
    uint64_t tallies[kStatsTallies] = {};
    std::vector<uint64_t> table[kStatsTables];   // row-major, stats_rows x kStatsWidth
};

class stats_counter {
    stats_result res_;
    bool begun_ = false, finished_ = false;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);   // little-endian hosts only, like the rest of the tool
        return v;
    }
    static uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }

public:
    void begin(const stats_params &pr) {
        if (pr.max_cycle < 1 || pr.max_cycle > 65535) throw std::runtime_error("--stats: max_cycle is " + std::to_string(pr.max_cycle) + ", it is 1 .. 65535");
        if (pr.max_insert < 1 || pr.max_insert > 65535) throw std::runtime_error("--stats: max_insert is " + std::to_string(pr.max_insert) + ", it is 1 .. 65535");
        res_ = stats_result{};
        res_.params = pr;
        for (size_t t = 0; t < kStatsTables; t++) res_.table[t].assign(stats_rows(t, pr) * kStatsWidth[t], 0);
        begun_ = true, finished_ = false;
    }

    // whole records in[rec_offset[i], rec_offset[i + 1]); skip may be null
    void add(const uint8_t *in, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        if (!begun_ || finished_) throw std::runtime_error("--stats: records outside begin and finish");
        // the checks first: a refused call changes nothing
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const uint64_t length = rec_offset[i + 1] - rec_offset[i];
            if (length < 36) throw std::runtime_error("--stats: a record of " + std::to_string(length) + " bytes");
            const uint32_t l_name = r[12], n_cigar = u16(r + 16), l_seq = u32(r + 20);
            if (36ull + l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2 + l_seq > length)
                throw std::runtime_error("--stats: a record's fields lie beyond its end");
            uint64_t query = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = u32(r + 36 + l_name + 4ull * k), op = c & 15u;
                if (op > 8) throw std::runtime_error("--stats: a CIGAR op with the code " + std::to_string(op));
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
            }
            if (n_cigar && l_seq && query != l_seq)
                throw std::runtime_error("--stats: a CIGAR of " + std::to_string(query) + " query bases on a record of " + std::to_string(l_seq));
        }
        const uint64_t C = res_.params.max_cycle, I = res_.params.max_insert;
        uint64_t *t = res_.tallies;
        for (size_t i = 0; i < n_records; i++) {
            if (skip && skip[i]) continue;
            const uint8_t *r = in + rec_offset[i];
            const int32_t ref = static_cast<int32_t>(u32(r + 4)), next_ref = static_cast<int32_t>(u32(r + 24)), tlen = static_cast<int32_t>(u32(r + 32));
            const uint32_t l_name = r[12], mapq = r[13], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            const uint8_t *cigar = r + 36 + l_name, *seq = cigar + 4ull * n_cigar, *qual = seq + (static_cast<uint64_t>(l_seq) + 1) / 2;
            const bool primary = !(flag & 0x900u), mapped = !(flag & 0x4u), paired = primary && (flag & 0x1u), reverse = flag & 0x10u;
            const bool placeholder = n_cigar == 2 && u32(cigar) == (l_seq << 4 | 4u) && (u32(cigar + 4) & 15u) == 3;
            const bool aligned = mapped && n_cigar > 0 && l_seq > 0 && !placeholder;
            const bool both = paired && mapped && !(flag & 0x8u), other_ref = both && next_ref != ref;
            t[0]++;
            t[1] += primary, t[2] += (flag & 0x100u) != 0, t[3] += (flag & 0x800u) != 0, t[4] += (flag & 0x400u) != 0, t[5] += (flag & 0x200u) != 0;
            t[6] += mapped, t[7] += primary && mapped, t[8] += paired, t[9] += paired && (flag & 0x40u), t[10] += paired && (flag & 0x80u);
            t[11] += paired && (flag & 0x2u) && mapped, t[12] += both, t[13] += paired && mapped && (flag & 0x8u);
            t[14] += other_ref, t[15] += other_ref && mapq >= 5, t[16] += mapped && reverse, t[17] += mapped && mapq == 0;
            if (primary) t[18] += l_seq;
            if (primary && mapped) t[19] += l_seq;
            t[20] += aligned, t[21] += mapped && placeholder;
            if (mapped) res_.table[kStatsMapq][mapq]++;
            if (primary) res_.table[kStatsRl][std::min<uint64_t>(l_seq, C)]++;
            if (both && next_ref == ref && tlen > 0) {
                const uint32_t way = flag & 0x30u;
                res_.table[kStatsIs][3 * std::min<uint64_t>(static_cast<uint64_t>(tlen), I) + (way == 0x20u ? 0 : way == 0x10u ? 1 : 2)]++;
                t[33]++;
            }
            auto cycle_of = [&](uint64_t j) { return reverse ? l_seq - 1 - j : j; };
            if (primary && l_seq > 0) {
                uint64_t n = 0, g = 0;
                for (uint64_t j = 0; j < l_seq; j++) {
                    const uint32_t code = (seq[j >> 1] >> ((j & 1) ? 0 : 4)) & 15u, q = qual[j];
                    const uint64_t c = cycle_of(j);
                    uint32_t letter = code == 1 ? 0u : code == 2 ? 1u : code == 4 ? 2u : code == 8 ? 3u : 4u;
                    if (letter < 4) n++, g += letter == 1 || letter == 2;
                    if (reverse && letter < 4) letter = 3 - letter;
                    if (c < C) res_.table[kStatsBc][5 * c + letter]++;
                    else t[32]++;
                    if (q != 0xFF) {
                        t[30] += q, t[31]++;
                        if (c < C) res_.table[kStatsQc][64 * c + std::min<uint32_t>(q, 63)]++;
                    }
                }
                if (n == 0) t[34]++;
                else res_.table[kStatsGc][(200 * g + n) / (2 * n)]++;
            }
            if (aligned) {
                uint64_t qc = 0;
                for (uint32_t k = 0; k < n_cigar; k++) {
                    const uint32_t w = u32(cigar + 4ull * k), op = w & 15u, len = w >> 4;
                    const int col = op == 7 ? 0 : op == 8 ? 1 : op == 0 ? 2 : op == 1 ? 3 : op == 4 ? 4 : -1;
                    if (col >= 0) {
                        for (uint64_t j = qc; j < qc + len; j++)
                            if (cycle_of(j) < C) res_.table[kStatsMc][6 * cycle_of(j) + col]++;
                        qc += len;
                    }
                    if (op == 0) t[22] += len;
                    if (op == 7) t[23] += len;
                    if (op == 8) t[24] += len;
                    if (op == 1) t[25] += len, t[28] += len > 0;
                    if (op == 2) t[26] += len, t[29] += len > 0;
                    if (op == 4) t[27] += len;
                    if ((op == 1 || op == 2) && len) res_.table[kStatsId][2 * std::min<uint32_t>(len, 255) + (op == 2)]++;
                    if (op == 2 && len && qc > 0 && cycle_of(qc - 1) < C) res_.table[kStatsMc][6 * cycle_of(qc - 1) + 5]++;
                }
            }
        }
    }

    void finish(stats_result &out) {
        if (!begun_ || finished_) throw std::runtime_error("--stats: finish outside begin");
        finished_ = true;
        out = res_;
    }
};

inline const char *const *stats_tally_names() {
    static const char *const names[kStatsTallies] = {
        "records", "primary", "secondary", "supplementary", "duplicates", "qc_failed", "mapped", "primary_mapped", "paired", "read1", "read2",
        "properly_paired", "both_mapped", "singletons", "mate_other_ref", "mate_other_ref_mapq5", "reverse_strand", "mapq0", "bases", "bases_mapped",
        "aligned_records", "left_out", "bases_m", "bases_eq", "bases_x", "inserted_bases", "deleted_bases", "soft_clipped_bases", "insertions",
        "deletions", "qual_sum", "qual_bases", "bases_beyond_cycle", "pairs_in_is", "reads_no_acgt"};
    return names;
}

// The file of --stats: tab-separated text.  Line 1 names the format; then SN lines of the tallies and four derived numbers
// (integer divisions, `.` where the divisor is 0); then the sections, each led by a `#` line that names its columns.  MAPQ, RL,
// GCF, ID and IS hold the rows with a non-zero cell; BCC, QCC and MCC the cycles 1 .. the last one with a non-zero cell of that
// table; QCC the columns 0 .. the largest quality seen.
inline void write_stats_file(std::ostream &f, const stats_result &res) {
    const uint64_t *t = res.tallies;
    std::string s = "# bucketmap --stats 1\n";
    for (size_t k = 0; k < kStatsTallies; k++) s += std::string("SN\t") + stats_tally_names()[k] + "\t" + std::to_string(t[k]) + "\n";
    auto derived = [&](const char *name, uint64_t num, uint64_t den) { s += std::string("SN\t") + name + "\t" + (den ? std::to_string(num / den) : std::string(".")) + "\n"; };
    derived("error_rate_ppm", t[24] * 1000000ull, t[23] + t[24]);
    derived("mean_quality_centi", t[30] * 100ull, t[31]);
    derived("mean_length_centi", t[18] * 100ull, t[1]);
    {
        const std::vector<uint64_t> &is = res.table[kStatsIs];
        const uint64_t I = res.params.max_insert;
        uint64_t total = 0, upto = 0, median = 0;
        for (uint64_t r = 0; r < I; r++) total += is[3 * r];
        for (uint64_t r = 0; r < I && total; r++) {
            upto += is[3 * r];
            if (2 * upto >= total) {
                median = r;
                break;
            }
        }
        derived("insert_size_median", median, total ? 1 : 0);
    }
    auto sparse = [&](const char *name, const char *head, size_t table) {
        const size_t w = kStatsWidth[table];
        const std::vector<uint64_t> &cells = res.table[table];
        s += std::string("# ") + name + "\t" + head + "\n";
        for (size_t r = 0; r < cells.size() / w; r++) {
            bool any = false;
            for (size_t c = 0; c < w; c++) any = any || cells[r * w + c];
            if (!any) continue;
            s += name;
            s += "\t" + std::to_string(r);
            for (size_t c = 0; c < w; c++) s += "\t" + std::to_string(cells[r * w + c]);
            s += "\n";
        }
    };
    sparse("MAPQ", "mapq\trecords", kStatsMapq);
    sparse("RL", "length\trecords", kStatsRl);
    sparse("GCF", "gc_percent\trecords", kStatsGc);
    sparse("ID", "length\tinsertions\tdeletions", kStatsId);
    sparse("IS", "insert_size\tinward\toutward\tother", kStatsIs);
    auto by_cycle = [&](const char *name, const std::string &head, size_t table, size_t shown) {
        const size_t w = kStatsWidth[table];
        const std::vector<uint64_t> &cells = res.table[table];
        size_t last = 0;                                 // rows shown: the cycles before it
        for (size_t k = 0; k < cells.size(); k++)
            if (cells[k]) last = k / w + 1;
        s += std::string("# ") + name + "\tcycle" + head + "\n";
        for (size_t r = 0; r < last; r++) {
            s += name;
            s += "\t" + std::to_string(r + 1);
            for (size_t c = 0; c < shown; c++) s += "\t" + std::to_string(cells[r * w + c]);
            s += "\n";
        }
    };
    by_cycle("BCC", "\tA\tC\tG\tT\tother", kStatsBc, 5);
    size_t top = 0;                                      // the QCC columns: 0 .. the largest quality seen
    bool any_q = false;
    for (size_t k = 0; k < res.table[kStatsQc].size(); k++)
        if (res.table[kStatsQc][k]) any_q = true, top = std::max(top, k % 64);
    std::string qhead;
    for (size_t q = 0; any_q && q <= top; q++) qhead += "\tq" + std::to_string(q);
    by_cycle("QCC", qhead, kStatsQc, any_q ? top + 1 : 0);
    by_cycle("MCC", "\t=\tX\tM\tI\tS\tD", kStatsMc, 6);
    f << s;
}

inline std::string stats_summary_line(const stats_result &res) {
    const uint64_t *t = res.tallies;
    return "Stats: " + std::to_string(t[0]) + " records (" + std::to_string(t[6]) + " mapped, " + std::to_string(t[11]) + " properly paired, " +
           std::to_string(t[4]) + " duplicates), " + std::to_string(t[18]) + " bases, " + std::to_string(t[24]) + " of " + std::to_string(t[23] + t[24]) +
           " =/X bases mismatch";
}

}  // namespace bm
