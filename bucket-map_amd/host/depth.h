// depth.h -- the coverage rule of include/bmc.h as plain C++17: what bmc_begin / bmc_add / bmc_finish compute on the device,
// value for value.
//
// The rule (placed and counted records, blocks and their clipping, depth, runs, the seven sums per reference and its known
// departure for long-CIGAR records) is stated in include/bmc.h; tests/depth_rule.py restates it a third time in Python.  This
// copy is the counter of every build without a device behind it (block_compressor's defaults in bgzf.h, so the oracle-backed
// test tools) and the reference the device is compared with.  It also writes the two files of --depth and --coverage.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

namespace bm {

constexpr size_t kDepthStats = 7;   // BMC_N_STATS: n_reads, cov_bases, sum_depth, sum_mapq, sum_qual, n_qual, n_long

struct depth_result {
    std::vector<uint32_t> runs;     // 4 per run: reference, start, end, depth
    std::vector<uint64_t> stats;    // kDepthStats per reference
    size_t n_runs() const { return runs.size() / 4; }
};

class depth_counter {
    std::vector<uint32_t> ref_len_;
    std::vector<uint64_t> base_;    // reference r: slots base_[r] .. base_[r + 1] - 1, one more than it has bases
    std::vector<uint32_t> diff_;
    std::vector<uint64_t> stats_;
    bool begun_ = false;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);   // little-endian hosts only, like the rest of the tool
        return v;
    }
    static uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }

public:
    void begin(const uint32_t *ref_len, size_t n_ref) {
        if (n_ref == 0) throw std::runtime_error("--depth: no reference");
        uint64_t bases = 0;
        for (size_t r = 0; r < n_ref; r++) {
            if (ref_len[r] == 0) throw std::runtime_error("--depth: reference " + std::to_string(r) + " has the length 0");
            bases += ref_len[r];
        }
        if (bases > (uint64_t{1} << 32) - (uint64_t{1} << 20) || bases + n_ref > 0xFFFFFFFEull)
            throw std::runtime_error("--depth: " + std::to_string(bases) + " bases, at most 2^32 - 2^20 are counted in one go");
        ref_len_.assign(ref_len, ref_len + n_ref);
        base_.assign(n_ref + 1, 0);
        for (size_t r = 0; r < n_ref; r++) base_[r + 1] = base_[r] + ref_len[r] + 1;
        diff_.assign(base_[n_ref], 0);
        stats_.assign(n_ref * kDepthStats, 0);
        begun_ = true;
    }

    // whole records in[rec_offset[i], rec_offset[i + 1]); skip may be null
    void add(const uint8_t *in, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        if (!begun_) throw std::runtime_error("--depth: records before the references");
        // the checks first: a refused call changes nothing
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const uint64_t length = rec_offset[i + 1] - rec_offset[i];
            if (length < 36) throw std::runtime_error("--depth: a record of " + std::to_string(length) + " bytes");
            const int32_t ref = static_cast<int32_t>(u32(r + 4));
            const uint32_t l_name = r[12], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if (36ull + l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2 + l_seq > length)
                throw std::runtime_error("--depth: a record's fields lie beyond its end");
            uint64_t query = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = u32(r + 36 + l_name + 4ull * k), op = c & 15u;
                if (op > 8) throw std::runtime_error("--depth: a CIGAR op with the code " + std::to_string(op));
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) query += c >> 4;
            }
            if (n_cigar && l_seq && query != l_seq)
                throw std::runtime_error("--depth: a CIGAR of " + std::to_string(query) + " query bases on a record of " + std::to_string(l_seq));
            if (ref >= 0 && static_cast<size_t>(ref) >= ref_len_.size() && !(flag & 4u))
                throw std::runtime_error("--depth: a record names reference " + std::to_string(ref) + ", there are " + std::to_string(ref_len_.size()));
        }
        for (size_t i = 0; i < n_records; i++) {
            const uint8_t *r = in + rec_offset[i];
            const int32_t ref = static_cast<int32_t>(u32(r + 4)), pos = static_cast<int32_t>(u32(r + 8));
            const uint32_t l_name = r[12], mapq = r[13], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
            if ((flag & (0x4u | 0x100u | 0x200u | 0x400u)) || (skip && skip[i])) continue;
            if (ref < 0 || static_cast<size_t>(ref) >= ref_len_.size() || pos < 0 || static_cast<uint32_t>(pos) >= ref_len_[ref] || n_cigar == 0) continue;
            const uint8_t *cigar = r + 36 + l_name, *qual = cigar + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2;
            uint64_t *st = stats_.data() + static_cast<size_t>(ref) * kDepthStats;
            if (n_cigar == 2 && u32(cigar) == (l_seq << 4 | 4u) && (u32(cigar + 4) & 15u) == 3) {   // the long-CIGAR placeholder
                st[6]++;
                continue;
            }
            st[0]++;
            st[3] += mapq;
            const uint64_t rlen = ref_len_[ref];
            uint32_t *d = diff_.data() + base_[ref];
            uint64_t rc = static_cast<uint64_t>(pos), qc = 0;
            for (uint32_t k = 0; k < n_cigar; k++) {
                const uint32_t c = u32(cigar + 4ull * k), op = c & 15u, len = c >> 4;
                const bool block = op == 0 || op == 7 || op == 8;
                if (block && len && rc < rlen) {
                    const uint64_t e = std::min<uint64_t>(rc + len, rlen);
                    d[rc]++;
                    d[e]--;                              // e <= rlen: the reference's extra slot at most
                    if (l_seq)
                        for (uint64_t j = 0; j < e - rc; j++) {
                            const uint8_t q = qual[qc + j];
                            if (q != 0xFF) st[4] += q, st[5]++;
                        }
                }
                if (block || op == 2 || op == 3) rc += len;
                if (block || op == 1 || op == 4) qc += len;
            }
        }
    }

    // the runs and the sums of everything added; depth, where given, receives every reference's depths back to back
    void finish(depth_result &out, std::vector<uint32_t> *depth = nullptr) {
        if (!begun_) throw std::runtime_error("--depth: a result before the references");
        out.runs.clear();
        if (depth) depth->clear();
        for (size_t r = 0; r < ref_len_.size(); r++) {
            uint64_t *st = stats_.data() + r * kDepthStats;
            st[1] = st[2] = 0;
            const uint32_t *d = diff_.data() + base_[r];
            uint32_t now = 0, before = 0;
            for (uint32_t p = 0; p <= ref_len_[r]; p++) {   // the extra slot closes the last run: its depth is 0
                now += d[p];
                if (now != before) {
                    if (before > 0) out.runs[out.runs.size() - 2] = p;
                    if (now > 0) out.runs.insert(out.runs.end(), {static_cast<uint32_t>(r), p, 0u, now});
                }
                if (p < ref_len_[r]) {
                    st[1] += now > 0;
                    st[2] += now;
                    if (depth) depth->push_back(now);
                }
                before = now;
            }
        }
        out.stats = stats_;
    }
};

// --depth FILE: bedGraph lines, one per run
inline void write_depth_file(std::ostream &out, const depth_result &res, const std::vector<std::string> &ref_ids) {
    std::string buf;
    for (size_t k = 0; k < res.n_runs(); k++) {
        const uint32_t *run = res.runs.data() + 4 * k;
        buf += ref_ids.at(run[0]);
        for (int f = 1; f < 4; f++) buf += '\t', buf += std::to_string(run[f]);
        buf += '\n';
        if (buf.size() > (1u << 20)) out.write(buf.data(), static_cast<std::streamsize>(buf.size())), buf.clear();
    }
    out.write(buf.data(), static_cast<std::streamsize>(buf.size()));
}

// --coverage FILE: the header line, then one line per reference; a ratio with the divisor 0 is 0
inline void write_coverage_file(std::ostream &out, const depth_result &res, const std::vector<std::string> &ref_ids, const std::vector<uint32_t> &ref_len) {
    out << "#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmeanbaseq\tmeanmapq\n";
    auto ratio = [](double a, double b) { return b == 0 ? 0.0 : a / b; };
    for (size_t r = 0; r < ref_ids.size(); r++) {
        const uint64_t *st = res.stats.data() + r * kDepthStats;
        char line[256];
        std::snprintf(line, sizeof line, "\t1\t%u\t%llu\t%llu\t%.4f\t%.4f\t%.4f\t%.4f\n", ref_len[r], static_cast<unsigned long long>(st[0]),
                      static_cast<unsigned long long>(st[1]), ratio(100.0 * static_cast<double>(st[1]), ref_len[r]),
                      ratio(static_cast<double>(st[2]), ref_len[r]), ratio(static_cast<double>(st[4]), static_cast<double>(st[5])),
                      ratio(static_cast<double>(st[3]), static_cast<double>(st[0])));
        out << ref_ids[r] << line;
    }
}

}  // namespace bm
