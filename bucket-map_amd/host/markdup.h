// markdup.h -- the duplicate-marking rule of include/bmd.h as plain C++17: what bmd_ends and bmd_mark compute on the device,
// value for value.
//
// The rule (fields, eligibility, the unclipped 5' end E, scores, mates, kinds, the marking and its known departures from
// Picard / samtools markdup) is stated in include/bmd.h; tests/markdup_rule.py restates it a third time in Python.  This copy
// is the marker of every build without a device behind it (block_compressor's defaults in bgzf.h, so the oracle-backed test
// tools) and the reference the device is compared with.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <numeric>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace bm {

namespace markdup_detail {
inline uint32_t u32(const uint8_t *p) {
    uint32_t v;
    std::memcpy(&v, p, 4);   // little-endian hosts only, like the rest of the tool
    return v;
}
inline uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }

// records x (the 0x40 one) and y, the next, are mates
inline bool mates(const uint8_t *x, const uint8_t *y) {
    const uint32_t fx = u16(x + 18), fy = u16(y + 18), mask = 0x1u | 0x40u | 0x80u | 0x100u | 0x800u;
    if ((fx & mask) != (0x1u | 0x40u) || (fy & mask) != (0x1u | 0x80u)) return false;
    return x[12] == y[12] && std::memcmp(x + 36, y + 36, x[12]) == 0;
}
}  // namespace markdup_detail

// end[i] = E(i) or 0, score[i], kind[i] of the n_records records in[rec_offset[i], rec_offset[i + 1])
inline void markdup_ends(const uint8_t *in, const uint64_t *rec_offset, size_t n_records, std::vector<uint64_t> &end, std::vector<uint64_t> &score,
                         std::vector<uint8_t> &kind) {
    using namespace markdup_detail;
    end.assign(n_records, 0);
    score.assign(n_records, 0);
    kind.assign(n_records, 0);
    for (size_t i = 0; i < n_records; i++) {
        const uint8_t *r = in + rec_offset[i];
        const uint64_t length = rec_offset[i + 1] - rec_offset[i];
        if (length < 36) throw std::runtime_error("--markdup: a record of " + std::to_string(length) + " bytes");
        const int32_t ref = static_cast<int32_t>(u32(r + 4)), pos = static_cast<int32_t>(u32(r + 8));
        const uint32_t l_name = r[12], n_cigar = u16(r + 16), flag = u16(r + 18), l_seq = u32(r + 20);
        const uint64_t qual_at = 36ull + l_name + 4ull * n_cigar + (static_cast<uint64_t>(l_seq) + 1) / 2;
        if (qual_at + l_seq > length) throw std::runtime_error("--markdup: a record's fields lie beyond its end");
        for (uint32_t k = 0; k < l_seq; k++) {
            const uint8_t q = r[qual_at + k];
            if (q >= 15 && q != 0xFF) score[i] += q;
        }
        const uint8_t *cigar = r + 36 + l_name;
        auto is_clip = [&](uint32_t k) { return (u32(cigar + 4 * k) & 15u) == 4 || (u32(cigar + 4 * k) & 15u) == 5; };
        int64_t reflen = 0, lead = 0, trail = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            const uint32_t c = u32(cigar + 4 * k), op = c & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reflen += c >> 4;
        }
        for (uint32_t k = 0; k < n_cigar && is_clip(k); k++) lead += u32(cigar + 4 * k) >> 4;
        for (uint32_t k = n_cigar; k-- > 0 && is_clip(k);) trail += u32(cigar + 4 * k) >> 4;
        const bool reverse = flag & 0x10u;
        const int64_t end5 = reverse ? pos + reflen + trail - 1 : pos - lead;
        const bool placeholder = n_cigar == 2 && u32(cigar) == (l_seq << 4 | 4u) && (u32(cigar + 4) & 15u) == 3;
        const bool ok = !(flag & (0x4u | 0x100u | 0x800u)) && ref >= 0 && !placeholder && end5 >= -(int64_t{1} << 31) && end5 < (int64_t{1} << 31);
        if (ok) {
            end[i] = static_cast<uint64_t>(static_cast<uint32_t>(ref)) << 33 | static_cast<uint64_t>(end5 + (int64_t{1} << 31)) << 1 | (reverse ? 1u : 0u);
            kind[i] = 1;
        }
    }
    for (size_t i = 0; i + 1 < n_records; i++)
        if (kind[i] && kind[i + 1] && mates(in + rec_offset[i], in + rec_offset[i + 1])) kind[i] = 2, kind[i + 1] = 3;
}

// dup[i] and counts = (pair units, fragment units, duplicate records from pair units, duplicate fragment records)
inline void markdup_mark(const uint64_t *end, const uint64_t *score, const uint8_t *kind, size_t n, std::vector<uint8_t> &dup, uint64_t counts[4]) {
    dup.assign(n, 0);
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (size_t i = 0; i < n; i++) {
        if (kind[i] > 3) throw std::runtime_error("--markdup: a descriptor of kind " + std::to_string(kind[i]));
        if ((kind[i] == 2 && (i + 1 == n || kind[i + 1] != 3)) || (kind[i] == 3 && (i == 0 || kind[i - 1] != 2)))
            throw std::runtime_error("--markdup: half a pair unit among the descriptors");
    }
    using key_t = std::pair<uint64_t, uint64_t>;
    auto key_of = [&](size_t i) { return key_t(std::min(end[i], end[i + 1]), std::max(end[i], end[i + 1])); };
    std::vector<size_t> pairs, frags;
    for (size_t i = 0; i < n; i++)
        if (kind[i] == 2) pairs.push_back(i);
        else if (kind[i] == 1) frags.push_back(i);
    // the greatest score first, then the lowest i: the head of each run of equal keys is the kept unit
    std::stable_sort(pairs.begin(), pairs.end(), [&](size_t x, size_t y) {
        const key_t a = key_of(x), b = key_of(y);
        return a != b ? a < b : score[x] + score[x + 1] > score[y] + score[y + 1];
    });
    for (size_t k = 1; k < pairs.size(); k++)
        if (key_of(pairs[k]) == key_of(pairs[k - 1])) dup[pairs[k]] = dup[pairs[k] + 1] = 1, counts[2] += 2;
    std::set<uint64_t> pair_ends;
    for (size_t i : pairs) pair_ends.insert(end[i]), pair_ends.insert(end[i + 1]);
    std::stable_sort(frags.begin(), frags.end(), [&](size_t x, size_t y) { return end[x] != end[y] ? end[x] < end[y] : score[x] > score[y]; });
    for (size_t k = 0; k < frags.size(); k++)
        if (pair_ends.count(end[frags[k]]) || (k > 0 && end[frags[k]] == end[frags[k - 1]])) dup[frags[k]] = 1, counts[3]++;
    counts[0] = pairs.size(), counts[1] = frags.size();
}

}  // namespace bm
