// split_pick_check.cpp -- TEST ONLY: a program of its own around host/split_pick.h, built under -fsanitize=address,undefined
// by tests/test_split.py.  It prints one line per case -- the inputs and what the header computed -- and the test recomputes
// every line with the Python restatement (bucket_map_amd.verify.select_segments, split_mapq, sa_entry).
//   P <min_score> <permille> <max_segments> <use_contig> <n> {score q_lo q_hi g_lo g_hi rc contig}*n | <n_seg> {seg s2}*max_segments
//   Q <s1> <s2> <mapq>
//   A <rname> <pos0> <reverse> <mapq> <nm> <k> {entry}*k | <text>
#include "../../bucket-map_amd/host/split_pick.h"

#include <cinttypes>
#include <cstdio>
#include <random>

namespace {

void pick_case(const std::vector<int64_t> &score, const std::vector<uint32_t> &q_lo, const std::vector<uint32_t> &q_hi,
               const std::vector<int64_t> &g_lo, const std::vector<int64_t> &g_hi, const std::vector<uint8_t> &rc,
               const std::vector<uint32_t> &contig, bool use_contig, uint32_t min_score, uint32_t permille, uint32_t max_segments) {
    const uint32_t n = static_cast<uint32_t>(score.size());
    const uint32_t group_offset[2] = {0, n};
    bm::split_result out;
    bm::select_segments(score.data(), q_lo.data(), q_hi.data(), g_lo.data(), g_hi.data(), rc.data(), use_contig ? contig.data() : nullptr,
                        group_offset, 1, min_score, permille, max_segments, out);
    std::printf("P %u %u %u %d %u", min_score, permille, max_segments, use_contig ? 1 : 0, n);
    for (uint32_t a = 0; a < n; a++)
        std::printf(" %" PRId64 " %u %u %" PRId64 " %" PRId64 " %d %u", score[a], q_lo[a], q_hi[a], g_lo[a], g_hi[a], rc[a], contig[a]);
    std::printf(" | %u", out.n_seg[0]);
    for (uint32_t k = 0; k < max_segments; k++) std::printf(" %u %" PRId64, out.seg[k], out.s2[k]);
    std::printf("\n");
}

}  // namespace

int main() {
    std::mt19937_64 rng(20260114);
    auto below = [&](uint64_t n) { return static_cast<uint64_t>(rng() % n); };
    // an empty group, and one without anything eligible
    pick_case({}, {}, {}, {}, {}, {}, {}, false, 40, 500, 8);
    pick_case({39, 0, -5}, {0, 10, 20}, {10, 20, 30}, {100, 200, 300}, {110, 210, 310}, {0, 1, 0}, {0, 0, 0}, true, 40, 500, 8);
    for (int t = 0; t < 600; t++) {
        // few distinct scores, short reads and a small genome: ties, overlaps at the threshold and dups all occur
        const uint32_t n = static_cast<uint32_t>(below(t % 7 == 0 ? 40 : 9));
        const uint32_t m = 20 + static_cast<uint32_t>(below(40));
        std::vector<int64_t> score(n), g_lo(n), g_hi(n);
        std::vector<uint32_t> q_lo(n), q_hi(n), contig(n);
        std::vector<uint8_t> rc(n);
        for (uint32_t a = 0; a < n; a++) {
            score[a] = static_cast<int64_t>(below(8)) * 5 - 5 + (below(10) == 0 ? (int64_t{1} << 40) : 0);
            q_lo[a] = static_cast<uint32_t>(below(m));
            q_hi[a] = q_lo[a] + static_cast<uint32_t>(below(m - q_lo[a] + 1));
            g_lo[a] = static_cast<int64_t>(below(120)) + (below(12) == 0 ? (int64_t{1} << 61) : 0);
            g_hi[a] = g_lo[a] + static_cast<int64_t>(below(40));
            rc[a] = static_cast<uint8_t>(below(2) * (1 + below(3)));
            contig[a] = static_cast<uint32_t>(below(2));
        }
        const uint32_t permille[5] = {0, 250, 500, 999, 1000};
        pick_case(score, q_lo, q_hi, g_lo, g_hi, rc, contig, below(4) != 0, 1 + static_cast<uint32_t>(below(3)) * 10, permille[below(5)],
                  t % 5 == 0 ? 16 : 1 + static_cast<uint32_t>(below(4)));
    }
    const int64_t s[] = {1, 2, 39, 40, 41, 100, 6000, int64_t{1} << 43, (int64_t{1} << 43) + 7};
    for (const int64_t s1 : s) {
        std::printf("Q %" PRId64 " %" PRId64 " %u\n", s1, bm::kSplitNone, bm::split_mapq(s1, bm::kSplitNone));
        for (const int64_t s2 : s) std::printf("Q %" PRId64 " %" PRId64 " %u\n", s1, s2, bm::split_mapq(s1, s2));
    }
    for (int t = 0; t < 60; t++) {
        const uint32_t ops[] = {4, 7, 8, 1, 2, 7, 8, 7};
        std::vector<uint32_t> entry;
        const uint32_t k = static_cast<uint32_t>(below(9));
        for (uint32_t i = 0; i < k; i++) entry.push_back((1 + static_cast<uint32_t>(below(300))) << 4 | ops[below(8)]);
        const char *names[] = {"chr1", "chrUn_KI270442v1", "2"};
        const char *rname = names[below(3)];
        const uint64_t pos0 = below(3) == 0 ? (uint64_t{1} << 33) + below(1000) : below(100000);
        const bool reverse = below(2) != 0;
        const unsigned int mapq = static_cast<unsigned int>(below(61));
        const uint32_t nm = static_cast<uint32_t>(below(5000));
        std::string text;
        bm::append_sa_entry(text, rname, pos0, reverse, entry.data(), entry.size(), mapq, nm);
        std::printf("A %s %" PRIu64 " %d %u %u %u", rname, pos0, reverse ? 1 : 0, mapq, nm, k);
        for (const uint32_t e : entry) std::printf(" %u", e);
        std::printf(" | %s\n", text.c_str());
    }
    return 0;
}
