// TEST ONLY: host/stats.h as a program of its own (tests/test_stats.py builds it with -fsanitize=address,undefined).
//   stats_check <records.bin> <skip.bin | -> <n_adds> <shuffle_seed> <max_cycle> <max_insert> [text]
// records.bin is a BAM record stream (records back to back, each led by its block_size), skip.bin a byte per record.  The
// records are shuffled when shuffle_seed is not 0 (the skip bytes with them), cut into n_adds stretches and handed to one
// stats_counter, one add() per stretch.  Prints "tallies" with the 35 numbers, then per table "table <index> <rows> <width>" and
// one line "<row> <column> <count>" per non-zero cell; with `text`, write_stats_file's text instead and the summary line on
// stderr.  A refused begin(), add() or finish() prints "refused <what>" and returns 3.
#include "../../bucket-map_amd/host/stats.h"

#include <fstream>
#include <iostream>
#include <iterator>

static std::vector<uint8_t> read_file(const char *path) {
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc < 7) return 2;
    const std::vector<uint8_t> stream = read_file(argv[1]);
    std::vector<uint8_t> skip;
    if (std::string(argv[2]) != "-") skip = read_file(argv[2]);
    const size_t n_adds = std::stoull(argv[3]);
    uint64_t seed = std::stoull(argv[4]);
    bm::stats_params pr;
    pr.max_cycle = static_cast<uint32_t>(std::stoul(argv[5]));
    pr.max_insert = static_cast<uint32_t>(std::stoul(argv[6]));
    const bool as_text = argc > 7 && std::string(argv[7]) == "text";
    if (n_adds == 0) return 2;

    std::vector<std::pair<size_t, size_t>> recs;         // (start, length)
    for (size_t at = 0; at < stream.size();) {
        if (stream.size() - at < 4) return 2;
        uint32_t size;
        std::memcpy(&size, stream.data() + at, 4);
        if (size > stream.size() - at - 4) return 2;
        recs.emplace_back(at, 4 + static_cast<size_t>(size));
        at += 4 + static_cast<size_t>(size);
    }
    if (!skip.empty() && skip.size() != recs.size()) return 2;
    std::vector<size_t> order(recs.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    if (seed)
        for (size_t i = order.size(); i > 1; i--) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(order[i - 1], order[(seed >> 33) % i]);
        }
    try {
        bm::stats_counter counter;
        counter.begin(pr);
        for (size_t add = 0; add < n_adds; add++) {
            const size_t lo = recs.size() * add / n_adds, hi = recs.size() * (add + 1) / n_adds;
            std::vector<uint8_t> part, part_skip;
            std::vector<uint64_t> off{0};
            for (size_t k = lo; k < hi; k++) {
                const auto [at, len] = recs[order[k]];
                part.insert(part.end(), stream.begin() + static_cast<std::ptrdiff_t>(at), stream.begin() + static_cast<std::ptrdiff_t>(at + len));
                off.push_back(part.size());
                if (!skip.empty()) part_skip.push_back(skip[order[k]]);
            }
            counter.add(part.data(), off.data(), hi - lo, skip.empty() ? nullptr : part_skip.data());
        }
        bm::stats_result res;
        counter.finish(res);
        if (as_text) {
            bm::write_stats_file(std::cout, res);
            std::cerr << bm::stats_summary_line(res) << "\n";
            return 0;
        }
        std::string text = "tallies";
        for (uint64_t v : res.tallies) text += ' ', text += std::to_string(v);
        text += "\n";
        for (size_t t = 0; t < bm::kStatsTables; t++) {
            const size_t w = bm::kStatsWidth[t];
            text += "table " + std::to_string(t) + " " + std::to_string(res.table[t].size() / w) + " " + std::to_string(w) + "\n";
            for (size_t k = 0; k < res.table[t].size(); k++)
                if (res.table[t][k]) text += std::to_string(k / w) + " " + std::to_string(k % w) + " " + std::to_string(res.table[t][k]) + "\n";
        }
        std::cout << text;
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    return 0;
}
