// TEST ONLY: host/depth.h as a program of its own (tests/test_depth.py builds it with -fsanitize=address,undefined).
//   depth_check <records.bin> <skip.bin | -> <n_calls> <shuffle_seed> <ref_len>...
// records.bin is a BAM record stream (records back to back, each led by its block_size), skip.bin a byte per record.  The
// records are shuffled when shuffle_seed is not 0 (the skip bytes with them), cut into n_calls stretches and handed to one
// depth_counter, one add() per stretch.  Prints "runs N", the runs, "stats", seven numbers per reference, and per reference
// "depth" and its depths; a refused add() prints "refused <what>" and returns 3.
#include "../../bucket-map_amd/host/depth.h"

#include <fstream>
#include <iostream>
#include <iterator>

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const std::vector<uint8_t> stream((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    std::vector<uint8_t> skip;
    if (std::string(argv[2]) != "-") {
        std::ifstream s(argv[2], std::ios::binary);
        skip.assign((std::istreambuf_iterator<char>(s)), std::istreambuf_iterator<char>());
    }
    const size_t n_calls = std::stoull(argv[3]);
    uint64_t seed = std::stoull(argv[4]);
    std::vector<uint32_t> ref_len;
    for (int k = 5; k < argc; k++) ref_len.push_back(static_cast<uint32_t>(std::stoul(argv[k])));

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
        bm::depth_counter counter;
        counter.begin(ref_len.data(), ref_len.size());
        for (size_t call = 0; call < n_calls; call++) {
            const size_t lo = recs.size() * call / n_calls, hi = recs.size() * (call + 1) / n_calls;
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
        bm::depth_result res;
        std::vector<uint32_t> depth;
        counter.finish(res, &depth);
        std::cout << "runs " << res.n_runs() << "\n";
        for (size_t k = 0; k < res.n_runs(); k++)
            std::cout << res.runs[4 * k] << " " << res.runs[4 * k + 1] << " " << res.runs[4 * k + 2] << " " << res.runs[4 * k + 3] << "\n";
        std::cout << "stats\n";
        for (size_t r = 0; r < ref_len.size(); r++) {
            for (size_t k = 0; k < bm::kDepthStats; k++) std::cout << (k ? " " : "") << res.stats[r * bm::kDepthStats + k];
            std::cout << "\n";
        }
        size_t at = 0;
        for (size_t r = 0; r < ref_len.size(); r++) {
            std::cout << "depth";
            for (uint32_t p = 0; p < ref_len[r]; p++) std::cout << " " << depth[at++];
            std::cout << "\n";
        }
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    return 0;
}
