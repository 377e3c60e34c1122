// TEST ONLY: host/pileup.h as a program of its own (tests/test_pileup.py builds it with -fsanitize=address,undefined).
//   pileup_check <records.bin> <skip.bin | -> <bases.bin> <n_calls> <shuffle_seed> <min_mapq> <min_bq> <min_alt> <min_frac_ppm> <ref_len>...
//   pileup_check ppm <text>
// records.bin is a BAM record stream (records back to back, each led by its block_size), skip.bin a byte per record, bases.bin
// the references' bases back to back.  The records are shuffled when shuffle_seed is not 0 (the skip bytes with them), cut into
// n_calls stretches and handed to one pileup_counter, one add() per stretch.  Prints "sites N", the sites (twelve numbers
// each), "stats", six numbers per reference, and per reference "counts" and its eight counters per position; a refused begin()
// or add() prints "refused <what>" and returns 3.  The second form prints what cli.h's parse_ppm makes of the text, or "refused".
#include "../../bucket-map_amd/host/cli.h"
#include "../../bucket-map_amd/host/pileup.h"

#include <fstream>
#include <iostream>
#include <iterator>

static std::vector<uint8_t> read_file(const char *path) {
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc == 3 && std::string(argv[1]) == "ppm") {
        unsigned long ppm = 0;
        if (bm::parse_ppm(argv[2], ppm)) std::cout << ppm << "\n";
        else std::cout << "refused\n";
        return 0;
    }
    if (argc < 11) return 2;
    const std::vector<uint8_t> stream = read_file(argv[1]);
    std::vector<uint8_t> skip;
    if (std::string(argv[2]) != "-") skip = read_file(argv[2]);
    const std::vector<uint8_t> bases = read_file(argv[3]);
    const size_t n_calls = std::stoull(argv[4]);
    uint64_t seed = std::stoull(argv[5]);
    bm::pileup_thresholds th;
    th.min_mapq = static_cast<uint32_t>(std::stoul(argv[6]));
    th.min_bq = static_cast<uint32_t>(std::stoul(argv[7]));
    th.min_alt = static_cast<uint32_t>(std::stoul(argv[8]));
    th.min_frac_ppm = static_cast<uint32_t>(std::stoul(argv[9]));
    std::vector<uint32_t> ref_len;
    for (int k = 10; k < argc; k++) ref_len.push_back(static_cast<uint32_t>(std::stoul(argv[k])));
    std::vector<const uint8_t *> ref_bases;
    size_t total = 0;
    for (uint32_t len : ref_len) {
        ref_bases.push_back(bases.data() + total);
        total += len;
    }
    if (total != bases.size()) return 2;

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
        bm::pileup_counter counter;
        counter.begin(ref_len.data(), ref_len.size(), ref_bases.data(), th);
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
        bm::pileup_result res;
        std::vector<uint32_t> counts;
        counter.finish(res, &counts);
        std::string text = "sites " + std::to_string(res.n_sites()) + "\n";
        for (size_t k = 0; k < res.n_sites(); k++)
            for (size_t f = 0; f < bm::kPileupSiteWords; f++)
                text += std::to_string(res.sites[bm::kPileupSiteWords * k + f]) + (f + 1 < bm::kPileupSiteWords ? " " : "\n");
        text += "stats\n";
        for (size_t r = 0; r < ref_len.size(); r++)
            for (size_t k = 0; k < bm::kPileupStats; k++) text += std::to_string(res.stats[r * bm::kPileupStats + k]) + (k + 1 < bm::kPileupStats ? " " : "\n");
        size_t at = 0;
        for (size_t r = 0; r < ref_len.size(); r++) {
            text += "counts";
            for (size_t k = 0; k < static_cast<size_t>(ref_len[r]) * bm::kPileupCounters; k++) text += ' ', text += std::to_string(counts[at++]);
            text += "\n";
        }
        std::cout << text;
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    return 0;
}
