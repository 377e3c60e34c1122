// TEST ONLY: host/genotype.h as a program of its own (tests/test_genotype.py builds it with -fsanitize=address,undefined).
//   genotype_check <records.bin> <skip.bin | -> <sites.bin> <n_calls> <shuffle_seed> <min_mapq> <min_bq> <q_absent> <q_cap> <prior> <ref_len>...
//   genotype_check vcf <calls.bin> <min_qual> <sample> <name:length>...
// records.bin is a BAM record stream (records back to back, each led by its block_size), skip.bin a byte per record, sites.bin
// twelve u32 per site.  The records are shuffled when shuffle_seed is not 0 (the skip bytes with them), cut into n_calls
// stretches and handed to one genotype_counter, one add() per stretch; call() runs after the first stretch too (its result is
// dropped: it must not end or disturb the counting) and after the last.  Prints "calls N", the calls (24 numbers each), and per
// reference "cells" and its four cells per position; a refused begin(), add() or call() prints "refused <what>" and returns 3.
// The second form prints write_vcf_file's text for calls.bin (24 u32 per call).
#include "../../bucket-map_amd/host/genotype.h"

#include <fstream>
#include <iostream>
#include <iterator>

static std::vector<uint8_t> read_file(const char *path) {
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static std::vector<uint32_t> words_of(const std::vector<uint8_t> &bytes) {
    std::vector<uint32_t> out(bytes.size() / 4);
    if (!out.empty()) std::memcpy(out.data(), bytes.data(), out.size() * 4);
    return out;
}

int main(int argc, char **argv) {
    if (argc >= 5 && std::string(argv[1]) == "vcf") {
        bm::genotype_result res;
        res.calls = words_of(read_file(argv[2]));
        std::vector<std::string> ids;
        std::vector<uint32_t> lens;
        for (int k = 5; k < argc; k++) {
            const std::string s = argv[k];
            const size_t colon = s.rfind(':');
            ids.push_back(s.substr(0, colon));
            lens.push_back(static_cast<uint32_t>(std::stoul(s.substr(colon + 1))));
        }
        const uint32_t min_qual = static_cast<uint32_t>(std::stoul(argv[3]));
        bm::write_vcf_file(std::cout, res, ids, lens, argv[4], min_qual);
        const bm::genotype_summary s = bm::summarize_genotypes(res, min_qual);
        std::cerr << "summary " << s.variants << " " << s.het << " " << s.hom << " " << s.low_qual << "\n";
        return 0;
    }
    if (argc < 12) return 2;
    const std::vector<uint8_t> stream = read_file(argv[1]);
    std::vector<uint8_t> skip;
    if (std::string(argv[2]) != "-") skip = read_file(argv[2]);
    const std::vector<uint32_t> sites = words_of(read_file(argv[3]));
    const size_t n_calls = std::stoull(argv[4]);
    uint64_t seed = std::stoull(argv[5]);
    bm::genotype_params pr;
    pr.min_mapq = static_cast<uint32_t>(std::stoul(argv[6]));
    pr.min_bq = static_cast<uint32_t>(std::stoul(argv[7]));
    pr.q_absent = static_cast<uint32_t>(std::stoul(argv[8]));
    pr.q_cap = static_cast<uint32_t>(std::stoul(argv[9]));
    pr.prior = static_cast<uint32_t>(std::stoul(argv[10]));
    std::vector<uint32_t> ref_len;
    for (int k = 11; k < argc; k++) ref_len.push_back(static_cast<uint32_t>(std::stoul(argv[k])));

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
        bm::genotype_counter counter;
        counter.begin(ref_len.data(), ref_len.size(), pr);
        std::vector<uint32_t> calls;
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
            if (call == 0) counter.call(sites.data(), sites.size() / bm::kGenotypeSiteWords, calls);
        }
        counter.call(sites.data(), sites.size() / bm::kGenotypeSiteWords, calls);
        const size_t n = calls.size() / bm::kGenotypeCallWords;
        std::string text = "calls " + std::to_string(n) + "\n";
        for (size_t k = 0; k < n; k++)
            for (size_t f = 0; f < bm::kGenotypeCallWords; f++)
                text += std::to_string(calls[bm::kGenotypeCallWords * k + f]) + (f + 1 < bm::kGenotypeCallWords ? " " : "\n");
        size_t at = 0;
        for (size_t r = 0; r < ref_len.size(); r++) {
            text += "cells";
            for (size_t k = 0; k < static_cast<size_t>(ref_len[r]) * bm::kGenotypeCells; k++) text += ' ', text += std::to_string(counter.cells()[at++]);
            text += "\n";
        }
        std::cout << text;
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    return 0;
}
