// TEST ONLY: host/indel.h as a program of its own (tests/test_indel.py builds it with -fsanitize=address,undefined).
//   indel_check <records.bin> <skip.bin | -> <n_calls> <shuffle_seed> <min_mapq> <min_alt> <min_frac_ppm> <q_indel> <prior> <ref_len>...
//   indel_check vcf <calls.bin> <min_qual> <name:bases>...
// records.bin is a BAM record stream (records back to back, each led by its block_size), skip.bin a byte per record.  The
// records are shuffled when shuffle_seed is not 0 (the skip bytes with them), cut into n_calls stretches and handed to one
// indel_caller, one add() per stretch.  Prints "events N", "alleles N" and the alleles (8 numbers each), "calls N" and the calls
// (16 numbers each), per reference "stats" and its three sums, per reference "cover" and its cover per position, and the
// summary line for min_qual 20; a refused begin() or add() prints "refused <what>" and returns 3.
// The second form prints the header line and append_indel_vcf_line's text for the variant calls of calls.bin (16 u32 per call).
#include "../../bucket-map_amd/host/indel.h"

#include <fstream>
#include <iostream>
#include <iterator>

static std::vector<uint8_t> read_file(const char *path) {
    std::ifstream in(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv) {
    if (argc >= 4 && std::string(argv[1]) == "vcf") {
        const std::vector<uint8_t> bytes = read_file(argv[2]);
        std::vector<uint32_t> calls(bytes.size() / 4);
        if (!calls.empty()) std::memcpy(calls.data(), bytes.data(), calls.size() * 4);
        std::vector<std::string> ids, bases;
        for (int k = 4; k < argc; k++) {
            const std::string s = argv[k];
            const size_t colon = s.rfind(':');
            ids.push_back(s.substr(0, colon));
            bases.push_back(s.substr(colon + 1));
        }
        const uint32_t min_qual = static_cast<uint32_t>(std::stoul(argv[3]));
        std::string text = bm::indel_vcf_header();
        try {
            for (size_t k = 0; k < calls.size() / bm::kIndelCallWords; k++) {
                const uint32_t *c = calls.data() + bm::kIndelCallWords * k;
                if (c[5] & bm::kIndelVariant) bm::append_indel_vcf_line(text, c, ids.at(c[0]), bases.at(c[0]), min_qual);
            }
        } catch (const std::exception &e) {
            std::cout << "refused " << e.what() << "\n";
            return 3;
        }
        std::cout << text;
        return 0;
    }
    if (argc < 11) return 2;
    const std::vector<uint8_t> stream = read_file(argv[1]);
    std::vector<uint8_t> skip;
    if (std::string(argv[2]) != "-") skip = read_file(argv[2]);
    const size_t n_calls = std::stoull(argv[3]);
    uint64_t seed = std::stoull(argv[4]);
    bm::indel_params pr;
    pr.min_mapq = static_cast<uint32_t>(std::stoul(argv[5]));
    pr.min_alt = static_cast<uint32_t>(std::stoul(argv[6]));
    pr.min_frac_ppm = static_cast<uint32_t>(std::stoul(argv[7]));
    pr.q_indel = static_cast<uint32_t>(std::stoul(argv[8]));
    pr.prior = static_cast<uint32_t>(std::stoul(argv[9]));
    std::vector<uint32_t> ref_len;
    for (int k = 10; k < argc; k++) ref_len.push_back(static_cast<uint32_t>(std::stoul(argv[k])));

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
        bm::indel_caller caller;
        caller.begin(ref_len.data(), ref_len.size(), pr);
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
            caller.add(part.data(), off.data(), hi - lo, skip.empty() ? nullptr : part_skip.data());
        }
        bm::indel_result res;
        caller.finish(res);
        std::string text = "events " + std::to_string(res.n_events) + "\nalleles " + std::to_string(res.n_alleles()) + "\n";
        for (size_t k = 0; k < res.n_alleles(); k++)
            for (size_t f = 0; f < bm::kIndelAlleleWords; f++)
                text += std::to_string(res.alleles[bm::kIndelAlleleWords * k + f]) + (f + 1 < bm::kIndelAlleleWords ? " " : "\n");
        text += "calls " + std::to_string(res.n_calls()) + "\n";
        for (size_t k = 0; k < res.n_calls(); k++)
            for (size_t f = 0; f < bm::kIndelCallWords; f++)
                text += std::to_string(res.calls[bm::kIndelCallWords * k + f]) + (f + 1 < bm::kIndelCallWords ? " " : "\n");
        size_t at = 0;
        for (size_t r = 0; r < ref_len.size(); r++) {
            text += "stats";
            for (size_t k = 0; k < bm::kIndelStats; k++) text += ' ', text += std::to_string(res.stats[r * bm::kIndelStats + k]);
            text += "\n";
        }
        for (size_t r = 0; r < ref_len.size(); r++) {
            text += "cover";
            for (size_t k = 0; k < ref_len[r]; k++) text += ' ', text += std::to_string(caller.cover()[at++]);
            text += "\n";
        }
        text += bm::indel_summary_line(bm::summarize_indels(res, 20)) + "\n";
        std::cout << text;
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    return 0;
}
