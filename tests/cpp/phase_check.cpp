// TEST ONLY: host/phase.h as a program of its own (tests/test_phase.py builds it with -fsanitize=address,undefined).
//   phase_check <records.bin> <skip.bin | -> <calls.bin> <n_adds> <shuffle_seed> <min_mapq> <min_bq> <min_links> <min_frac_ppm> <reach> <ref_len>...
//   phase_check vcf <calls.bin> <sites.bin | -> <notes.bin | -> <observations> <min_qual> <sample> <name:length>...
// records.bin is a BAM record stream (records back to back, each led by its block_size), skip.bin a byte per record, calls.bin
// 24 u32 per call.  The records are shuffled when shuffle_seed is not 0 (the skip bytes with them), cut into n_adds stretches
// and handed to one phase_linker, one add() per stretch.  Prints "sites H", the eight words of every site, "stats" with the
// four sums and "links" with reach x 4 numbers per site; a refused begin(), add() or finish() prints "refused <what>" and
// returns 3.
// The second form prints write_vcf_file's text for calls.bin with the phase of sites.bin (8 u32 per site) and, where given,
// the bias annotations of notes.bin (16 u32 per call), and on stderr the summary line.
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
    if (argc >= 9 && std::string(argv[1]) == "vcf") {
        bm::genotype_result res;
        res.calls = words_of(read_file(argv[2]));
        bm::phase_result phased;
        const bool with_phase = std::string(argv[3]) != "-";
        if (with_phase) phased.sites = words_of(read_file(argv[3]));
        bm::vcf_bias bias;
        const bool with_bias = std::string(argv[4]) != "-";
        if (with_bias) {
            bias.notes = words_of(read_file(argv[4]));
            if (bias.notes.size() / bm::kBiasOutWords != res.n_calls()) return 2;
        }
        phased.stats[0] = phased.n_sites(), phased.stats[3] = std::stoull(argv[5]);
        for (size_t k = 0; k < phased.n_sites(); k++) {
            const uint32_t flags = phased.sites[bm::kPhaseOutWords * k + bm::kPhaseWFlags];
            phased.stats[1] += (flags & bm::kPhasePhased) != 0;
            phased.stats[2] += flags == (bm::kPhasePhased | bm::kPhaseRoot);
        }
        const uint32_t min_qual = static_cast<uint32_t>(std::stoul(argv[6]));
        std::vector<std::string> ids;
        std::vector<uint32_t> lens;
        for (int k = 8; k < argc; k++) {
            const std::string s = argv[k];
            const size_t colon = s.rfind(':');
            ids.push_back(s.substr(0, colon));
            lens.push_back(static_cast<uint32_t>(std::stoul(s.substr(colon + 1))));
        }
        bm::vcf_phase linked;
        linked.sites = phased.sites;
        linked.index(res.n_calls());
        bm::write_vcf_file(std::cout, res, ids, lens, argv[7], min_qual, nullptr, nullptr, nullptr, with_bias ? &bias : nullptr, with_phase ? &linked : nullptr);
        if (with_phase) std::cerr << bm::phase_summary_line(bm::summarize_phase(phased, res.calls.data())) << "\n";
        return 0;
    }
    if (argc < 12) return 2;
    const std::vector<uint8_t> stream = read_file(argv[1]);
    std::vector<uint8_t> skip;
    if (std::string(argv[2]) != "-") skip = read_file(argv[2]);
    const std::vector<uint32_t> calls = words_of(read_file(argv[3]));
    const size_t n_adds = std::stoull(argv[4]), n_calls = calls.size() / bm::kPhaseCallWords;
    uint64_t seed = std::stoull(argv[5]);
    bm::phase_params pr;
    pr.min_mapq = static_cast<uint32_t>(std::stoul(argv[6]));
    pr.min_bq = static_cast<uint32_t>(std::stoul(argv[7]));
    pr.min_links = static_cast<uint32_t>(std::stoul(argv[8]));
    pr.min_frac_ppm = static_cast<uint32_t>(std::stoul(argv[9]));
    pr.reach = static_cast<uint32_t>(std::stoul(argv[10]));
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
        bm::phase_linker linker;
        const size_t H = linker.begin(ref_len.data(), ref_len.size(), pr, calls.data(), n_calls);
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
            linker.add(part.data(), off.data(), hi - lo, skip.empty() ? nullptr : part_skip.data());
        }
        bm::phase_result res;
        linker.finish(res);
        std::string text = "sites " + std::to_string(H) + "\n";
        for (size_t k = 0; k < H; k++)
            for (size_t f = 0; f < bm::kPhaseOutWords; f++) text += std::to_string(res.sites[bm::kPhaseOutWords * k + f]) + (f + 1 < bm::kPhaseOutWords ? " " : "\n");
        text += "stats";
        for (uint64_t v : res.stats) text += ' ', text += std::to_string(v);
        text += "\nlinks\n";
        const size_t per = static_cast<size_t>(pr.reach) * 4;
        for (size_t k = 0; k < H; k++)
            for (size_t f = 0; f < per; f++) text += std::to_string(linker.links()[per * k + f]) + (f + 1 < per ? " " : "\n");
        std::cout << text;
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    return 0;
}
