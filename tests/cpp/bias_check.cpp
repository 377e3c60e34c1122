// TEST ONLY: host/bias.h as a program of its own (tests/test_bias.py builds it with -fsanitize=address,undefined).
//   bias_check <tables.bin> <records.bin> <skip.bin | -> <calls.bin> <n_adds> <shuffle_seed> <min_mapq> <min_bq> <ref_len>...
//   bias_check vcf <calls.bin> <notes.bin> <min_qual> <max_fs> <min_mq> <sample> <name:length>...
// tables.bin is LF (65 536 u32) and then E (12 001 u64) as bmb_tables makes them, records.bin a BAM record stream (records back
// to back, each led by its block_size), skip.bin a byte per record, calls.bin 24 u32 per call.  The records are shuffled when
// shuffle_seed is not 0 (the skip bytes with them), cut into n_adds stretches and handed to one bias_counter, one add() per
// stretch; annotate() runs after the first stretch too (its result is dropped: it must not end or disturb the counting) and
// after the last.  Prints "notes N", the annotations (16 numbers each), and per reference "strand" with its four cells per
// position and "mapq" with its one; a refused begin(), add() or annotate() prints "refused <what>" and returns 3.
// The second form prints write_vcf_file's text for calls.bin with the annotations of notes.bin (16 u32 per call) and, on
// stderr, the summary line.
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
        bm::vcf_bias bias;
        bias.notes = words_of(read_file(argv[3]));
        if (bias.notes.size() / bm::kBiasOutWords != res.n_calls()) return 2;
        const uint32_t min_qual = static_cast<uint32_t>(std::stoul(argv[4]));
        bias.max_fs = static_cast<uint32_t>(std::stoul(argv[5]));
        bias.min_mq = static_cast<uint32_t>(std::stoul(argv[6]));
        std::vector<std::string> ids;
        std::vector<uint32_t> lens;
        for (int k = 8; k < argc; k++) {
            const std::string s = argv[k];
            const size_t colon = s.rfind(':');
            ids.push_back(s.substr(0, colon));
            lens.push_back(static_cast<uint32_t>(std::stoul(s.substr(colon + 1))));
        }
        bm::write_vcf_file(std::cout, res, ids, lens, argv[7], min_qual, nullptr, nullptr, nullptr, &bias);
        std::cerr << bm::bias_summary_line(bm::summarize_bias(bias)) << "\n";
        return 0;
    }
    if (argc < 10) return 2;
    const std::vector<uint8_t> raw = read_file(argv[1]);
    bm::bias_tables tables;
    if (raw.size() != bm::kBiasNLf * 4 + bm::kBiasNE * 8) return 2;
    tables.lf.resize(bm::kBiasNLf), tables.e.resize(bm::kBiasNE);
    std::memcpy(tables.lf.data(), raw.data(), bm::kBiasNLf * 4);
    std::memcpy(tables.e.data(), raw.data() + bm::kBiasNLf * 4, bm::kBiasNE * 8);
    const std::vector<uint8_t> stream = read_file(argv[2]);
    std::vector<uint8_t> skip;
    if (std::string(argv[3]) != "-") skip = read_file(argv[3]);
    const std::vector<uint32_t> calls = words_of(read_file(argv[4]));
    const size_t n_adds = std::stoull(argv[5]), n_calls = calls.size() / bm::kBiasCallWords;
    uint64_t seed = std::stoull(argv[6]);
    bm::bias_params pr;
    pr.min_mapq = static_cast<uint32_t>(std::stoul(argv[7]));
    pr.min_bq = static_cast<uint32_t>(std::stoul(argv[8]));
    std::vector<uint32_t> ref_len;
    for (int k = 9; k < argc; k++) ref_len.push_back(static_cast<uint32_t>(std::stoul(argv[k])));

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
        bm::bias_counter counter;
        counter.begin(ref_len.data(), ref_len.size(), pr);
        std::vector<uint32_t> notes;
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
            if (add == 0) counter.annotate(calls.data(), n_calls, tables, notes);
        }
        counter.annotate(calls.data(), n_calls, tables, notes);
        std::string text = "notes " + std::to_string(n_calls) + "\n";
        for (size_t k = 0; k < n_calls; k++)
            for (size_t f = 0; f < bm::kBiasOutWords; f++) text += std::to_string(notes[bm::kBiasOutWords * k + f]) + (f + 1 < bm::kBiasOutWords ? " " : "\n");
        size_t at = 0;
        for (size_t r = 0; r < ref_len.size(); r++) {
            text += "strand";
            for (size_t k = 0; k < static_cast<size_t>(ref_len[r]) * bm::kBiasStrandCells; k++) text += ' ', text += std::to_string(counter.strand_cells()[at * bm::kBiasStrandCells + k]);
            text += "\nmapq";
            for (size_t k = 0; k < ref_len[r]; k++) text += ' ', text += std::to_string(counter.mapq_cells()[at + k]);
            text += "\n";
            at += ref_len[r];
        }
        std::cout << text;
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    return 0;
}
