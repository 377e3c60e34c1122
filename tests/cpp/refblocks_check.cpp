// TEST ONLY: host/refblocks.h as a program of its own (tests/test_refblocks.py builds it with -fsanitize=address,undefined).
//   refblocks_check <records.bin> <bases.bin> <bands | -> <exclude.bin | -> <n_calls> <min_mapq> <min_bq> <q_absent> <q_cap> <ref_len>...
//   refblocks_check gvcf <calls.bin> <blocks.bin> <bases.bin> <min_qual> <sample> <name:length>...
// records.bin is a BAM record stream, bases.bin the references' bases back to back, bands a comma list, exclude.bin three u32
// per interval.  The records are cut into n_calls stretches and handed to one genotype_counter; refblocks_of runs after the
// first stretch too (its result is dropped) and after the last.  Prints "blocks N", the blocks (8 numbers each), "counts" with
// n_excluded and n_no_allele, and per reference "conf" and its two words per position; a refusal prints "refused <what>" and
// returns 3.  The second form prints the text of a --gvcf file without indel lines for calls.bin (24 u32 per call) and
// blocks.bin (8 u32 per block), merged as the tools merge them, and the summary line on stderr.
#include "../../bucket-map_amd/host/refblocks.h"

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
    if (argc >= 8 && std::string(argv[1]) == "gvcf") {
        bm::genotype_result res;
        res.calls = words_of(read_file(argv[2]));
        bm::refblock_result blk;
        blk.blocks = words_of(read_file(argv[3]));
        const std::vector<uint8_t> bases = read_file(argv[4]);
        std::vector<std::string> ids;
        std::vector<uint32_t> lens;
        std::vector<const uint8_t *> at;
        size_t total = 0;
        for (int k = 7; k < argc; k++) {
            const std::string s = argv[k];
            const size_t colon = s.rfind(':');
            ids.push_back(s.substr(0, colon));
            lens.push_back(static_cast<uint32_t>(std::stoul(s.substr(colon + 1))));
            at.push_back(bases.data() + total);
            total += lens.back();
        }
        if (total != bases.size()) return 2;
        const uint32_t min_qual = static_cast<uint32_t>(std::stoul(argv[5]));
        size_t next = 0;
        const bm::vcf_between between = [&](std::string &buf, uint32_t ref, uint64_t pos) {
            for (; next < blk.n_blocks(); next++) {
                const uint32_t *b = blk.blocks.data() + bm::kRefBlockWords * next;
                if (b[0] > ref || (b[0] == ref && static_cast<uint64_t>(b[1]) + 1 >= pos)) break;
                bm::append_block_line(buf, b, ids.at(b[0]), at.at(b[0]));
            }
        };
        const char *const more[3] = {bm::gvcf_alt_header(), bm::gvcf_info_header(), bm::gvcf_format_header()};
        bm::write_vcf_file(std::cout, res, ids, lens, argv[6], min_qual, nullptr, &between, more);
        bm::refblock_count_rest(blk, lens, bm::refblock_excluded(res, nullptr, lens));
        std::cerr << bm::refblock_summary_line(blk, lens) << "\n";
        return 0;
    }
    if (argc < 11) return 2;
    const std::vector<uint8_t> stream = read_file(argv[1]), bases = read_file(argv[2]);
    std::vector<uint32_t> bands, exclude;
    if (std::string(argv[3]) != "-") {
        const std::string s = argv[3];
        for (size_t a = 0; a <= s.size();) {
            const size_t e = std::min(s.find(',', a), s.size());
            bands.push_back(static_cast<uint32_t>(std::stoul(s.substr(a, e - a))));
            a = e + 1;
        }
    }
    if (std::string(argv[4]) != "-") exclude = words_of(read_file(argv[4]));
    const size_t n_calls = std::stoull(argv[5]);
    bm::genotype_params pr;
    pr.min_mapq = static_cast<uint32_t>(std::stoul(argv[6]));
    pr.min_bq = static_cast<uint32_t>(std::stoul(argv[7]));
    pr.q_absent = static_cast<uint32_t>(std::stoul(argv[8]));
    pr.q_cap = static_cast<uint32_t>(std::stoul(argv[9]));
    std::vector<uint32_t> ref_len;
    std::vector<const uint8_t *> at;
    size_t total = 0;
    for (int k = 10; k < argc; k++) {
        ref_len.push_back(static_cast<uint32_t>(std::stoul(argv[k])));
        at.push_back(bases.data() + total);
        total += ref_len.back();
    }
    if (total != bases.size()) return 2;
    std::vector<uint64_t> off{0};
    for (size_t a = 0; a < stream.size();) {
        if (stream.size() - a < 4) return 2;
        uint32_t size;
        std::memcpy(&size, stream.data() + a, 4);
        if (size > stream.size() - a - 4) return 2;
        a += 4 + static_cast<size_t>(size);
        off.push_back(a);
    }
    const size_t n = off.size() - 1;
    try {
        bm::genotype_counter counter;
        counter.begin(ref_len.data(), ref_len.size(), pr);
        bm::refblock_result res;
        std::vector<uint32_t> conf;
        for (size_t call = 0; call < n_calls; call++) {
            const size_t lo = n * call / n_calls, hi = n * (call + 1) / n_calls;
            std::vector<uint64_t> part(off.begin() + static_cast<std::ptrdiff_t>(lo), off.begin() + static_cast<std::ptrdiff_t>(hi) + 1);
            for (uint64_t &o : part) o -= off[lo];
            counter.add(stream.data() + off[lo], part.data(), hi - lo, nullptr);
            if (call == 0) bm::refblocks_of(counter.cells(), ref_len, at.data(), bands, exclude, res, &conf);
        }
        bm::refblocks_of(counter.cells(), ref_len, at.data(), bands, exclude, res, &conf);
        std::string text = "blocks " + std::to_string(res.n_blocks()) + "\n";
        for (size_t k = 0; k < res.n_blocks(); k++)
            for (size_t f = 0; f < bm::kRefBlockWords; f++) text += std::to_string(res.blocks[bm::kRefBlockWords * k + f]) + (f + 1 < bm::kRefBlockWords ? " " : "\n");
        text += "counts " + std::to_string(res.n_excluded) + " " + std::to_string(res.n_no_allele) + "\n";
        size_t p = 0;
        for (size_t r = 0; r < ref_len.size(); r++) {
            text += "conf";
            for (size_t k = 0; k < 2 * static_cast<size_t>(ref_len[r]); k++) text += ' ', text += std::to_string(conf[p++]);
            text += "\n";
        }
        std::cout << text;
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    return 0;
}
