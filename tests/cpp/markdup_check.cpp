// TEST ONLY: host/markdup.h and host/bam_sort.h in mark mode, with the host compressor, as a program of its own
// (tests/test_markdup.py builds it with -fsanitize=address,undefined).
//   markdup_check <in.sam> <out.bam> [run_bytes]
// The @ lines are the header text, its first line rewritten to say SO:coordinate (its @SQ lines give the references); every
// other line goes through sam_line_to_bam and into a bam_sorter in mark mode with runs of run_bytes (default: one run).  Writes
// out.bam and out.bam.bai as sam_text does with --markdup, and prints "records runs pair_units fragment_units
// duplicates_from_pairs duplicate_fragments".
#include "../../bucket-map_amd/host/bam.h"
#include "../../bucket-map_amd/host/bam_sort.h"

#include <fstream>
#include <iostream>

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const size_t run_bytes = argc > 3 ? std::stoull(argv[3]) : ~size_t{0} >> 1;
    std::ifstream in(argv[1], std::ios::binary);
    std::string line, text, head;
    std::vector<std::string> ids, records;
    std::vector<size_t> lengths;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '@') {
            text += line.rfind("@HD", 0) == 0 ? std::string("@HD\tVN:1.6\tSO:coordinate\n") : line + "\n";
            if (line.rfind("@SQ\tSN:", 0) == 0) {
                const size_t tab = line.find('\t', 7);
                ids.push_back(line.substr(7, tab - 7));
                lengths.push_back(std::stoul(line.substr(tab + 4)));
            }
        } else if (!line.empty()) {
            records.push_back(line);
        }
    }
    try {
        bm::bam_ref_index index;
        bm::bam_header(text, ids, lengths, head, index);
        bm::block_compressor z;
        std::vector<uint8_t> blocks;
        z.deflate(reinterpret_cast<const uint8_t *>(head.data()), head.size(), blocks);
        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char *>(blocks.data()), static_cast<std::streamsize>(blocks.size()));
        bm::bam_sorter sorter(&z, argv[2], run_bytes, true);
        std::string stream;
        for (const std::string &r : records) {             // a few records a call, as the flushes of sam_text hand them over
            bm::sam_line_to_bam(r, index, stream);
            if (stream.size() > 1000) {
                sorter.add(reinterpret_cast<const uint8_t *>(stream.data()), stream.size());
                stream.clear();
            }
        }
        sorter.add(reinterpret_cast<const uint8_t *>(stream.data()), stream.size());
        sorter.finish(o, blocks.size(), ids.size());
        o.close();
        if (!o) return 1;
        const uint64_t *c = sorter.dup_counts();
        std::cout << sorter.n_records() << " " << sorter.n_runs() << " " << c[0] << " " << c[1] << " " << c[2] << " " << c[3] << "\n";
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 3;
    }
    return 0;
}
