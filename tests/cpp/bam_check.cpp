// TEST ONLY: host/bam.h + host/bgzf.h as a program of its own (tests/test_bgzf.py builds it with -fsanitize=address,undefined).
//   bam_check <in.sam> <out.bam>
// The @ lines are the header text (its @SQ lines give the references); every other line goes through sam_line_to_bam.  The
// header is a block of its own, the records are cut every kBgzfBlockMax bytes, then the EOF block -- as sam_text writes it.
#include "../../bucket-map_amd/host/bam.h"
#include "../../bucket-map_amd/host/bgzf.h"

#include <cstdio>
#include <fstream>
#include <iostream>

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::string line, text, head, stream;
    std::vector<std::string> ids;
    std::vector<size_t> lengths;
    std::vector<std::string> records;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '@') {
            text += line + "\n";
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
        for (const std::string &r : records) bm::sam_line_to_bam(r, index, stream);
    } catch (const std::exception &e) {
        std::cerr << e.what() << "\n";
        return 3;
    }
    bm::block_compressor z;
    std::vector<uint8_t> out;
    z.deflate(reinterpret_cast<const uint8_t *>(head.data()), head.size(), out);
    z.deflate(reinterpret_cast<const uint8_t *>(stream.data()), stream.size(), out);
    out.insert(out.end(), bm::kBgzfEof, bm::kBgzfEof + 28);
    std::ofstream o(argv[2], std::ios::binary);
    o.write(reinterpret_cast<const char *>(out.data()), static_cast<std::streamsize>(out.size()));
    return o ? 0 : 1;
}
