// TEST ONLY: host/overlap_clip.h as a program of its own (tests/test_overlap.py builds it with -fsanitize=address,undefined).
//   overlap_check <batch.txt>
// batch.txt, whitespace-separated: the genome's letters; n, match, penalty, with_contig; then per alignment text_start text_len
// text_rc begin mate contig, the query's letters ("-": none), the number of CIGAR entries and per entry op and length.
// Prints per alignment "score clip_left clip_right pos ref_len nm cut", the entries as a CIGAR string and the reference letters
// ("-": none each), then "pairs P bases B"; a refused batch prints "refused <what>" and returns 3.
#include "../../bucket-map_amd/host/overlap_clip.h"

#include <fstream>
#include <iostream>

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string genome, query;
    uint32_t n = 0, match = 0, penalty = 0, with_contig = 0;
    if (!(in >> genome >> n >> match >> penalty >> with_contig)) return 2;
    std::vector<uint64_t> text_start(n), query_start(n), cigar_offset(1, 0);
    std::vector<uint32_t> text_len(n), query_len(n), begin(n), mate(n), contig(n), cigar;
    std::vector<uint8_t> text_rc(n), reads;
    for (uint32_t a = 0; a < n; a++) {
        uint32_t rc = 0, ne = 0;
        if (!(in >> text_start[a] >> text_len[a] >> rc >> begin[a] >> mate[a] >> contig[a] >> query >> ne)) return 2;
        text_rc[a] = static_cast<uint8_t>(rc);
        if (query == "-") query.clear();
        query_start[a] = reads.size();
        query_len[a] = static_cast<uint32_t>(query.size());
        reads.insert(reads.end(), query.begin(), query.end());
        for (uint32_t k = 0; k < ne; k++) {
            uint32_t op = 0, len = 0;
            if (!(in >> op >> len)) return 2;
            cigar.push_back(len << 4 | op);
        }
        cigar_offset.push_back(cigar.size());
    }
    bm::clipping out;
    std::vector<uint32_t> cut;
    uint64_t pairs = 0, bases = 0;
    try {
        bm::clip_overlap_on_host(reinterpret_cast<const uint8_t *>(genome.data()), reads.data(), text_start.data(), text_len.data(),
                                 text_rc.data(), query_start.data(), query_len.data(), begin.data(), cigar_offset.data(), cigar.data(),
                                 mate.data(), with_contig ? contig.data() : nullptr, n, match, penalty, out, cut, pairs, bases);
    } catch (const std::exception &e) {
        std::cout << "refused " << e.what() << "\n";
        return 3;
    }
    for (uint32_t a = 0; a < n; a++) {
        std::string cg, ref(out.ref_bases.begin() + static_cast<std::ptrdiff_t>(out.ref_offset[a]),
                            out.ref_bases.begin() + static_cast<std::ptrdiff_t>(out.ref_offset[a + 1]));
        bm::sam_tags::append_cigar(cg, out.xcigar.data() + out.xcigar_offset[a], static_cast<size_t>(out.xcigar_offset[a + 1] - out.xcigar_offset[a]));
        std::cout << out.score[a] << ' ' << out.clip_left[a] << ' ' << out.clip_right[a] << ' ' << out.pos[a] << ' ' << out.ref_len[a] << ' '
                  << out.nm[a] << ' ' << cut[a] << ' ' << (cg.empty() ? "-" : cg) << ' ' << (ref.empty() ? "-" : ref) << "\n";
    }
    std::cout << "pairs " << pairs << " bases " << bases << "\n";
    return 0;
}
