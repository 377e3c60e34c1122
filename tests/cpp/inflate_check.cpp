// TEST ONLY: host/bgzf_in.h and host/inflate_rule.h -- the lines the inflate kernel runs -- as a program of its own
// (tests/test_inflate.py builds it with -fsanitize=address,undefined).
//   inflate_check <in> [<out>]
// lays <in> out as BGZF and inflates every member; prints ONE line and exits 0 whatever the file holds:
//   ok <bytes> <n_stored> <n_fixed> <n_dynamic>      the text went to <out>
//   format <message>                                 not BGZF framing
//   data <block> <reason>                            the first bad block and its BMU_REASON_*
// Every member's payload and output live in heap buffers of exactly their size, so the sanitizer sees a byte too many.
#include "../../bucket-map_amd/host/bgzf_in.h"

#include <cstdio>
#include <fstream>
#include <iterator>

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<uint8_t> in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<bm::bgzf_member> members;
    std::string error;
    if (!bm::bgzf_layout(in.data(), in.size(), members, error)) {
        std::printf("format %s\n", error.c_str());
        return 0;
    }
    std::vector<uint8_t> text;
    uint32_t n_type[3] = {0, 0, 0};
    for (size_t b = 0; b < members.size(); b++) {
        const bm::bgzf_member &m = members[b];
        const std::vector<uint8_t> payload(in.begin() + static_cast<std::ptrdiff_t>(m.payload),
                                           in.begin() + static_cast<std::ptrdiff_t>(m.payload + m.payload_len));
        std::vector<uint8_t> out(m.isize);
        uint32_t r = bm::inflate_member(payload.data(), m.payload_len, out.data(), m.isize, n_type);
        if (!r && bm::bgzf_detail::crc32(out.data(), out.size()) != m.crc) r = bmu_rule::kCrc;
        if (r) {
            std::printf("data %zu %u\n", b, r);
            return 0;
        }
        text.insert(text.end(), out.begin(), out.end());
    }
    if (argc > 2) {
        std::ofstream o(argv[2], std::ios::binary);
        o.write(reinterpret_cast<const char *>(text.data()), static_cast<std::streamsize>(text.size()));
        if (!o) return 1;
    }
    std::printf("ok %zu %u %u %u\n", text.size(), n_type[0], n_type[1], n_type[2]);
    return 0;
}
