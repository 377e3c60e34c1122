// bam.h -- SAM text to BAM: the header, and one record from its formatted SAM line.
//
// Encoding from the line keeps every call site and every option of the tools as it is, and guarantees that the BAM holds
// what the SAM would have held (tests/test_bgzf.py decodes the BAM back to text and compares).  The BGZF layer that
// carries the stream is host/bgzf.h / include/bmz.h.
#pragma once

#include <charconv>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace bm {

using bam_ref_index = std::unordered_map<std::string, int32_t>;

namespace bam_detail {

inline void put_u16(std::string &out, uint32_t v) { out.push_back(static_cast<char>(v)), out.push_back(static_cast<char>(v >> 8)); }
inline void put_u32(std::string &out, uint32_t v) {
    for (int k = 0; k < 4; k++) out.push_back(static_cast<char>(v >> (8 * k)));
}
inline void set_u32(std::string &out, size_t at, uint32_t v) {
    for (int k = 0; k < 4; k++) out[at + k] = static_cast<char>(v >> (8 * k));
}
[[noreturn]] inline void bad(std::string_view line, const std::string &what) {
    throw std::runtime_error("cannot write this record as BAM (" + what + "): " + std::string(line.substr(0, std::min<size_t>(line.size(), 200))));
}
inline int64_t integer(std::string_view s, std::string_view line, const char *field) {
    int64_t v = 0;
    const auto r = std::from_chars(s.data(), s.data() + s.size(), v);
    if (s.empty() || r.ec != std::errc() || r.ptr != s.data() + s.size()) bad(line, std::string(field) + " is not a number");
    return v;
}

}  // namespace bam_detail

// SAM spec 5.3: the smallest bin that holds [beg, end), 0-based half-open
inline uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return static_cast<uint32_t>(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return static_cast<uint32_t>(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return static_cast<uint32_t>(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return static_cast<uint32_t>(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return static_cast<uint32_t>(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// magic, l_text, the header text exactly as given, n_ref and the references; fills ref_index (name -> refID)
inline void bam_header(std::string_view text, const std::vector<std::string> &ref_ids, const std::vector<size_t> &ref_lengths,
                       std::string &out, bam_ref_index &ref_index) {
    using namespace bam_detail;
    out.append("BAM\1", 4);
    put_u32(out, static_cast<uint32_t>(text.size()));
    out.append(text);
    put_u32(out, static_cast<uint32_t>(ref_ids.size()));
    ref_index.clear();
    for (size_t i = 0; i < ref_ids.size(); i++) {
        put_u32(out, static_cast<uint32_t>(ref_ids[i].size() + 1));
        out.append(ref_ids[i]);
        out.push_back('\0');
        put_u32(out, static_cast<uint32_t>(ref_lengths[i]));
        ref_index.emplace(ref_ids[i], static_cast<int32_t>(i));   // the first of equal names, as a reader resolves them
    }
}

// One alignment record, appended to out, from its SAM line (with or without the trailing newline).
inline void sam_line_to_bam(std::string_view line, const bam_ref_index &ref_index, std::string &out) {
    using namespace bam_detail;
    if (!line.empty() && line.back() == '\n') line.remove_suffix(1);
    std::string_view f[11];
    size_t at = 0;
    for (int k = 0; k < 11; k++) {
        const size_t tab = line.find('\t', at);
        if (k < 10 && tab == std::string_view::npos) bad(line, "fewer than 11 fields");
        f[k] = line.substr(at, tab == std::string_view::npos ? std::string_view::npos : tab - at);
        at = tab == std::string_view::npos ? line.size() : tab + 1;
    }
    const std::string_view tags = at < line.size() ? line.substr(at) : std::string_view{};
    auto ref_id = [&](std::string_view name, const char *field) -> int32_t {
        if (name == "*") return -1;
        const auto it = ref_index.find(std::string(name));
        if (it == ref_index.end()) bad(line, std::string(field) + " names no @SQ line");
        return it->second;
    };
    const std::string_view qname = f[0];
    if (qname.empty() || qname.size() > 254) bad(line, "QNAME must be 1..254 characters");
    const int64_t flag = integer(f[1], line, "FLAG"), pos = integer(f[3], line, "POS") - 1, mapq = integer(f[4], line, "MAPQ"),
                  pnext = integer(f[7], line, "PNEXT") - 1, tlen = integer(f[8], line, "TLEN");
    if (flag < 0 || flag > 0xFFFF || mapq < 0 || mapq > 255 || pos < -1 || pos > 0x7FFFFFFF || pnext < -1 || pnext > 0x7FFFFFFF ||
        tlen < INT32_MIN || tlen > INT32_MAX)
        bad(line, "a number beyond its BAM field");
    const int32_t rid = ref_id(f[2], "RNAME"), next_rid = f[6] == "=" ? rid : ref_id(f[6], "RNEXT");

    std::vector<uint32_t> cigar;
    uint64_t ref_len = 0;
    if (f[5] != "*") {
        uint64_t n = 0;
        bool digits = false;
        for (char ch : f[5]) {
            if (ch >= '0' && ch <= '9') {
                n = n * 10 + static_cast<uint64_t>(ch - '0');
                digits = true;
                if (n >= (1u << 28)) bad(line, "a CIGAR length beyond 2^28");
                continue;
            }
            const size_t op = std::string_view("MIDNSHP=X").find(ch);
            if (op == std::string_view::npos || !digits) bad(line, "CIGAR");
            cigar.push_back(static_cast<uint32_t>(n) << 4 | static_cast<uint32_t>(op));
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += n;
            n = 0, digits = false;
        }
        if (digits) bad(line, "CIGAR");
    }
    const std::string_view seq = f[9] == "*" ? std::string_view{} : f[9];
    if (f[10] != "*" && f[10].size() != seq.size()) bad(line, "SEQ and QUAL differ in length");
    const bool long_cigar = cigar.size() > 65535;

    const size_t start = out.size();
    put_u32(out, 0);                                              // block_size, set below
    put_u32(out, static_cast<uint32_t>(rid));
    put_u32(out, static_cast<uint32_t>(pos));
    out.push_back(static_cast<char>(qname.size() + 1));
    out.push_back(static_cast<char>(mapq));
    put_u16(out, reg2bin(pos, pos + static_cast<int64_t>(ref_len ? ref_len : 1)));
    put_u16(out, long_cigar ? 2u : static_cast<uint32_t>(cigar.size()));
    put_u16(out, static_cast<uint32_t>(flag));
    put_u32(out, static_cast<uint32_t>(seq.size()));
    put_u32(out, static_cast<uint32_t>(next_rid));
    put_u32(out, static_cast<uint32_t>(pnext));
    put_u32(out, static_cast<uint32_t>(static_cast<int32_t>(tlen)));
    out.append(qname);
    out.push_back('\0');
    if (long_cigar) {                                             // the CG:B,I convention: <l_seq>S<ref_len>N here
        put_u32(out, static_cast<uint32_t>(seq.size()) << 4 | 4u);
        put_u32(out, static_cast<uint32_t>(ref_len) << 4 | 3u);
    } else {
        for (uint32_t c : cigar) put_u32(out, c);
    }
    static const auto code = [] {
        std::vector<uint8_t> t(256, 15);
        const char *alphabet = "=ACMGRSVTWYHKDBN";
        for (int i = 0; i < 16; i++) {
            t[static_cast<uint8_t>(alphabet[i])] = static_cast<uint8_t>(i);
            if (alphabet[i] >= 'A') t[static_cast<uint8_t>(alphabet[i] + 32)] = static_cast<uint8_t>(i);
        }
        return t;
    }();
    for (size_t i = 0; i < seq.size(); i += 2) {
        const uint8_t hi = code[static_cast<uint8_t>(seq[i])], lo = i + 1 < seq.size() ? code[static_cast<uint8_t>(seq[i + 1])] : 0;
        out.push_back(static_cast<char>(hi << 4 | lo));
    }
    if (f[10] == "*") out.append(seq.size(), static_cast<char>(0xFF));
    else
        for (char q : f[10]) out.push_back(static_cast<char>(q - 33));

    for (size_t t = 0; t < tags.size();) {
        size_t e = tags.find('\t', t);
        if (e == std::string_view::npos) e = tags.size();
        const std::string_view tag = tags.substr(t, e - t);
        t = e + 1;
        if (tag.size() < 5 || tag[2] != ':' || tag[4] != ':') bad(line, "tag " + std::string(tag));
        const std::string_view value = tag.substr(5);
        out.append(tag.substr(0, 2));
        switch (tag[3]) {
        case 'i': {
            const int64_t v = integer(value, line, "an integer tag");
            if (v >= -128 && v <= 127) out.push_back('c'), out.push_back(static_cast<char>(v));
            else if (v >= 0 && v <= 255) out.push_back('C'), out.push_back(static_cast<char>(v));
            else if (v >= -32768 && v <= 32767) out.push_back('s'), put_u16(out, static_cast<uint32_t>(v));
            else if (v >= 0 && v <= 65535) out.push_back('S'), put_u16(out, static_cast<uint32_t>(v));
            else if (v >= INT32_MIN && v <= INT32_MAX) out.push_back('i'), put_u32(out, static_cast<uint32_t>(v));
            else if (v >= 0 && v <= 0xFFFFFFFFll) out.push_back('I'), put_u32(out, static_cast<uint32_t>(v));
            else bad(line, "an integer tag beyond 32 bits");
            break;
        }
        case 'Z':
            out.push_back('Z');
            out.append(value);
            out.push_back('\0');
            break;
        case 'A':
            if (value.size() != 1) bad(line, "tag " + std::string(tag));
            out.push_back('A');
            out.push_back(value[0]);
            break;
        default:
            bad(line, "a tag of type " + std::string(1, tag[3]) + ", which the tools never write");
        }
    }
    if (long_cigar) {
        out.append("CGBI", 4);
        put_u32(out, static_cast<uint32_t>(cigar.size()));
        for (uint32_t c : cigar) put_u32(out, c);
    }
    set_u32(out, start, static_cast<uint32_t>(out.size() - start - 4));
}

}  // namespace bm
