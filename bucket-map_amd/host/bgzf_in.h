// bgzf_in.h -- compressed input: the BGZF layout walk, a serial host inflater and the interface behind which the product
// plugs in the device (include/bmu.h).
//
// BGZF is gzip cut into independent members of at most 64 KiB with each member's size in its header (the BC extra
// subfield), so all blocks of a file can be inflated at once.  bgzf_layout() -- which is bmu_layout -- finds the members
// on the host; block_inflater turns a run of whole members into text.  The default is the serial decoder below, built from
// inflate_rule.h, the same lines the kernel runs: it is the inflater of every build without a device behind it (the
// oracle-backed test tools) and of tests/cpp/inflate_check.cpp.  The product plugs in bmu_inflate (gpu_block_inflater.h).
//
// Plain gzip (no BC subfield) is one serial stream: nothing can keep a device busy on it and the project has no CPU path,
// so it is refused with a message that names bgzip.
#pragma once

#include "bgzf.h"
#include "inflate_rule.h"

#include <sys/mman.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace bm {

struct bgzf_member {
    uint64_t at = 0;          // where the member starts in the file
    uint64_t payload = 0;     // ... and its DEFLATE payload
    uint32_t payload_len = 0;
    uint32_t isize = 0;
    uint32_t crc = 0;
};

namespace bgzf_detail {
inline uint32_t le16(const uint8_t *p) { return p[0] | static_cast<uint32_t>(p[1]) << 8; }
inline uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }
}  // namespace bgzf_detail

// The members of in[0, n).  RFC 1952: magic 1f 8b, CM 8, FEXTRA set; the BC subfield of length 2 is found by walking the
// subfields; FNAME, FCOMMENT and FHCRC are skipped; BSIZE + 1 must reach a trailer inside the buffer; ISIZE <= 65536.
// Empty members are legal anywhere.  false: *error says what is wrong and where.
inline bool bgzf_layout(const uint8_t *in, uint64_t n, std::vector<bgzf_member> &members, std::string &error) {
    using bgzf_detail::le16;
    using bgzf_detail::le32;
    members.clear();
    auto fail = [&](uint64_t at, const char *what) {
        error = "not BGZF: " + std::string(what) + " at byte " + std::to_string(at);
        return false;
    };
    for (uint64_t at = 0; at < n;) {
        if (n - at < 18) return fail(at, n - at >= 2 && in[at] == 0x1f && in[at + 1] == 0x8b ? "a truncated member" : "bytes that start no gzip member");
        const uint8_t *h = in + at;
        if (h[0] != 0x1f || h[1] != 0x8b) return fail(at, "bytes that start no gzip member");
        if (h[2] != 8) return fail(at, "a compression method other than deflate");
        const uint32_t flg = h[3];
        if (flg & 0xE0u) return fail(at, "reserved gzip flags");
        if (!(flg & 4u))
            return fail(at, "a gzip member without the BC size field (plain gzip is one serial stream; recompress the file with bgzip)");
        const uint32_t xlen = le16(h + 10);
        if (n - at < 12ull + xlen) return fail(at, "a truncated member");
        int64_t bsize = -1;
        for (uint32_t x = 0; x + 4 <= xlen;) {
            const uint8_t *sf = h + 12 + x;
            const uint32_t slen = le16(sf + 2);
            if (x + 4 + slen > xlen) return fail(at, "an extra subfield that overruns the extra field");
            if (sf[0] == 'B' && sf[1] == 'C' && slen == 2 && bsize < 0) bsize = le16(sf + 4);
            x += 4 + slen;
        }
        if (bsize < 0)
            return fail(at, "a gzip member without the BC size field (plain gzip is one serial stream; recompress the file with bgzip)");
        const uint64_t total = static_cast<uint64_t>(bsize) + 1;
        if (total > n - at) return fail(at, "a member whose BSIZE reaches beyond the end");
        uint64_t p = 12ull + xlen;
        for (uint32_t bit : {8u, 16u}) {                         // FNAME, FCOMMENT: zero-terminated
            if (!(flg & bit)) continue;
            while (p < total && h[p]) p++;
            if (p >= total) return fail(at, "an unterminated name or comment");
            p++;
        }
        if (flg & 2u) p += 2;                                    // FHCRC
        if (p + 8 > total) return fail(at, "a member whose BSIZE leaves no room for the trailer");
        bgzf_member m;
        m.at = at;
        m.payload = at + p;
        m.payload_len = static_cast<uint32_t>(total - 8 - p);
        m.crc = le32(h + total - 8);
        m.isize = le32(h + total - 4);
        if (m.isize > 65536) return fail(at, "a member with ISIZE beyond 65536");
        members.push_back(m);
        at += total;
    }
    return true;
}

// One member's payload inflated into out[0, isize): the serial restatement of the kernel (bmu_kernels.hip.h), from the same
// inflate_rule.h.  Returns a bmu_rule reason (kOk: isize bytes were written and the CRC has NOT been looked at yet);
// n_type[0..2] count the stored, fixed and dynamic DEFLATE blocks seen.
inline uint32_t inflate_member(const uint8_t *payload, uint32_t n, uint8_t *out, uint32_t isize, uint32_t n_type[3]) {
    using namespace bmu_rule;
    static thread_local Tables T;
    BitReader br;
    br.buf = payload, br.base = 0, br.limit = n, br.end = n;
    uint32_t at = 0;
    for (;;) {
        br.refill();
        const uint32_t bfinal = br.bits(1), btype = br.bits(2);
        if (br.overrun()) return kTruncated;
        if (btype == 3) return kBadType;
        n_type[btype]++;
        if (btype == 0) {
            uint32_t start = 0, len = 0;
            if (const uint32_t r = read_stored_header(br, &start, &len)) return r;
            if (len > isize - at) return kTooLong;
            if (len) std::memcpy(out + at, payload + start, len);
            at += len;
        } else {
            if (const uint32_t r = btype == 1 ? build_fixed(T) : read_dynamic_header(T, br)) return r;
            for (;;) {
                uint32_t tok = 0;
                const int32_t r = next_token(T, br, &tok);
                if (r < 0) return static_cast<uint32_t>(-r);
                if (r == kEndOfBlock) break;
                if (!(tok & kTokMatch)) {
                    if (at >= isize) return kTooLong;
                    out[at++] = static_cast<uint8_t>(tok);
                    continue;
                }
                const uint32_t len = (tok >> 16) & 0x1FFu, dist = tok & 0xFFFFu;
                if (dist > at) return kDistance;
                if (len > isize - at) return kTooLong;
                for (uint32_t i = 0; i < len; i++, at++) out[at] = out[at - dist];
            }
        }
        if (bfinal) break;
    }
    return at == isize ? kOk : kTooShort;
}

inline const char *inflate_reason_text(uint32_t reason) {
    static const char *const text[] = {"ok", "truncated stream", "invalid block type", "stored LEN/NLEN mismatch", "invalid code",
                                       "distance beyond the start of the block", "output longer than ISIZE", "output shorter than ISIZE",
                                       "CRC mismatch"};
    return reason < 9 ? text[reason] : "unknown";
}

// Who inflates: in[0, n) is a run of whole BGZF members (a piece of a file cut at member borders), out has room for the
// sum of their ISIZEs, which is returned.  Throws std::runtime_error on bytes that are not BGZF and on a bad block (the
// message names the block within the piece and the reason).  The default is the host decoder above.
struct block_inflater {
    virtual ~block_inflater() = default;
    virtual uint64_t inflate(const uint8_t *in, size_t n, uint8_t *out, size_t out_cap) {
        std::vector<bgzf_member> members;
        std::string error;
        if (!bgzf_layout(in, n, members, error)) throw std::runtime_error(error);
        uint64_t at = 0;
        for (size_t b = 0; b < members.size(); b++) {
            const bgzf_member &m = members[b];
            if (m.isize > out_cap - at) throw std::runtime_error("inflate: the output buffer is too small");
            uint32_t n_type[3] = {0, 0, 0};
            uint32_t r = inflate_member(in + m.payload, m.payload_len, out + at, m.isize, n_type);
            if (!r && bgzf_detail::crc32(out + at, m.isize) != m.crc) r = bmu_rule::kCrc;
            if (r) throw std::runtime_error("BGZF block " + std::to_string(b) + " is bad: " + inflate_reason_text(r));
            at += m.isize;
        }
        return at;
    }
};

// The inflater the readers of bm_genome.h use: the host decoder until a tool installs its own (main.cpp does, from
// bm_make_inflater, before the first file is opened).  Not owned.
inline block_inflater *&input_inflater_slot() {
    static block_inflater *current = nullptr;
    return current;
}
inline void set_input_inflater(block_inflater *z) { input_inflater_slot() = z; }   // nullptr: the host decoder again
inline block_inflater *input_inflater() {
    static block_inflater host;
    return input_inflater_slot() ? input_inflater_slot() : &host;
}

inline bool has_gzip_magic(const void *p, size_t n) {
    const uint8_t *b = static_cast<const uint8_t *>(p);
    return n >= 2 && b[0] == 0x1f && b[1] == 0x8b;
}

// A compressed file's text: an anonymous mapping of the layout's total size (release with munmap(text, bytes) when
// bytes > 0), filled piece by piece -- whole members, at most piece_bytes of text each -- so the inflater's buffers do
// not grow with the file.  `what` names the file in errors; a bad block is reported by its number in the FILE.
struct inflated_text {
    char *text = nullptr;
    size_t bytes = 0;
};
inline inflated_text inflate_file(const uint8_t *in, size_t n, const std::string &what, size_t piece_bytes = 256u << 20) {
    std::vector<bgzf_member> members;
    std::string error;
    if (!bgzf_layout(in, n, members, error)) throw std::runtime_error(what + " is " + error);
    uint64_t total = 0;
    for (const bgzf_member &m : members) total += m.isize;
    inflated_text t;
    t.bytes = static_cast<size_t>(total);
    if (!total) return t;
    void *map = ::mmap(nullptr, t.bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (map == MAP_FAILED) throw std::runtime_error("no memory for the " + std::to_string(total) + " bytes of text in " + what);
    t.text = static_cast<char *>(map);
    block_inflater *z = input_inflater();
    uint64_t out_at = 0;
    for (size_t b0 = 0; b0 < members.size();) {
        size_t b1 = b0;
        uint64_t piece = 0;
        while (b1 < members.size() && (b1 == b0 || piece + members[b1].isize <= piece_bytes)) piece += members[b1++].isize;
        const uint64_t in0 = members[b0].at, in1 = b1 < members.size() ? members[b1].at : n;
        try {
            const uint64_t got = z->inflate(in + in0, static_cast<size_t>(in1 - in0), reinterpret_cast<uint8_t *>(t.text) + out_at,
                                            static_cast<size_t>(piece));
            if (got != piece) throw std::runtime_error("inflate returned " + std::to_string(got) + " bytes for " + std::to_string(piece));
        } catch (const std::exception &e) {
            ::munmap(map, t.bytes);
            throw std::runtime_error(what + " (compressed, blocks from " + std::to_string(b0) + "): " + e.what());
        }
        out_at += piece;
        b0 = b1;
    }
    return t;
}

}  // namespace bm
