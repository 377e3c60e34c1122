// inflate_rule.h -- the serial parts of an RFC 1951 decoder, written once for the host and for the device: the bit reader,
// table construction with its validity checks, the code-length header of a dynamic block and single-symbol decode.
//
// No HIP dependency: plain C++ for the host decoder (bgzf_in.h) and the stand-alone check (tests/cpp/inflate_check.cpp),
// __host__ __device__ when hipcc compiles it for the kernel (csrc/bmu_kernels.hip.h), which runs these same lines on one
// lane with the tables and the input window in LDS.
//
// What it accepts is what zlib accepts: stored, fixed and dynamic blocks in any mix, codes up to 15 bits, the run symbols
// 16/17/18 (a run may cross from the literal/length lengths into the distance lengths), a literal/length or distance code
// that is complete or consists of ONE code of length 1, and a distance code without any code (a block of literals only).
// Everything else ends in a reason code; no table write is indexed by a length that has not passed the Kraft check, and
// every loop is bounded by the symbols of a header or, in the callers, by the bits of the member and the bytes to ISIZE.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define BMU_HD __host__ __device__
#else
#define BMU_HD
#endif

namespace bmu_rule {

// why a block was refused (BMU_REASON_* in include/bmu.h)
enum : uint32_t {
    kOk = 0,
    kTruncated = 1,     // the stream needs bits beyond the member's payload
    kBadType = 2,       // BTYPE 11
    kStoredLen = 3,     // LEN != ~NLEN
    kBadCode = 4,       // oversubscribed, incomplete or otherwise invalid code, or a bit pattern no code has
    kDistance = 5,      // a match reaches back beyond the start of the block's output
    kTooLong = 6,       // the stream produces more than ISIZE bytes
    kTooShort = 7,      // ... or fewer
    kCrc = 8            // the output's CRC32 is not the trailer's
};

constexpr uint32_t kFastBits = 10, kMaxBits = 15, kMaxLitLen = 288, kMaxDist = 32, kMaxLens = kMaxLitLen + kMaxDist;

// Bits of the payload, least significant first.  The payload's bytes [base, limit) lie at buf[0, limit - base): the whole
// payload on the host (base 0, limit = end), a window that the kernel slides on the device (the caller never lets a read
// get within 8 bytes of a limit that is not the end).  Beyond `end` zero bits are fed and counted: overrun() tells.
struct BitReader {
    const uint8_t *buf = nullptr;
    uint32_t base = 0, limit = 0, end = 0;
    uint32_t next = 0;       // the next byte to enter acc
    uint32_t have = 0;
    uint64_t acc = 0;

    BMU_HD void refill() {
        if (have > 56) return;
        if (next + 8 <= limit) {
            // eight bytes at once (little-endian, as the rest of the tool): whole bytes are counted, and the bits that land
            // above `have` are the stream's own, ORed in again -- the same bits -- by the refill that counts their byte
            uint64_t w;
            __builtin_memcpy(&w, buf + (next - base), 8);
            acc |= w << have;
            const uint32_t n = (63u - have) >> 3;
            next += n;
            have += 8u * n;
            return;
        }
        while (have <= 56) {
            uint64_t b = 0;
            if (next < limit) b = buf[next - base];
            else if (limit < end) break;
            acc |= b << have;
            have += 8;
            next++;
        }
    }
    BMU_HD uint32_t peek(uint32_t n) const { return static_cast<uint32_t>(acc) & ((1u << n) - 1u); }
    BMU_HD void drop(uint32_t n) {
        acc >>= n;
        have -= n;
    }
    // n <= 16; the caller refills often enough that 16 bits are there
    BMU_HD uint32_t bits(uint32_t n) {
        const uint32_t v = peek(n);
        drop(n);
        return v;
    }
    BMU_HD uint32_t consumed_bits() const { return 8u * next - have; }
    BMU_HD bool overrun() const { return consumed_bits() > 8u * end; }
};

// One canonical code: codes of up to kFastBits bits are looked up in `fast` (symbol << 4 | length, indexed by the next
// bits as they lie in the stream; 0 = not a short code), longer ones are found length by length from count/sym.
struct Huff {
    uint16_t fast[1u << kFastBits];
    uint16_t count[kMaxBits + 1], offs[kMaxBits + 1], next_code[kMaxBits + 1];
    uint16_t sym[kMaxLitLen];
};

struct Tables {
    Huff ll, d;
    uint8_t lens[kMaxLens];
    uint8_t cl[19];
};

// lens[0, n), n <= 288, every length <= 15.  false: oversubscribed, or incomplete in a way inflate does not accept
// (one_code_ok: no code at all, or one code of length 1).  Nothing is written by index of a length before the check.
BMU_HD inline bool build(Huff &h, const uint8_t *lens, uint32_t n, bool one_code_ok) {
    for (uint32_t l = 0; l <= kMaxBits; l++) h.count[l] = 0;
    for (uint32_t s = 0; s < n; s++) h.count[lens[s] & 15u]++;
    int32_t left = 1;
    for (uint32_t l = 1; l <= kMaxBits; l++) {
        left = left * 2 - static_cast<int32_t>(h.count[l]);
        if (left < 0) return false;
    }
    const uint32_t n_codes = n - h.count[0];
    if (left > 0 && !(one_code_ok && (n_codes == 0 || (n_codes == 1 && h.count[1] == 1)))) return false;
    uint32_t code = 0;
    h.offs[0] = 0, h.offs[1] = 0, h.next_code[0] = 0;
    for (uint32_t l = 1; l <= kMaxBits; l++) {
        code = (code + (l > 1 ? h.count[l - 1] : 0u)) << 1;
        h.next_code[l] = static_cast<uint16_t>(code);
        if (l < kMaxBits) h.offs[l + 1] = static_cast<uint16_t>(h.offs[l] + h.count[l]);
    }
    for (uint32_t i = 0; i < (1u << kFastBits); i++) h.fast[i] = 0;
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = lens[s] & 15u;
        if (!l) continue;
        h.sym[h.offs[l]++] = static_cast<uint16_t>(s);          // offs[l] + count[l] <= n_codes <= 288
        const uint32_t c = h.next_code[l]++;
        if (l > kFastBits) continue;
        uint32_t r = 0;
        for (uint32_t k = 0; k < l; k++) r |= ((c >> k) & 1u) << (l - 1 - k);
        for (uint32_t j = r; j < (1u << kFastBits); j += 1u << l) h.fast[j] = static_cast<uint16_t>(s << 4 | l);
    }
    return true;
}

// The next symbol, or -1 when the next 15 bits are no code.  Needs 15 bits in acc (zero bits beyond the end count).
BMU_HD inline int32_t decode(const Huff &h, BitReader &br) {
    const uint32_t e = h.fast[br.peek(kFastBits)];
    if (e) {
        br.drop(e & 15u);
        return static_cast<int32_t>(e >> 4);
    }
    uint32_t code = 0, first = 0, index = 0;
    const uint32_t v = br.peek(kMaxBits);
    for (uint32_t len = 1; len <= kMaxBits; len++) {
        code |= (v >> (len - 1)) & 1u;
        const uint32_t cnt = h.count[len];
        if (code < first + cnt) {                                // code >= first always
            br.drop(len);
            return h.sym[index + (code - first)];
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

BMU_HD inline void fixed_lengths(uint8_t *lens) {
    for (uint32_t s = 0; s < kMaxLitLen; s++) lens[s] = static_cast<uint8_t>(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    for (uint32_t s = 0; s < kMaxDist; s++) lens[kMaxLitLen + s] = 5;
}

BMU_HD inline uint32_t build_fixed(Tables &T) {
    fixed_lengths(T.lens);
    return build(T.ll, T.lens, kMaxLitLen, false) && build(T.d, T.lens + kMaxLitLen, kMaxDist, false) ? kOk : kBadCode;
}

BMU_HD inline uint32_t cl_order(uint32_t i) {
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return static_cast<uint32_t>((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// The header of a dynamic block, from HLIT on, and both tables.  At most 14 + 57 + 316 * 14 bits: the caller has 1 KiB of
// window ahead.  *run_syms gets bit k set when run symbol 16 + k was used (statistics only).
BMU_HD inline uint32_t read_dynamic_header(Tables &T, BitReader &br, uint32_t *run_syms = nullptr) {
    br.refill();
    const uint32_t hlit = br.bits(5) + 257, hdist = br.bits(5) + 1, hclen = br.bits(4) + 4;
    if (hlit > 286 || hdist > 30) return kBadCode;
    for (uint32_t i = 0; i < 19; i++) T.cl[i] = 0;
    for (uint32_t i = 0; i < hclen; i++) {
        br.refill();
        T.cl[cl_order(i)] = static_cast<uint8_t>(br.bits(3));
    }
    if (br.overrun()) return kTruncated;
    if (!build(T.d, T.cl, 19, false)) return kBadCode;           // the distance table's room serves the code-length code
    const uint32_t n = hlit + hdist;
    for (uint32_t i = 0; i < n;) {
        br.refill();
        const int32_t s = decode(T.d, br);
        if (br.overrun()) return kTruncated;
        if (s < 0) return kBadCode;
        if (s < 16) {
            T.lens[i++] = static_cast<uint8_t>(s);
            continue;
        }
        uint32_t rep, val = 0;
        if (s == 16) {
            if (i == 0) return kBadCode;
            val = T.lens[i - 1];
            rep = 3 + br.bits(2);
        } else if (s == 17) {
            rep = 3 + br.bits(3);
        } else {
            rep = 11 + br.bits(7);
        }
        if (run_syms) *run_syms |= 1u << (s - 16);
        if (br.overrun()) return kTruncated;
        if (i + rep > n) return kBadCode;
        for (; rep; rep--) T.lens[i++] = static_cast<uint8_t>(val);
    }
    if (T.lens[256] == 0) return kBadCode;                       // no end-of-block code
    if (!build(T.ll, T.lens, hlit, true)) return kBadCode;
    if (!build(T.d, T.lens + hlit, hdist, true)) return kBadCode;
    return kOk;
}

BMU_HD inline uint32_t len_base(uint32_t s, uint32_t *extra) {   // s = symbol - 257, 0..28
    if (s < 8 || s == 28) {
        *extra = 0;
        return s == 28 ? 258u : 3u + s;
    }
    const uint32_t e = (s >> 2) - 1;
    *extra = e;
    return 3u + ((4u + (s & 3u)) << e);
}
BMU_HD inline uint32_t dist_base(uint32_t s, uint32_t *extra) {  // 0..29
    if (s < 4) {
        *extra = 0;
        return 1u + s;
    }
    const uint32_t e = (s >> 1) - 1;
    *extra = e;
    return 1u + ((2u + (s & 1u)) << e);
}

constexpr uint32_t kTokMatch = 1u << 31;     // a token: a literal is its byte; a match is bit 31 | length << 16 | distance
constexpr int32_t kEndOfBlock = 1;

// One literal, match or end-of-block of a Huffman block: 0 with *tok set, kEndOfBlock, or -(reason).  At most 48 bits.
BMU_HD inline int32_t next_token(const Tables &T, BitReader &br, uint32_t *tok) {
    br.refill();
    const int32_t s = decode(T.ll, br);
    if (s < 0) return br.overrun() ? -static_cast<int32_t>(kTruncated) : -static_cast<int32_t>(kBadCode);
    if (s < 256) {
        *tok = static_cast<uint32_t>(s);
        return br.overrun() ? -static_cast<int32_t>(kTruncated) : 0;
    }
    if (s == 256) return br.overrun() ? -static_cast<int32_t>(kTruncated) : kEndOfBlock;
    if (s > 285) return -static_cast<int32_t>(kBadCode);
    uint32_t extra;
    uint32_t len = len_base(static_cast<uint32_t>(s) - 257u, &extra);
    len += br.bits(extra);
    const int32_t ds = decode(T.d, br);
    if (ds < 0 || ds > 29) return br.overrun() ? -static_cast<int32_t>(kTruncated) : -static_cast<int32_t>(kBadCode);
    uint32_t dist = dist_base(static_cast<uint32_t>(ds), &extra);
    dist += br.bits(extra);
    if (br.overrun()) return -static_cast<int32_t>(kTruncated);
    *tok = kTokMatch | len << 16 | dist;
    return 0;
}

// The header of a stored block, after BTYPE: on kOk the LEN bytes start at payload byte *start and the reader stands
// behind them with an empty accumulator.
BMU_HD inline uint32_t read_stored_header(BitReader &br, uint32_t *start, uint32_t *len) {
    br.drop(br.have & 7u);
    br.refill();
    const uint32_t n = br.bits(16);
    br.refill();
    const uint32_t nn = br.bits(16);
    if (br.overrun()) return kTruncated;
    if ((n ^ 0xFFFFu) != nn) return kStoredLen;
    const uint32_t at = br.next - br.have / 8;                   // have is a multiple of 8 here
    if (at + n > br.end) return kTruncated;
    *start = at, *len = n;
    br.next = at + n, br.acc = 0, br.have = 0;
    return kOk;
}

}  // namespace bmu_rule
