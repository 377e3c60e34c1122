// bgzf.h -- the BGZF block rule of include/bmz.h as plain C++17: what bmz_deflate computes on the device, byte for byte.
//
// The rule (parse, forms, code construction, wrapper) is stated in include/bmz.h; tests/bgzf_rule.py restates it a third
// time in Python.  This copy is the compressor of every build without a device behind it (the oracle-backed test tools)
// and the reference the device is compared with.  A block's bytes depend on the block's input alone.
#pragma once

#include "depth.h"
#include "pileup.h"
#include "genotype.h"
#include "indel.h"
#include "refblocks.h"
#include "markdup.h"
#include "stats.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace bm {

constexpr uint32_t kBgzfBlockMax = 65280;   // BMZ_BLOCK_MAX
constexpr uint32_t kBgzfT = 256, kBgzfHashBits = 15, kBgzfMinMatch = 4, kBgzfMaxMatch = 258, kBgzfMaxDist = 32768;
constexpr uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

namespace bgzf_detail {

constexpr uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                    4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
constexpr uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

inline uint32_t len_sym(uint32_t len) {
    uint32_t s = 28;
    while (len_base[s] > len) s--;
    return s;
}
inline uint32_t dist_sym(uint32_t dist) {
    uint32_t s = 29;
    while (dist_base[s] > dist) s--;
    return s;
}
inline uint32_t fixed_ll_len(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

// a token: a literal is its byte; a match is bit 31 | length << 15 | distance - 1
inline void parse(const uint8_t *b, uint32_t n, std::vector<uint32_t> &tokens) {
    std::vector<int32_t> cand(n, -1), table(1u << kBgzfHashBits, -1);
    auto hash = [&](uint32_t i) {
        uint32_t v;
        std::memcpy(&v, b + i, 4);   // little-endian hosts only, like the rest of the tool
        return (v * 2654435761u) >> (32 - kBgzfHashBits);
    };
    for (uint32_t lo = 0; lo < n; lo += kBgzfT) {
        const uint32_t hi = std::min(n, lo + kBgzfT);
        for (uint32_t i = lo; i < hi && i + 4 <= n; i++) cand[i] = table[hash(i)];
        for (uint32_t i = lo; i < hi && i + 4 <= n; i++) table[hash(i)] = static_cast<int32_t>(i);
    }
    tokens.clear();
    for (uint32_t p = 0; p < n;) {
        uint32_t len = 0;
        const int32_t c = cand[p];
        if (c >= 0 && p - static_cast<uint32_t>(c) <= kBgzfMaxDist) {
            const uint32_t cap = std::min(kBgzfMaxMatch, n - p);
            while (len < cap && b[c + len] == b[p + len]) len++;
        }
        if (len >= kBgzfMinMatch) {
            tokens.push_back(0x80000000u | len << 15 | (p - static_cast<uint32_t>(c) - 1));
            p += len;
        } else {
            tokens.push_back(b[p]);
            p++;
        }
    }
}

// the rule's code construction over n_sym <= 286 symbols
inline void code_lengths(const uint32_t *freq, uint32_t n_sym, uint32_t max_bits, uint8_t *lens) {
    std::fill(lens, lens + n_sym, uint8_t{0});
    uint32_t order[286], m = 0;
    for (uint32_t s = 0; s < n_sym; s++)
        if (freq[s]) order[m++] = s;
    if (m <= 1) {
        lens[m ? order[0] : 0] = 1;
        return;
    }
    std::sort(order, order + m, [&](uint32_t x, uint32_t y) { return freq[x] != freq[y] ? freq[x] < freq[y] : x < y; });
    uint32_t w[2 * 286], parent[2 * 286], depth[2 * 286];
    for (uint32_t i = 0; i < m; i++) w[i] = freq[order[i]];
    uint32_t a = 0, q = m, nxt = m;
    for (uint32_t k = 0; k + 1 < m; k++) {
        uint32_t pair[2];
        for (int j = 0; j < 2; j++) pair[j] = (a < m && (q >= nxt || w[a] <= w[q])) ? a++ : q++;
        w[nxt] = w[pair[0]] + w[pair[1]];
        parent[pair[0]] = parent[pair[1]] = nxt;
        nxt++;
    }
    depth[2 * m - 2] = 0;
    for (uint32_t node = 2 * m - 2; node-- > 0;) depth[node] = depth[parent[node]] + 1;
    uint32_t count[16] = {0}, kraft = 0;
    for (uint32_t leaf = 0; leaf < m; leaf++) count[std::min(depth[leaf], max_bits)]++;
    for (uint32_t l = 1; l <= max_bits; l++) kraft += count[l] << (max_bits - l);
    while (kraft > (1u << max_bits)) {
        uint32_t bits = max_bits - 1;
        while (count[bits] == 0) bits--;
        count[bits]--;
        count[bits + 1] += 2;
        count[max_bits]--;
        kraft--;
    }
    uint32_t at = 0;
    for (uint32_t l = max_bits; l >= 1; l--)
        for (uint32_t k = 0; k < count[l]; k++) lens[order[at++]] = static_cast<uint8_t>(l);
}

// RFC 1951 3.2.2, the codes bit-reversed as they enter the stream
inline void canonical(const uint8_t *lens, uint32_t n_sym, uint16_t *codes) {
    uint32_t count[17] = {0}, next[17] = {0}, code = 0;
    for (uint32_t s = 0; s < n_sym; s++)
        if (lens[s]) count[lens[s]]++;
    for (uint32_t l = 1; l <= 15; l++) {
        code = (code + count[l - 1]) << 1;
        next[l] = code;
    }
    for (uint32_t s = 0; s < n_sym; s++) {
        codes[s] = 0;
        if (!lens[s]) continue;
        uint32_t c = next[lens[s]]++, r = 0;
        for (uint32_t k = 0; k < lens[s]; k++) r |= ((c >> k) & 1u) << (lens[s] - 1 - k);
        codes[s] = static_cast<uint16_t>(r);
    }
}

struct bit_writer {
    uint8_t *out;
    uint64_t acc = 0;
    uint32_t have = 0;
    size_t at = 0;
    void put(uint32_t value, uint32_t bits) {
        acc |= static_cast<uint64_t>(value) << have;
        have += bits;
        while (have >= 8) {
            out[at++] = static_cast<uint8_t>(acc);
            acc >>= 8;
            have -= 8;
        }
    }
    size_t finish() {
        if (have) out[at++] = static_cast<uint8_t>(acc);
        acc = 0, have = 0;
        return at;
    }
};

inline void put_tokens(bit_writer &w, const std::vector<uint32_t> &tokens, const uint8_t *ll_len, const uint8_t *d_len) {
    uint16_t ll_code[288], d_code[30];
    canonical(ll_len, 288, ll_code);   // 288: the fixed code counts the two symbols deflate never uses
    canonical(d_len, 30, d_code);
    for (uint32_t t : tokens) {
        if (t >> 31) {
            const uint32_t len = (t >> 15) & 0x1FFu, dist = (t & 0x7FFFu) + 1;
            uint32_t s = len_sym(len);
            w.put(ll_code[257 + s], ll_len[257 + s]);
            w.put(len - len_base[s], len_extra[s]);
            s = dist_sym(dist);
            w.put(d_code[s], d_len[s]);
            w.put(dist - dist_base[s], dist_extra[s]);
        } else {
            w.put(ll_code[t], ll_len[t]);
        }
    }
    w.put(ll_code[256], ll_len[256]);
}

inline uint32_t crc32(const uint8_t *p, size_t n) {
    static const auto table = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = c & 1u ? (c >> 1) ^ 0xEDB88320u : c >> 1;
            t[i] = c;
        }
        return t;
    }();
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return ~c;
}

}  // namespace bgzf_detail

// One complete BGZF block for in[0, n), n <= kBgzfBlockMax, written to out (n + 31 bytes of room).  Returns its length;
// *form = 0 stored, 1 fixed, 2 dynamic.  only_form >= 0 forces a form (size comparisons in the tests).
inline size_t bgzf_deflate_block(const uint8_t *in, uint32_t n, uint8_t *out, int *form = nullptr, int only_form = -1) {
    using namespace bgzf_detail;
    std::vector<uint32_t> tokens;
    parse(in, n, tokens);
    uint32_t ll_freq[286] = {0}, d_freq[30] = {0};
    for (uint32_t t : tokens) {
        if (t >> 31) {
            ll_freq[257 + len_sym((t >> 15) & 0x1FFu)]++;
            d_freq[dist_sym((t & 0x7FFFu) + 1)]++;
        } else {
            ll_freq[t]++;
        }
    }
    ll_freq[256]++;
    uint8_t ll_len[288] = {0}, d_len[30], cl_len[19], fixed_ll[288], fixed_d[30];
    code_lengths(ll_freq, 286, 15, ll_len);
    code_lengths(d_freq, 30, 15, d_len);
    for (uint32_t s = 0; s < 288; s++) fixed_ll[s] = static_cast<uint8_t>(fixed_ll_len(s));
    std::fill(fixed_d, fixed_d + 30, uint8_t{5});
    uint32_t hlit = 286, hdist = 30, hclen = 19;
    while (!ll_len[hlit - 1]) hlit--;
    while (!d_len[hdist - 1]) hdist--;
    uint32_t cl_freq[19] = {0};
    for (uint32_t s = 0; s < hlit; s++) cl_freq[ll_len[s]]++;
    for (uint32_t s = 0; s < hdist; s++) cl_freq[d_len[s]]++;
    code_lengths(cl_freq, 19, 7, cl_len);
    while (hclen > 4 && !cl_len[cl_order[hclen - 1]]) hclen--;
    uint64_t extra = 0, fixed_bits = 3, dyn_bits = 3 + 14 + 3 * hclen;
    for (uint32_t s = 0; s < 29; s++) extra += static_cast<uint64_t>(ll_freq[257 + s]) * len_extra[s];
    for (uint32_t s = 0; s < 30; s++) extra += static_cast<uint64_t>(d_freq[s]) * dist_extra[s];
    for (uint32_t s = 0; s < 286; s++) fixed_bits += static_cast<uint64_t>(ll_freq[s]) * fixed_ll[s], dyn_bits += static_cast<uint64_t>(ll_freq[s]) * ll_len[s];
    for (uint32_t s = 0; s < 30; s++) fixed_bits += static_cast<uint64_t>(d_freq[s]) * 5, dyn_bits += static_cast<uint64_t>(d_freq[s]) * d_len[s];
    for (uint32_t l = 0; l < 16; l++) dyn_bits += static_cast<uint64_t>(cl_freq[l]) * cl_len[l];
    const uint64_t size[3] = {5ull + n, (fixed_bits + extra + 7) / 8, (dyn_bits + extra + 7) / 8};
    int f = only_form;
    if (f < 0) {
        f = 0;
        for (int k = 1; k < 3; k++)
            if (size[k] < size[f]) f = k;
    }
    if (form) *form = f;
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    std::memcpy(out, head, 16);
    bit_writer w{out + 18};
    if (f == 0) {
        out[18] = 1;
        out[19] = static_cast<uint8_t>(n), out[20] = static_cast<uint8_t>(n >> 8);
        out[21] = static_cast<uint8_t>(~n), out[22] = static_cast<uint8_t>(~n >> 8);
        if (n) std::memcpy(out + 23, in, n);
        w.at = 5 + n;
    } else if (f == 1) {
        w.put(1, 1);
        w.put(1, 2);
        put_tokens(w, tokens, fixed_ll, fixed_d);
    } else {
        uint16_t cl_code[19];
        canonical(cl_len, 19, cl_code);
        w.put(1, 1);
        w.put(2, 2);
        w.put(hlit - 257, 5);
        w.put(hdist - 1, 5);
        w.put(hclen - 4, 4);
        for (uint32_t k = 0; k < hclen; k++) w.put(cl_len[cl_order[k]], 3);
        for (uint32_t s = 0; s < hlit; s++) w.put(cl_code[ll_len[s]], cl_len[ll_len[s]]);
        for (uint32_t s = 0; s < hdist; s++) w.put(cl_code[d_len[s]], cl_len[d_len[s]]);
        put_tokens(w, tokens, ll_len, d_len);
    }
    const size_t payload = w.finish(), total = 18 + payload + 8;
    out[16] = static_cast<uint8_t>(total - 1), out[17] = static_cast<uint8_t>((total - 1) >> 8);
    const uint32_t crc = crc32(in, n);
    uint8_t *tail = out + 18 + payload;
    for (int k = 0; k < 4; k++) tail[k] = static_cast<uint8_t>(crc >> (8 * k)), tail[4 + k] = static_cast<uint8_t>(n >> (8 * k));
    return total;
}

// The coordinate-sort key of a BAM record (rec points at its block_size): (uint32)refID << 32 | (uint32)(pos + 1), so
// refID = -1 sorts last and pos = -1 before pos = 0.  include/bms.h states the same rule for the device.
inline uint64_t bam_sort_key(const uint8_t *rec) {
    uint32_t ref, pos;
    std::memcpy(&ref, rec + 4, 4);
    std::memcpy(&pos, rec + 8, 4);
    return static_cast<uint64_t>(ref) << 32 | static_cast<uint32_t>(pos + 1u);
}

// Who deflates the BAM stream: blocks are cut by size alone (kBgzfBlockMax bytes, the last one shorter), each becomes one
// BGZF block, appended to `out` in order.  The default is the host rule above; the product plugs in the device
// (gpu_block_compressor in make_mapper_gpu.cpp), whose bytes are the same.
struct block_compressor {
    virtual ~block_compressor() = default;
    virtual void deflate(const uint8_t *in, size_t n, std::vector<uint8_t> &out) {
        for (size_t at = 0; at < n; at += kBgzfBlockMax) {
            const uint32_t len = static_cast<uint32_t>(std::min<size_t>(kBgzfBlockMax, n - at));
            const size_t before = out.size();
            out.resize(before + len + 31);
            out.resize(before + bgzf_deflate_block(in + at, len, out.data() + before));
        }
    }

    // --sort (include/bms.h states the order): the n_records records in[rec_offset[i], rec_offset[i + 1]) in ascending
    // bam_sort_key order, equal keys in the order they came in.  sorted = the sorted stream, perm[k] = the record at place
    // k, sorted_offset[k] = where it starts (n_records + 1 values).  The default is the host's std::stable_sort and a copy;
    // the product plugs in bms_sort.
    virtual void sort_records(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, std::vector<uint8_t> &sorted,
                              std::vector<uint32_t> &perm, std::vector<uint64_t> &sorted_offset) {
        (void)n;
        perm.resize(n_records);
        for (size_t i = 0; i < n_records; i++) perm[i] = static_cast<uint32_t>(i);
        std::vector<uint64_t> key(n_records);
        for (size_t i = 0; i < n_records; i++) key[i] = bam_sort_key(in + rec_offset[i]);
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
        sorted_offset.assign(n_records + 1, 0);
        sorted.resize(n);
        for (size_t k = 0; k < n_records; k++) {
            const uint64_t at = rec_offset[perm[k]], len = rec_offset[perm[k] + 1] - at;
            std::memcpy(sorted.data() + sorted_offset[k], in + at, len);
            sorted_offset[k + 1] = sorted_offset[k] + len;
        }
    }
    // the same sort, then deflate() of the sorted stream, appended to out (bms_sort_deflate in the product: the sorted
    // stream does not leave the device)
    virtual void sort_deflate(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, std::vector<uint8_t> &out,
                              std::vector<uint32_t> &perm, std::vector<uint64_t> &sorted_offset) {
        std::vector<uint8_t> sorted;
        sort_records(in, n, rec_offset, n_records, sorted, perm, sorted_offset);
        deflate(sorted.data(), sorted.size(), out);
    }
    // radix passes of the last sort_records / sort_deflate (the host sort has none)
    virtual uint32_t last_sort_passes() const { return 0; }

    // --markdup (include/bmd.h states the rule): the descriptors of the records -- E or 0, the score, the kind --, the marks
    // from descriptors of any origin with counts = (pair units, fragment units, duplicate records from pair units, duplicate
    // fragment records), and both followed by sort_deflate() of the stream with 0x400 set in the duplicates' flags.  The
    // defaults are the host rule of markdup.h; the product plugs in bmd_ends, bmd_mark and bmd_mark_sort_deflate.
    virtual void dup_ends(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, std::vector<uint64_t> &end,
                          std::vector<uint64_t> &score, std::vector<uint8_t> &kind) {
        (void)n;
        markdup_ends(in, rec_offset, n_records, end, score, kind);
    }
    virtual void dup_mark(const uint64_t *end, const uint64_t *score, const uint8_t *kind, size_t n_records, std::vector<uint8_t> &dup,
                          uint64_t counts[4]) {
        markdup_mark(end, score, kind, n_records, dup, counts);
    }
    virtual void mark_sort_deflate(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, std::vector<uint8_t> &out,
                                   std::vector<uint32_t> &perm, std::vector<uint64_t> &sorted_offset, std::vector<uint8_t> &dup,
                                   uint64_t counts[4]) {
        std::vector<uint64_t> end, score;
        std::vector<uint8_t> kind;
        dup_ends(in, n, rec_offset, n_records, end, score, kind);
        dup_mark(end.data(), score.data(), kind.data(), n_records, dup, counts);
        std::vector<uint8_t> marked(in, in + n);
        for (size_t i = 0; i < n_records; i++)
            if (dup[i]) marked[rec_offset[i] + 19] |= 4;
        sort_deflate(marked.data(), n, rec_offset, n_records, out, perm, sorted_offset);
    }

    // --depth / --coverage (include/bmc.h states the rule): the references, then whole records in any order and over any
    // number of calls (skip, where given, is a byte per record: not 0 leaves the record out), then the runs of equal depth
    // and the seven sums per reference.  The defaults are the host rule of depth.h; the product plugs in bmc_begin, bmc_add
    // and bmc_finish.
    virtual void depth_begin(const uint32_t *ref_len, size_t n_ref) { depth_.begin(ref_len, n_ref); }
    virtual void depth_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        (void)n;
        depth_.add(in, rec_offset, n_records, skip);
    }
    virtual void depth_finish(depth_result &out) { depth_.finish(out); }

    // --pileup (include/bmp.h states the rule): the references with their bases (ref_bases[r]: ref_len[r] bytes) and the four
    // thresholds, then whole records as for depth_add, then the sites and the six sums per reference.  The defaults are the
    // host rule of pileup.h; the product plugs in bmp_begin, bmp_add, bmp_finish and bmp_sites.
    virtual void pileup_begin(const uint32_t *ref_len, size_t n_ref, const uint8_t *const *ref_bases, const pileup_thresholds &th) {
        pileup_.begin(ref_len, n_ref, ref_bases, th);
    }
    virtual void pileup_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        (void)n;
        pileup_.add(in, rec_offset, n_records, skip);
    }
    virtual void pileup_finish(pileup_result &out) { pileup_.finish(out); }

    // --vcf (include/bmg.h states the rule): the references and the five parameters, then whole records as for pileup_add,
    // then the calls of sites as pileup_finish lists them (kGenotypeSiteWords each; kGenotypeCallWords per call).  The defaults
    // are the host rule of genotype.h; the product plugs in bmg_begin, bmg_add and bmg_call.
    virtual void genotype_begin(const uint32_t *ref_len, size_t n_ref, const genotype_params &pr) { genotype_.begin(ref_len, n_ref, pr); }
    virtual void genotype_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        (void)n;
        genotype_.add(in, rec_offset, n_records, skip);
    }
    virtual void genotype_call(const uint32_t *sites, size_t n_sites, std::vector<uint32_t> &out) { genotype_.call(sites, n_sites, out); }

    // --vcf-indels (include/bmn.h states the rule): the references and the five parameters, then whole records as for
    // pileup_add, then the alleles, the calls and the three sums per reference.  The defaults are the host rule of indel.h; the
    // product plugs in bmn_begin, bmn_add, bmn_finish, bmn_alleles and bmn_calls.
    virtual void indel_begin(const uint32_t *ref_len, size_t n_ref, const indel_params &pr) { indel_.begin(ref_len, n_ref, pr); }
    virtual void indel_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        (void)n;
        indel_.add(in, rec_offset, n_records, skip);
    }
    virtual void indel_finish(indel_result &out) { indel_.finish(out); }

    // --vcf-bias (include/bmb.h states the rule): the references and the two parameters, then whole records as for
    // genotype_add, then the annotations of calls as genotype_call writes them (kBiasOutWords per call) from the two tables
    // bmb_tables makes.  The defaults are the host rule of bias.h; the product plugs in bmb_begin, bmb_add and bmb_annotate,
    // whose context has uploaded the same tables.
    virtual void bias_begin(const uint32_t *ref_len, size_t n_ref, const bias_params &pr) { bias_.begin(ref_len, n_ref, pr); }
    virtual void bias_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        (void)n;
        bias_.add(in, rec_offset, n_records, skip);
    }
    virtual void bias_annotate(const uint32_t *calls, size_t n_calls, const bias_tables &tables, std::vector<uint32_t> &out) {
        bias_.annotate(calls, n_calls, tables, out);
    }

    // --vcf-phase (include/bmk.h states the rule): the references, the five parameters and the calls of genotype_call, whose
    // het SNVs are the phase sites (returns their number); then whole records as for genotype_add, in any order and cut
    // anywhere; then the eight words per site and the four sums.  The defaults are the host rule of phase.h; the product plugs
    // in bmk_begin, bmk_add, bmk_finish and bmk_phase.
    virtual size_t phase_begin(const uint32_t *ref_len, size_t n_ref, const phase_params &pr, const uint32_t *calls, size_t n_calls) {
        return phase_.begin(ref_len, n_ref, pr, calls, n_calls);
    }
    virtual void phase_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        (void)n;
        phase_.add(in, rec_offset, n_records, skip);
    }
    virtual void phase_finish(phase_result &out) { phase_.finish(out); }

    // --stats (include/bmq.h states the rule): the two parameters; then whole records as for depth_add, in any order and cut
    // anywhere; then the 35 tallies and the eight tables.  The defaults are the host rule of stats.h; the product plugs in
    // bmq_begin, bmq_add, bmq_finish and bmq_table.
    virtual void stats_begin(const stats_params &pr) { stats_.begin(pr); }
    virtual void stats_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) {
        (void)n;
        stats_.add(in, rec_offset, n_records, skip);
    }
    virtual void stats_finish(stats_result &out) { stats_.finish(out); }

    // --gvcf (include/bmr.h states the rule): after genotype_begin and the genotype_add calls, the reference blocks of the cells
    // they filled, against ref_bases (ref_len[r] bytes each), under the band bounds and outside the excluded intervals (three
    // words each).  The default is the host rule of refblocks.h; the product plugs in bmr_run and bmr_blocks.
    virtual void refblocks(const uint32_t *ref_len, size_t n_ref, const uint8_t *const *ref_bases, const std::vector<uint32_t> &bands,
                           const std::vector<uint32_t> &exclude, refblock_result &out) {
        refblocks_of(genotype_.cells(), std::vector<uint32_t>(ref_len, ref_len + n_ref), ref_bases, bands, exclude, out);
    }

private:
    depth_counter depth_;
    pileup_counter pileup_;
    genotype_counter genotype_;
    indel_caller indel_;
    bias_counter bias_;
    phase_linker phase_;
    stats_counter stats_;
};

}  // namespace bm
