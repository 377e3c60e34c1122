// left_align_check.cpp -- host/left_align.h (bmv_leftalign's contract restated for the host) as a stand-alone program for
// a sanitizer build: the hand-worked cases of include/bmv.h's rule on both strands, then seeded random paths over a two-letter
// alphabet.  Every case is checked for the contract's invariants and idempotence, and printed on one line
//   window query text_rc begin cigar -> begin cigar changed dropped
// so that tests/test_leftalign.py can hold the output against its own restatement.  Exit status 0: all held.
#include "../../bucket-map_amd/host/left_align.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

using entries = std::vector<uint32_t>;

std::string text(const entries &e) {
    std::string s;
    for (const uint32_t x : e) s += std::to_string(x >> 4) + "MID"[x & 15u];
    return s.empty() ? "*" : s;
}

entries parse(const char *s) {
    entries e;
    while (*s) {
        char *end;
        const unsigned long len = std::strtoul(s, &end, 10);
        e.push_back(static_cast<uint32_t>(len << 4) | (*end == 'M' ? 0u : *end == 'I' ? 1u : 2u));
        s = end + 1;
    }
    return e;
}

std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}

int failures = 0;

void fail(const char *what, const std::string &line) {
    std::fprintf(stderr, "FAILED (%s): %s\n", what, line.c_str());
    failures++;
}

struct outcome {
    uint32_t begin, dropped;
    uint8_t changed;
    entries cigar;
};

outcome run(const std::string &window, const std::string &query, uint8_t rc, uint32_t begin, const entries &cigar) {
    const uint64_t text_start = 0, query_start = 0, offset[2] = {0, cigar.size()};
    const uint32_t text_len = static_cast<uint32_t>(window.size()), query_len = static_cast<uint32_t>(query.size());
    bm::left_alignment out;
    bm::leftalign::left_align_on_host(reinterpret_cast<const uint8_t *>(window.data()), reinterpret_cast<const uint8_t *>(query.data()),
                                      &text_start, &text_len, &rc, &query_start, &query_len, &begin, offset, cigar.data(), 1, out);
    return {out.begin[0], out.dropped[0], out.changed[0], out.cigar};
}

// one case: run, the invariants, idempotence, the line
outcome check(const std::string &window, const std::string &query, uint8_t rc, uint32_t begin, const entries &cigar) {
    const outcome got = run(window, query, rc, begin, cigar);
    const std::string line = window + " " + query + " " + std::to_string(rc) + " " + std::to_string(begin) + " " + text(cigar) + " -> " +
                             std::to_string(got.begin) + " " + text(got.cigar) + " " + std::to_string(got.changed) + " " + std::to_string(got.dropped);
    std::puts(line.c_str());
    uint64_t in_query = 0, in_text = 0, gaps = 0;
    for (const uint32_t e : got.cigar) {
        if ((e & 15u) != 2u) in_query += e >> 4;
        if ((e & 15u) != 1u) in_text += e >> 4;
    }
    for (const uint32_t e : cigar) gaps += (e & 15u) != 0u;
    if (in_query != query.size()) fail("M + I lengths", line);
    if (got.begin + in_text > window.size()) fail("leaves the window", line);
    for (size_t i = 1; i < got.cigar.size(); i++)
        if ((got.cigar[i] & 15u) == (got.cigar[i - 1] & 15u)) fail("adjacent entries share an op", line);
    if (!got.cigar.empty() && ((got.cigar.front() & 15u) == 2u || (got.cigar.back() & 15u) == 2u)) fail("begins or ends with D", line);
    if (got.cigar.size() > cigar.size() + gaps) fail("more than E + gaps entries", line);
    if (got.changed != (got.begin != begin || got.cigar != cigar)) fail("changed", line);
    const outcome again = run(window, query, rc, got.begin, got.cigar);
    if (again.begin != got.begin || again.cigar != got.cigar || again.changed || again.dropped) fail("not idempotent", line);
    return got;
}

struct hand_case {
    const char *window, *query, *given, *result;
    uint32_t pos, dropped;
};

const hand_case kCases[] = {
    {"ACGTAAAAAAGTCC", "ACGTAAAAGTCC", "8M2D4M", "4M2D8M", 0, 0},
    {"GGCAGCAGCAGTT", "GGCAGCAGCAGCAGTT", "11M3I2M", "1M3I12M", 0, 0},
    {"CGTAAAAAAAAGC", "CGTAAAAAAGC", "4M1D2M1D5M", "3M2D8M", 0, 0},
    {"AAAAACGT", "AAACGT", "2M2D4M", "6M", 2, 2},
    {"AAAAGG", "AAAAAGG", "4M1I2M", "1I6M", 0, 0},
    {"CCAAAAGG", "CCTAAGG", "2M1I2D4M", "2M1I2D4M", 0, 0},
    {"GATATATC", "GATATC", "5M2D1M", "1M2D5M", 0, 0},
    {"GACATATC", "GACATC", "5M2D1M", "3M2D3M", 0, 0},
};

uint64_t state = 0x9E3779B97F4A7C15ull;
uint32_t next(uint32_t below) {                                 // a small generator of the program's own: the same cases everywhere
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>((state >> 33) % below);
}

}  // namespace

int main() {
    for (const hand_case &c : kCases) {
        const std::string window = c.window, query = c.query;
        const entries given = parse(c.given), want = parse(c.result);
        const outcome f = check(window, query, 0, 0, given);
        if (f.begin != c.pos || f.cigar != want || f.dropped != c.dropped) fail("hand case, forward", window);
        // the same event read from the other strand: the aligner saw the reverse complement of the window
        const outcome r = check(window, revcomp(query), 1, 0, entries(given.rbegin(), given.rend()));
        uint32_t ref = 0;
        for (const uint32_t e : want) ref += (e & 15u) != 1u ? e >> 4 : 0u;
        if (r.begin != window.size() - c.pos - ref || r.cigar != entries(want.rbegin(), want.rend()) || r.dropped != c.dropped)
            fail("hand case, reverse", window);
    }
    for (int k = 0; k < 400; k++) {
        entries cigar;
        uint32_t last = 3, in_query = 0, in_text = 0;
        const uint32_t count = 1 + next(7);
        for (uint32_t i = 0; i < count; i++) {
            uint32_t op = next(3);
            while (op == last) op = next(3);
            const uint32_t len = 1 + next(op == 0 ? 11 : 4);
            cigar.push_back(len << 4 | op);
            if (op != 2u) in_query += len;
            if (op != 1u) in_text += len;
            last = op;
        }
        const uint32_t begin = next(4);
        std::string window(begin + in_text + next(4), 'A'), query(in_query, 'A');
        for (char &c : window) c = "AC"[next(2)];
        for (char &c : query) c = "AC"[next(2)];
        check(window, query, static_cast<uint8_t>(next(2)), begin, cigar);
    }
    if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
    return failures ? 1 : 0;
}
