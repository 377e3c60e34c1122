"""The fragment range learned from the data, without a GPU: the surface of bmv_frag_spans / bmv_frag / bmv_paired_begin /
bmv_paired_finish, the contract of the spans restated in numpy (verify.frag_spans) against an independent brute force, the
range from a histogram (verify.frag_range, host/frag_range.h) on hand-worked numbers, and the tools' --frag-auto through the
oracle-backed tool, whose verifier takes alignment_verifier::paired_auto's default (align everything, spans, range and pick on
the host)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_pair import COMP, random_pairs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")
PLAIN_TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle")
B = 2 ** 32 - 1
SMALL_GROUPS = dict(sizes=(0, 1, 1, 1, 2, 3), p_unknown=0.1, span=400)     # random_pairs arguments under which many groups settle


def test_header_binding_and_python_surface():
    from bucket_map_amd import verify
    text = open(os.path.join(ROOT, "include", "bmv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = verify.lib()
    names = ("bmv_frag_spans", "bmv_frag", "bmv_last_frag_stats", "bmv_paired_begin", "bmv_paired_finish")
    for name in names:
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)

    def args(name):
        decl = re.search(rf"{name}\s*\((.*?)\)", text, flags=re.S).group(1)
        return [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert args("bmv_frag_spans") == ["ctx", "text_start", "text_len", "text_rc", "query_len", "edits", "end", "contig", "n",
                                      "group_offset", "n_groups", "cap"]
    assert args("bmv_frag") == ["ctx", "out_span", "out_hist"]
    assert args("bmv_last_frag_stats") == ["ctx", "ms_kernels", "n_informative"]
    assert args("bmv_paired_begin")[-7:] == ["n", "group_offset", "n_groups", "margin", "hint", "contig", "cap"]
    assert args("bmv_paired_finish") == ["ctx", "min_frag", "max_frag", "total_cigar"]
    for name in names:
        assert len(args(name)) == len(verify.SYMBOLS[name][1]), name
    for fn in ("frag_spans", "paired_begin", "paired_finish", "frag_stats"):
        assert callable(getattr(verify.Verifier, fn))
    assert callable(verify.frag_spans) and callable(verify.frag_histogram) and callable(verify.frag_range)
    total = C.c_uint64()
    assert L.bmv_frag_spans(None, None, None, None, None, None, None, None, 0, None, 0, 1000) == 1
    assert b"bmv_frag_spans" in L.bmv_last_error()
    assert L.bmv_frag(None, None, None) == 1
    assert b"bmv_frag" in L.bmv_last_error()
    assert L.bmv_last_frag_stats(None, None, None) == 1
    assert b"bmv_last_frag_stats" in L.bmv_last_error()
    assert L.bmv_paired_begin(None, None, 0, None, None, None, None, None, 0, None, 0, None, None, None, 1000) == 1
    assert b"bmv_paired_begin" in L.bmv_last_error()
    assert L.bmv_paired_finish(None, 1, 1000, C.byref(total)) == 1
    assert b"bmv_paired_finish" in L.bmv_last_error()


# ---- frag_spans against a brute force ----
def brute_spans(ts, tl, trc, ql, edits, end, off, cap, contig=None):
    """bmv_frag_spans' definitions by the book: plain Python integers, sets of loci."""
    def left(a):
        return int(ts[a]) + int(tl[a]) - int(end[a]) if trc[a] else int(ts[a]) + int(end[a]) - int(ql[a])

    def right(a):
        return left(a) + int(ql[a])

    def locus(a):
        return (bool(trc[a]), left(a) if trc[a] else right(a))

    def settled_winner(g):
        known = sorted((int(edits[a]), a) for a in range(int(off[g]), int(off[g + 1])) if edits[a] != B)
        if not known or len({locus(a) for _, a in known}) != 1:
            return None
        return known[0][1]

    out = []
    for p in range((len(off) - 1) // 2):
        i, j = settled_winner(2 * p), settled_winner(2 * p + 1)
        span = 0
        if i is not None and j is not None and bool(trc[i]) != bool(trc[j]) and (contig is None or contig[i] == contig[j]):
            f, r = (j, i) if trc[i] else (i, j)
            if left(f) <= left(r) and right(f) <= right(r) and 1 <= right(r) - left(f) <= cap:
                span = right(r) - left(f)
        out.append(span)
    return out


def frag_edge_cases():
    """Hand-built pairs for cap = 500, each a list of (text_start, text_len, text_rc, query_len, edits, end) per mate, with the
    span they must give.  f(left) is a forward alignment with L = left, r(right) a reverse one with R = right."""
    f = lambda left, m=100, e=0, slack=10: (left - 5, m + slack + 5, 0, m, e, m + 5)                    # noqa: E731
    r = lambda right, m=100, e=0, slack=10: (right - m - slack, m + slack + 5, 1, m, e, m + 5)            # noqa: E731
    return {
        "plain": ([f(1000)], [r(1400)], 400),
        "mate 2 forward": ([r(1400)], [f(1000)], 400),
        "empty first group": ([], [r(1400)], 0),
        "empty second group": ([f(1000)], [], 0),
        "both empty": ([], [], 0),
        "an unknown group": ([f(1000, e=B)], [r(1400)], 0),
        "unknown candidates beside the winner do not unsettle": ([f(3000, e=B), f(1000, e=2), f(7000, e=B)], [r(1400, e=1)], 400),
        "a second known candidate at the same locus: still settled": ([f(1000), (990, 125, 0, 100, 3, 110)], [r(1400)], 400),
        "a second known candidate at another locus: not settled": ([f(1000), f(1050, e=3)], [r(1400)], 0),
        "... in the second group": ([f(1000)], [r(1400), r(1401, e=9)], 0),
        "the same coordinate on the other strand is another locus": ([f(1000), (990, 115, 1, 100, 4, 5)], [r(1400)], 0),    # L = 1 100 = R(f)
        "same strand": ([f(1000)], [f(1300)], 0),
        "both reverse": ([r(1100)], [r(1400)], 0),
        "dovetail: the reverse mate begins left of the forward one": ([f(1000)], [r(1299, m=300)], 0),
        "dovetail: the forward mate ends right of the reverse one": ([f(1000, m=300)], [r(1250)], 0),
        "span exactly cap": ([f(1000)], [r(1500)], 500),
        "span cap + 1": ([f(1000)], [r(1501)], 0),
        "span 1 cannot be proper with real reads, a zero-length pair can": ([(1000, 20, 0, 0, 0, 5)], [(1000, 20, 1, 0, 0, 14)], 1),
        "query_len 0 on both mates at one point: span 0 is not informative": ([(1000, 20, 0, 0, 0, 5)], [(1000, 20, 1, 0, 0, 15)], 0),
        "query_len 0 on one mate": ([(1000, 20, 0, 0, 0, 5)], [r(1400)], 395),
        "negative L": ([(0, 120, 0, 100, 0, 60)], [r(300)], 340),
        "negative L beyond cap": ([(0, 120, 0, 100, 0, 60)], [r(461)], 0),
    }


def flatten_frag(cases):
    ts, tl, trc, ql, ed, en, off = [], [], [], [], [], [], [0]
    for first, second, _ in cases:
        for mate in (first, second):
            for (s, w, rc, m, e, x) in mate:
                ts.append(s); tl.append(w); trc.append(rc); ql.append(m); ed.append(e); en.append(x)
            off.append(len(ts))
    return ts, tl, trc, ql, ed, en, off


def test_frag_spans_edge_cases():
    from bucket_map_amd import verify
    cases = frag_edge_cases()
    ts, tl, trc, ql, ed, en, off = flatten_frag(cases.values())
    got = verify.frag_spans(ts, tl, trc, ql, ed, en, off, 500)
    assert got.dtype == np.uint32
    assert dict(zip(cases, got.tolist())) == {k: c[2] for k, c in cases.items()}
    assert got.tolist() == brute_spans(ts, tl, trc, ql, ed, en, off, 500)
    # two contigs: the plain pair is uninformative, contig=None means one contig
    ctg = np.zeros(len(ts), np.uint32)
    ctg[off[1]] = 7
    on_two = verify.frag_spans(ts, tl, trc, ql, ed, en, off, 500, ctg)
    assert on_two[0] == 0 and on_two[1:].tolist() == got[1:].tolist()
    assert on_two.tolist() == brute_spans(ts, tl, trc, ql, ed, en, off, 500, ctg)
    hist = verify.frag_histogram(got, 500)
    assert hist.dtype == np.uint64 and len(hist) == 501 and hist.sum() == len(cases)
    assert hist[400] == 4 and hist[500] == 1 and hist[1] == 1 and hist[0] == sum(1 for c in cases.values() if c[2] == 0)
    for bad in (0, 65536):
        with pytest.raises(ValueError):
            verify.frag_spans(ts, tl, trc, ql, ed, en, off, bad)
    with pytest.raises(ValueError):
        verify.frag_spans(ts, tl, trc, ql, ed, en, off[:-1], 500)           # an odd number of groups
    with pytest.raises(ValueError):
        verify.frag_histogram([501], 500)
    empty = verify.frag_spans([], [], [], [], [], [], [0], 500)
    assert len(empty) == 0 and verify.frag_histogram(empty, 500).sum() == 0


def test_frag_spans_random_pairs():
    from bucket_map_amd import verify
    rng = np.random.default_rng(20251001)
    informative = 0
    for kind in (dict(), SMALL_GROUPS):                                 # test_pair's pairs; smaller groups settle more often
        ts, tl, trc, ql, ed, en, ctg, off = random_pairs(rng, 400, **kind)
        for contig in (ctg, None):
            for cap in (1, 300, 1000, 65535):
                got = verify.frag_spans(ts, tl, trc, ql, ed, en, off, cap, contig)
                assert got.tolist() == brute_spans(ts, tl, trc, ql, ed, en, off, cap, contig), (cap, contig is None)
                informative += int((got != 0).sum())
    assert informative > 100, "the random pairs show nothing: hardly any informative pair"
    # settled is "every known alignment at one locus": where the pair is informative, select_pairs finds no second locus
    got = verify.frag_spans(ts, tl, trc, ql, ed, en, off, 1000, ctg)
    pairs = verify.select_pairs(ts, tl, trc, ql, ed, en, off, 1, 1000, ctg)
    hit = got != 0
    assert (pairs["proper"][hit] == 1).all() and (pairs["s2"][hit] == verify.PAIR_NONE).all()
    assert (pairs["pick"][0::2][hit] == pairs["winner"][0::2][hit]).all()


# ---- frag_range, hand-worked ----
def _hist(spans, cap=3000, uninformative=0):
    h = np.zeros(cap + 1, np.uint64)
    h[0] = uninformative
    for s in spans:
        h[s] += 1
    return h


def test_frag_range_hand_worked():
    from bucket_map_amd import verify
    fr = verify.frag_range
    # too few pairs: the fallback, unchanged
    r = fr(_hist([300] * 63, uninformative=1000), 64, (1, 1000))
    assert (r["min_frag"], r["max_frag"], r["learned"], r["n_informative"], r["quartiles"]) == (1, 1000, False, 63, (0, 0, 0))
    assert fr(_hist([300] * 64), 64, (1, 1000))["learned"]
    r = fr(_hist([], uninformative=5), 0, (7, 9))                           # min_pairs 0 still needs one informative pair
    assert (r["min_frag"], r["max_frag"], r["learned"], r["n_informative"]) == (7, 9, False, 0)
    # n = 1: the three quartiles are the one span; slack = ceil(301 / 4) = 76
    r = fr(_hist([301]), 1, (1, 1000))
    assert r["quartiles"] == (301, 301, 301) and (r["min_frag"], r["max_frag"]) == (225, 377) and r["learned"]
    # all spans equal: IQR 0, slack = ceil(Q2 / 4)
    r = fr(_hist([2000] * 100), 64, (1, 1000))
    assert r["quartiles"] == (2000, 2000, 2000) and (r["min_frag"], r["max_frag"]) == (1500, 2500)
    r = fr(_hist([3] * 10), 1, (1, 1000))                                   # ceil(3 / 4) = 1
    assert (r["min_frag"], r["max_frag"]) == (2, 4)
    # Q1 - slack < 1 clamps to 1: spans 10 .. 109, Q = 35, 60, 85, IQR 50, slack 150
    r = fr(_hist(range(10, 110)), 64, (1, 1000))
    assert r["quartiles"] == (35, 60, 85) and (r["min_frag"], r["max_frag"]) == (1, 235)
    # two peaks: 60 at 300, 40 at 2000 -- v[25] = 300, v[50] = 300, v[75] = 2000: IQR 1700, slack 5100
    r = fr(_hist([300] * 60 + [2000] * 40), 64, (1, 1000))
    assert r["quartiles"] == (300, 300, 2000) and (r["min_frag"], r["max_frag"]) == (1, 7100)
    # the quartile indices floor(k n / 4): n = 4 -> 1, 2, 3; n = 5 -> 1, 2, 3; n = 7 -> 1, 3, 5
    v = [100, 110, 120, 130, 140, 150, 160]
    assert fr(_hist(v[:4]), 1, (1, 1000))["quartiles"] == (110, 120, 130)
    assert fr(_hist(v[:5]), 1, (1, 1000))["quartiles"] == (110, 120, 130)
    r = fr(_hist(v), 1, (1, 1000))
    assert r["quartiles"] == (110, 130, 150)                                # IQR 40, slack max(120, 33) = 120
    assert (r["min_frag"], r["max_frag"]) == (1, 270)
    # hist[0] never counts, max_frag may exceed the cap
    r = fr(_hist([65535] * 8, cap=65535, uninformative=10 ** 6), 8, (1, 1000))
    assert r["n_informative"] == 8 and (r["min_frag"], r["max_frag"]) == (65535 - 16384, 65535 + 16384)


# ---- the tool ----
FRAG_ARGS = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "4096", "-r", "150", "-f", "1"]
DUP_AT, DUP_LEN, COPY_AT = 8000, 1200, 44_000
LEARNED = re.compile(r"^\[INFO\]\tfragment range: (\d+),(\d+) learned from (\d+) of (\d+) pairs \(quartiles (\d+) (\d+) (\d+)\)$")
KEPT = re.compile(r"^\[INFO\]\tfragment range: (\d+),(\d+) kept, (\d+) of (\d+) pairs informative$")


def _revcomp(b):
    return bytes(b).translate(COMP)[::-1]


def make_frag_fixture(d, seed=14):
    """chrA: 60 kbp of random bases in which the 1 200 bases from 8 000 stand a second time at 44 000, in another bucket.
    pairs.fastq: 40 pairs of 150-base reads in unique sequence, fragments of 1 900 .. 2 300 bases, odd pairs with the reverse
    read first; then 4 pairs whose first mate lies inside the duplicate (even ones in the first copy, odd ones in the second) and
    whose second mate lies in unique sequence a fragment further.  rescue.fastq: 40 such unique pairs again and one pair whose
    second mate lies in the duplicate and carries mismatches at every 12th base, so that no k-mer of it is found.  Returns the
    truth per pair of pairs.fastq: (1-based POS of mate 1, of mate 2)."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)
    a = bases[rng.integers(0, 4, 60_000)]
    a[COPY_AT: COPY_AT + DUP_LEN] = a[DUP_AT: DUP_AT + DUP_LEN]
    with open(d / "g.fa", "w") as f:
        f.write(f">chrA\n{bytes(a).decode()}\n")

    def unique_pair(p, name):
        m1 = int(rng.integers(11_000, 40_000))
        frag = int(rng.integers(1900, 2301))
        s1, s2 = bytes(a[m1: m1 + 150]), _revcomp(a[m1 + frag - 150: m1 + frag])
        pos = (m1 + 1, m1 + frag - 150 + 1)
        if p % 2:
            s1, s2, pos = s2, s1, pos[::-1]
        return f"@{name}{p}/1\n{s1.decode()}\n+\n{'I' * 150}\n@{name}{p}/2\n{s2.decode()}\n+\n{'I' * 150}\n", pos

    truth = []
    with open(d / "pairs.fastq", "w") as f:
        for p in range(40):
            text, pos = unique_pair(p, "u")
            f.write(text)
            truth.append(pos)
        for p in range(4):
            base = COPY_AT if p % 2 else DUP_AT
            m1 = base + DUP_LEN - 150 - int(rng.integers(0, 200))
            frag = int(rng.integers(1900, 2301))
            m2 = m1 + frag - 150
            f.write(f"@d{p}/1\n{bytes(a[m1: m1 + 150]).decode()}\n+\n{'I' * 150}\n@d{p}/2\n{_revcomp(a[m2: m2 + 150]).decode()}\n+\n{'I' * 150}\n")
            truth.append((m1 + 1, m2 + 1))
    with open(d / "rescue.fastq", "w") as f:
        for p in range(40):
            f.write(unique_pair(p, "v")[0])
        m1 = 5000
        m2 = m1 + 2100 - 150
        far = a[m2: m2 + 150].copy()
        far[5::12] = bases[(np.searchsorted(bases, far[5::12]) + 1) % 4]
        f.write(f"@r0/1\n{bytes(a[m1: m1 + 150]).decode()}\n+\n{'I' * 150}\n@r0/2\n{_revcomp(far).decode()}\n+\n{'I' * 150}\n")
    return truth


@pytest.fixture(scope="module")
def frag_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("frag")
    return d, make_frag_fixture(d)


def run_frag_tool(exe, d, fastq, out, *extra, ok=True, block="4096", env=None):
    env = dict(os.environ, BM_VERIFY_BLOCK_READS=block, **(env or {}))
    r = subprocess.run([exe, *FRAG_ARGS, "-q", fastq, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def parse_range_lines(stderr):
    """The tool's fragment-range lines, one dict per verifier block."""
    out = []
    for line in stderr.split("\n"):
        if "fragment range" not in line:
            continue
        m, k = LEARNED.match(line), KEPT.match(line)
        assert m or k, f"not in the documented form: {line!r}"
        g = [int(x) for x in (m or k).groups()]
        out.append({"min": g[0], "max": g[1], "learned": bool(m), "informative": g[2], "pairs": g[3], "quartiles": tuple(g[4:])})
    return out


def sam_records(path):
    return [l.split("\t") for l in open(path).read().split("\n") if l and not l.startswith("@")]


def test_tool_learns_the_range_of_a_long_fragment_library(frag_files):
    d, truth = frag_files
    r = run_frag_tool(TOOL, d, "pairs.fastq", "paired.sam", "--paired")
    assert "fragment range" not in r.stderr
    paired = sam_records(d / "paired.sam")
    assert [x[0] for x in paired] == [f"{'u' if p < 40 else 'd'}{p if p < 40 else p - 40}" for p in range(44) for _ in (1, 2)]
    assert all(int(x[1]) & 0x2 == 0 for x in paired), "2 kbp fragments are not proper under the default range 1,1000"
    for p in range(40, 44):
        assert paired[2 * p][4] == "0", "the mate in the duplicate is a tie --paired cannot break under the default range"
    r = run_frag_tool(TOOL, d, "pairs.fastq", "auto.sam", "--frag-auto", "--frag-min-pairs", "20")
    lines = parse_range_lines(r.stderr)
    assert len(lines) == 1 and lines[0]["learned"] and lines[0]["pairs"] == 44
    assert lines[0]["informative"] == 40, "the fixture must give 40 informative pairs: every unique pair and no duplicate one"
    lo, hi = lines[0]["min"], lines[0]["max"]
    assert lo <= 1900 and hi >= 2300 and all(1900 <= q <= 2300 for q in lines[0]["quartiles"])
    auto = sam_records(d / "auto.sam")
    assert len(auto) == 88
    for p, (pos1, pos2) in enumerate(truth):
        m1, m2 = auto[2 * p], auto[2 * p + 1]
        assert int(m1[1]) & 0x3 == 0x3 and int(m2[1]) & 0x3 == 0x3, (p, m1[:4], m2[:4])
        assert int(m1[3]) == pos1 and int(m2[3]) == pos2 and m1[4] == m2[4] == "60", (p, m1[:5], m2[:5])
        assert 1900 <= abs(int(m1[8])) <= 2300
    # bm::frag_range (host/frag_range.h) held to the contract: the printed range and quartiles are verify.frag_range's over the
    # 40 informative spans, which are the unique pairs' TLENs (exact reads: R(r) - L(f) is the fragment)
    from bucket_map_amd import verify
    spans = [abs(int(auto[2 * p][8])) for p in range(40)]
    want = verify.frag_range(verify.frag_histogram(spans + [0] * 4, 10_000), 20, (1, 1000))
    assert want["learned"] and want["n_informative"] == 40
    assert (lo, hi, lines[0]["quartiles"]) == (want["min_frag"], want["max_frag"], want["quartiles"])
    ordered = sorted(spans)
    assert want["quartiles"] == (ordered[10], ordered[20], ordered[30])
    # the same bytes as --paired under the printed range
    run_frag_tool(TOOL, d, "pairs.fastq", "typed.sam", "--paired", "--frag-range", f"{lo},{hi}")
    assert (d / "auto.sam").read_bytes() == (d / "typed.sam").read_bytes()
    # too few informative pairs: the range is kept and nothing changes
    r = run_frag_tool(TOOL, d, "pairs.fastq", "kept.sam", "--frag-auto", "--frag-min-pairs", "1000")
    lines = parse_range_lines(r.stderr)
    assert lines == [{"min": 1, "max": 1000, "learned": False, "informative": 40, "pairs": 44, "quartiles": ()}]
    assert (d / "kept.sam").read_bytes() == (d / "paired.sam").read_bytes()
    # --frag-range is the fallback; --frag-cap bounds what counts: under cap 2000 the longer fragments are uninformative
    r = run_frag_tool(TOOL, d, "pairs.fastq", "kept2.sam", "--frag-auto", "--frag-min-pairs", "1000", "--frag-range", "5,3000")
    assert parse_range_lines(r.stderr)[0]["min"] == 5 and parse_range_lines(r.stderr)[0]["max"] == 3000
    r = run_frag_tool(TOOL, d, "pairs.fastq", "cap.sam", "--frag-cap", "2000", "--frag-min-pairs=5")
    short = sum(1 for p in range(40) if abs(int(auto[2 * p][8])) <= 2000)
    assert parse_range_lines(r.stderr)[0]["informative"] == short and 5 <= short < 40
    # a block learns from its own pairs only: blocks of 8 reads have 4 pairs each
    r = run_frag_tool(TOOL, d, "pairs.fastq", "blocks.sam", "--frag-auto", "--frag-min-pairs", "4", block="8")
    lines = parse_range_lines(r.stderr)
    assert len(lines) == 11 and all(x["pairs"] == 4 for x in lines) and [x["learned"] for x in lines] == [True] * 10 + [False]
    for b, line in enumerate(lines[:10]):                                   # n = 4: the quartiles are v[1], v[2], v[3]
        want = verify.frag_range(verify.frag_histogram(spans[4 * b: 4 * b + 4], 10_000), 4, (1, 1000))
        assert (line["min"], line["max"], line["quartiles"]) == (want["min_frag"], want["max_frag"], want["quartiles"]), b


def test_tool_refusals(frag_files):
    d, _ = frag_files
    for bad in (["--frag-cap", "0"], ["--frag-cap", "70000"], ["--frag-cap", "x"], ["--frag-min-pairs", "-1x"]):
        r = run_frag_tool(TOOL, d, "pairs.fastq", "never.sam", *bad, ok=False)
        assert f"Value parse failed for {bad[0]}" in r.stderr and not os.path.exists(d / "never.sam")
    for flag in (["--frag-auto"], ["--frag-cap", "10000"], ["--frag-min-pairs", "64"]):
        r = run_frag_tool(PLAIN_TOOL, d, "pairs.fastq", "never2.sam", *flag, ok=False)
        assert r.returncode == 255 and "belongs to bucketmap_align" in r.stderr and not os.path.exists(d / "never2.sam")
    r = run_frag_tool(TOOL, d, "pairs.fastq", "never3.sam", "--split", "--frag-auto", ok=False)
    assert "--split cannot be combined with --frag-auto" in r.stderr and not os.path.exists(d / "never3.sam")
