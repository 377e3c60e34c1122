"""Split alignments without a GPU: the plain-Python restatements of bmv_split's contract (include/bmv.h) that
tests/test_split_gpu.py compares the device against -- verify.clip_range held against test_clip's brute force over all (l, r),
verify.select_segments against a brute force that sorts once and walks once --, hand-worked cases, split_mapq, the SA:Z
formatter, host/split_pick.h under sanitizers, the ABI surface and the tools' --split options."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_annotate import D, I, M, pack
from test_clip import CASES, range_brute, restate_clip

from bucket_map_amd import verify

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = {
    "bucketmap": os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle"),
    "bucketmap_align": os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle"),
}
NAMES = ("bmv_split", "bmv_split_pick", "bmv_segments", "bmv_last_split_stats")
NONE, BEYOND = verify.SPLIT_NONE, verify.BEYOND
RANGE_KEYS = ("score", "clip_left", "clip_right", "pos", "ref_len")


# ------------------------------------------------------------------------------------------------ the ABI surface

def test_header_and_binding_agree_on_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "bmv.h")).read()
    assert re.search(r"#define\s+BMV_SPLIT_MAX_SEGMENTS\s+16u", text) and re.search(r"#define\s+BMV_SPLIT_NONE\s+INT64_MIN", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = verify.lib()
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
        n_args = len(re.search(rf"\b{name}\s*\((.*?)\)", text, flags=re.S).group(1).split(","))
        assert n_args == len(verify.SYMBOLS[name][1]), name
    assert all(callable(getattr(verify.Verifier, f)) for f in ("split", "split_pick", "split_stats"))
    assert verify.SPLIT_MAX_SEGMENTS == 16 and verify.SPLIT_NONE == -(2 ** 63)


def test_entry_points_fail_cleanly_without_a_context():
    L = verify.lib()
    assert L.bmv_split(None, None, 0, None, None, None, None, None, None, None, None, None, 0, None, 0, 1, 2, 40, 500, 8) == 1
    assert b"bmv_split" in L.bmv_last_error() and b"bmv_split_pick" not in L.bmv_last_error()
    assert L.bmv_split_pick(None, None, None, None, None, None, None, None, 0, None, 0, 40, 500, 8) == 1
    assert b"bmv_split_pick" in L.bmv_last_error()
    assert L.bmv_segments(None, None, None, None, None, None, None, None, None) == 1
    assert b"bmv_segments" in L.bmv_last_error()
    assert L.bmv_last_split_stats(None, None, None, None, None) == 1
    assert b"bmv_last_split_stats" in L.bmv_last_error()


# ------------------------------------------------------------------------------------------------ clip_range

def random_alignment(rng, letters=b"AC", max_entries=6, max_m=9):
    """A small random M/I/D path with its window and query over few letters, so that equal scores are common."""
    cigar, last = [], None
    for _ in range(int(rng.integers(1, max_entries))):
        op = int(rng.choice([o for o in (M, I, D) if o != last]))
        cigar.append((op, int(rng.integers(1, max_m if op == M else 4))))
        last = op
    rc, begin = int(rng.integers(0, 2)), int(rng.integers(0, 3))
    window = bytes(rng.choice(list(letters), begin + sum(n for op, n in cigar if op != I) + int(rng.integers(0, 3))).astype(np.uint8))
    query = bytes(rng.choice(list(letters), sum(n for op, n in cigar if op != D)).astype(np.uint8))
    return window, rc, query, begin, cigar


def test_clip_range_against_brute_force():
    """2 000 random column strings over two letters: verify.clip_range's one pass finds what the O(C^2) search over all
    (l, r) finds -- the same score, clips, pos and ref_len, ties included -- and bmv_clip's identities hold."""
    rng = np.random.default_rng(1401)
    cut = 0
    for t in range(2000):
        window, rc, query, begin, cigar = random_alignment(rng)
        match, penalty = ((1, 2), (1, 1), (3, 2), (1024, 1), (1, 1024))[t % 5]
        want = restate_clip(window, rc, query, begin, cigar, match, penalty, range_brute)
        got = verify.clip_range(window, query, rc, begin, pack(cigar), match, penalty)
        assert {k: got[k] for k in RANGE_KEYS} == {k: want[k] for k in RANGE_KEYS}, (window, rc, query, begin, cigar, match, penalty)
        m = len(query)
        kept = m - got["clip_left"] - got["clip_right"]
        assert kept >= 0 and got["pos"] + got["ref_len"] <= len(window)
        assert (got["q_lo"], got["q_hi"]) == ((got["clip_right"], m - got["clip_left"]) if rc else (got["clip_left"], m - got["clip_right"]))
        assert got["q_hi"] - got["q_lo"] == kept and (got["g_off_lo"], got["g_off_hi"]) == (got["pos"], got["pos"] + got["ref_len"])
        cut += got["score"] > 0 and kept < m
    assert cut > 400, "hardly any alignment was cut: the comparison shows little"


def test_clip_range_ties_follow_the_rules():
    """Equal-score ranges: the smallest r, then the largest l -- on columns written out by hand, on both strands."""
    # = = X X = =: [0, 2) and [4, 6) both score 2 -> the first; = = X = = =: P[6] - P[0] = P[6] - P[3] -> l = 3
    for window, rc, query, want in ((b"ACGTAC", 0, b"ACTGAC", (2, 0, 2)), (b"ACGTAC", 0, b"ACTTAC", (3, 3, 6)),
                                    (b"ACGTAC", 1, b"GTCAGT", (2, 0, 2)), (b"ACGTAC", 1, b"GTAAGT", (3, 3, 6))):
        got = verify.clip_range(window, query, rc, 0, pack([(M, 6)]))
        assert (got["score"], got["l"], got["r"]) == want


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_clip_range_on_the_hand_worked_cases_of_clip(case):
    """test_clip's hand-worked answers on both strands -- a range cut inside an M entry, I and D at the border, no = column,
    an empty CIGAR -- and the read-orientation interval derived from them."""
    _, window, rc, query, begin, cigar, (match, penalty), score, cl, cr, pos, ref_len = case[:12]
    got = verify.clip_range(window, query, rc, begin, pack(cigar), match, penalty)
    assert tuple(got[k] for k in RANGE_KEYS) == (score, cl, cr, pos, ref_len)
    m = len(query)
    assert (got["q_lo"], got["q_hi"]) == ((cr, m - cl) if rc else (cl, m - cr))


def test_read_orientation_of_the_kept_interval():
    """Worked by hand: the read GTACGTAAA aligned to the reverse strand keeps its FIRST six bases (forward: 3S6=)."""
    got = verify.clip_range(b"ACGTAC", b"GTACGTAAA", 1, 0, pack([(M, 6), (I, 3)]))
    assert (got["clip_left"], got["clip_right"], got["q_lo"], got["q_hi"], got["g_off_lo"], got["g_off_hi"]) == (3, 0, 0, 6, 0, 6)
    got = verify.clip_range(b"ACGTAC", b"ACGTACTTT", 0, 0, pack([(M, 6), (I, 3)]))
    assert (got["clip_left"], got["clip_right"], got["q_lo"], got["q_hi"]) == (0, 3, 0, 6)
    got = verify.clip_range(b"AAAA", b"CCCC", 1, 0, pack([(M, 4)]))          # no = column: cr = m, an empty interval
    assert (got["score"], got["q_lo"], got["q_hi"], got["g_off_lo"], got["g_off_hi"]) == (0, 4, 4, 0, 0)
    got = verify.clip_range(b"ACGT", b"AC", 0, 0, [])                        # an empty CIGAR: zeros
    assert (got["score"], got["clip_left"], got["clip_right"], got["pos"], got["ref_len"]) == (0, 0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ select_segments

def pick_brute(score, q_lo, q_hi, g_lo, g_hi, rc, off, min_score, permille, max_segments, contig=None):
    """The contract of include/bmv.h the other way round: the group's eligible alignments sorted once by (-S, index) and
    walked once -- one that conflicts with nothing taken so far is taken --, then s2 by its definition."""
    def ovl(lo, hi, a, b):
        return max(0, min(hi[a], hi[b]) - max(lo[a], lo[b]))

    def dup(a, b):
        return ((contig is None or contig[a] == contig[b]) and bool(rc[a]) == bool(rc[b]) and ovl(g_lo, g_hi, a, b) > 0
                and ovl(q_lo, q_hi, a, b) > 0)

    def conflict(a, b):
        return dup(a, b) or ovl(q_lo, q_hi, a, b) * 1000 > permille * min(q_hi[a] - q_lo[a], q_hi[b] - q_lo[b])

    n_groups = len(off) - 1
    n_seg, seg, s2 = [0] * n_groups, [[BEYOND] * max_segments for _ in range(n_groups)], [[NONE] * max_segments for _ in range(n_groups)]
    for g in range(n_groups):
        members = list(range(off[g], off[g + 1]))
        taken = []
        for a in sorted((a for a in members if score[a] >= min_score), key=lambda a: (-score[a], a)):
            if len(taken) < max_segments and not any(conflict(a, c) for c in taken):
                taken.append(a)
        n_seg[g] = len(taken)
        for k, c in enumerate(taken):
            seg[g][k] = c
            rivals = [score[a] for a in members if a not in taken and score[a] > 0 and not dup(a, c)
                      and 2 * ovl(q_lo, q_hi, a, c) >= q_hi[c] - q_lo[c]]
            s2[g][k] = max(rivals, default=NONE)
    return n_seg, seg, s2


def check_pick(score, q_lo, q_hi, g_lo, g_hi, rc, off, min_score, permille, max_segments, contig=None):
    got = verify.select_segments(score, q_lo, q_hi, g_lo, g_hi, rc, off, min_score, permille, max_segments, contig)
    n_seg, seg, s2 = pick_brute(score, q_lo, q_hi, g_lo, g_hi, rc, off, min_score, permille, max_segments, contig)
    assert got["n_seg"].tolist() == n_seg and got["seg"].tolist() == seg and got["s2"].tolist() == s2
    return got


def one(cands, min_score=40, permille=500, max_segments=8, contig=False):
    """One group of (score, q_lo, q_hi, g_lo, g_hi, rc[, contig]) tuples: the chosen list and s2 of the chosen."""
    cols = list(zip(*cands)) if cands else [[]] * 7
    got = check_pick(*[list(c) for c in cols[:6]], [0, len(cands)], min_score, permille, max_segments,
                     list(cols[6]) if contig else None)
    k = int(got["n_seg"][0])
    assert all(x == BEYOND for x in got["seg"][0, k:]) and all(x == NONE for x in got["s2"][0, k:])
    return got["seg"][0, :k].tolist(), got["s2"][0, :k].tolist()


def test_pick_empty_groups_and_nothing_eligible():
    got = check_pick([50], [0], [10], [0], [10], [0], [0, 0, 1, 1], 40, 500, 4)
    assert got["n_seg"].tolist() == [0, 1, 0]
    assert one([]) == ([], [])
    assert one([(39, 0, 10, 0, 10, 0), (0, 20, 30, 50, 60, 0), (-3, 40, 50, 90, 100, 1)]) == ([], [])
    got = check_pick([], [], [], [], [], [], [0], 40, 500, 4)
    assert got["seg"].shape == (0, 4)


def test_pick_min_score_border():
    assert one([(40, 0, 10, 0, 10, 0), (39, 20, 30, 50, 60, 0)]) == ([0], [NONE])
    assert one([(40, 0, 10, 0, 10, 0), (39, 20, 30, 50, 60, 0)], min_score=39) == ([0, 1], [NONE, NONE])
    assert one([(1, 0, 10, 0, 10, 0)], min_score=1) == ([0], [NONE])


def test_pick_score_ties_go_to_the_lowest_index():
    # three candidates for the same part of the read, two of them equal: the first of the equals wins, the others compete
    assert one([(50, 0, 100, 0, 100, 0), (60, 0, 100, 500, 600, 0), (60, 0, 100, 900, 1000, 0)]) == ([1], [60])
    # disjoint parts with equal scores come in index order
    assert one([(60, 200, 300, 0, 100, 0), (60, 0, 100, 500, 600, 1), (60, 100, 200, 900, 1000, 0)]) == ([0, 1, 2], [NONE] * 3)


def test_pick_overlap_at_the_threshold_and_one_base_over():
    # the shorter interval has 100 bases; 500 permille admits 50 shared bases and refuses 51
    at = [(90, 0, 200, 0, 200, 0), (80, 150, 250, 5000, 5100, 0)]
    over = [(90, 0, 200, 0, 200, 0), (80, 149, 249, 5000, 5100, 0)]
    assert one(at)[0] == [0, 1] and one(over)[0] == [0]
    assert one(over, permille=510)[0] == [0, 1] and one(at, permille=499)[0] == [0]
    # 0 permille: any shared base conflicts, touching intervals do not; 1000: only dups conflict
    assert one([(90, 0, 100, 0, 100, 0), (80, 100, 200, 5000, 5100, 0)], permille=0)[0] == [0, 1]
    assert one([(90, 0, 100, 0, 100, 0), (80, 99, 200, 5000, 5100, 0)], permille=0)[0] == [0]
    assert one([(90, 0, 100, 0, 100, 0), (80, 0, 100, 5000, 5100, 0)], permille=1000)[0] == [0, 1]


def test_pick_dup_needs_strand_contig_and_both_overlaps():
    a = (90, 0, 100, 1000, 1100, 0, 0)
    # the same alignment through a second window: a slightly different range at the same place -- never a second segment, and
    # no competitor either
    assert one([a, (85, 90, 190, 1090, 1190, 0, 0)], permille=1000, contig=True) == ([0], [NONE])
    # the other strand, or another contig: no dup; under 1000 permille nothing else conflicts
    assert one([a, (85, 90, 190, 1090, 1190, 1, 0)], permille=1000, contig=True)[0] == [0, 1]
    assert one([a, (85, 90, 190, 1090, 1190, 0, 1)], permille=1000, contig=True)[0] == [0, 1]
    assert one([a[:6], (85, 90, 190, 1090, 1190, 0)], permille=1000)[0] == [0]                 # contig None: one contig
    # a tandem copy: the reference intervals overlap, the query intervals do not -- two segments
    assert one([a, (85, 100, 200, 1050, 1150, 0, 0)], permille=0, contig=True)[0] == [0, 1]
    # the reference intervals touch but share no base: no dup
    assert one([a, (85, 90, 190, 1100, 1200, 0, 0)], permille=1000, contig=True)[0] == [0, 1]


def test_pick_max_segments_one_and_sixteen():
    parts = [(100 - k, 10 * k, 10 * k + 10, 1000 * k, 1000 * k + 10, k % 2) for k in range(20)]
    assert one(parts, max_segments=1) == ([0], [NONE])
    assert one(parts, max_segments=16) == (list(range(16)), [NONE] * 16)
    # what did not fit is no competitor of a segment it does not overlap, and one of a segment it covers
    parts.append((70, 0, 10, 77000, 77010, 0))
    assert one(parts, max_segments=16)[1] == [70] + [NONE] * 15


def test_competitors_cover_half_of_the_segment():
    seg = (90, 0, 100, 0, 100, 0)
    # a candidate below min_score is never chosen; it competes when it covers exactly half of the segment ...
    assert one([seg, (39, 50, 300, 5000, 5250, 0)]) == ([0], [39])
    # ... and not with one base less
    assert one([seg, (39, 51, 300, 5000, 5249, 0)]) == ([0], [NONE])
    # an eligible one that shares 50 of the segment's 100 bases is a second segment under 500 permille, and a chosen
    # alignment is nobody's competitor
    assert one([seg, (50, 50, 300, 5000, 5250, 0)]) == ([0, 1], [NONE, NONE])
    # under 0 permille it conflicts, stays out and competes -- again only from half of the segment on
    assert one([seg, (50, 50, 300, 5000, 5250, 0)], permille=0) == ([0], [50])
    assert one([seg, (50, 51, 300, 5000, 5249, 0)], permille=0) == ([0], [NONE])
    # an ineligible candidate competes as long as its score is positive; the greatest one counts
    assert one([seg, (39, 0, 100, 5000, 5100, 0), (12, 0, 100, 7000, 7100, 1), (0, 0, 100, 9000, 9100, 0)]) == ([0], [39])
    # a dup never competes
    assert one([seg, (80, 10, 100, 10, 100, 0)]) == ([0], [NONE])


def test_pick_random_groups_against_the_brute_force():
    rng = np.random.default_rng(1402)
    chosen = 0
    for t in range(600):
        sizes = rng.integers(0, 12, int(rng.integers(1, 5)))
        off = [0] + np.cumsum(sizes).tolist()
        n, m = off[-1], int(rng.integers(20, 60))
        score = (rng.integers(0, 8, n) * 5 - 5).tolist()
        q_lo = rng.integers(0, m, n)
        q_hi = (q_lo + rng.integers(0, m - q_lo + 1)).tolist()
        g_lo = rng.integers(0, 120, n)
        g_hi = (g_lo + rng.integers(0, 40, n)).tolist()
        got = check_pick(score, q_lo.tolist(), q_hi, g_lo.tolist(), g_hi, rng.integers(0, 2, n).tolist(), off, int(rng.choice([1, 10, 20])),
                         int(rng.choice([0, 250, 500, 1000])), int(rng.choice([1, 2, 3, 16])),
                         rng.integers(0, 2, n).tolist() if t % 3 else None)
        chosen += int(got["n_seg"].sum())
    assert chosen > 1000


# ------------------------------------------------------------------------------------------------ split_mapq, SA:Z

def test_split_mapq_cases():
    assert verify.split_mapq(100, NONE) == 60 and verify.split_mapq(1, NONE) == 60
    assert verify.split_mapq(100, 100) == 0 and verify.split_mapq(100, 101) == 0 and verify.split_mapq(40, 2 ** 40) == 0
    assert verify.split_mapq(100, 50) == 30 and verify.split_mapq(100, 1) == 59 and verify.split_mapq(100, 99) == 0
    assert verify.split_mapq(7, 3) == 34                                     # 4 * 60 / 7, integer division
    assert verify.split_mapq(2 ** 43, 2 ** 42) == 30 and verify.split_mapq(2 ** 43 + 7, 1) == 59      # 64-bit products


def test_sa_entry_merges_equal_and_unequal_runs():
    S, EQ, X = 4, 7, 8
    xc = pack([(S, 3), (EQ, 5), (X, 1), (EQ, 2), (I, 2), (X, 1), (D, 1), (EQ, 4), (S, 7)])
    assert verify.sa_entry("chr2", 99, False, xc, 37, 5) == "chr2,100,+,3S8M2I1M1D4M7S,37,5;"
    assert verify.sa_entry("chr2", 0, True, pack([(EQ, 10)]), 60, 0) == "chr2,1,-,10M,60,0;"
    assert verify.sa_entry("c", 2 ** 33, True, pack([(S, 1), (EQ, 1)]), 0, 0) == f"c,{2 ** 33 + 1},-,1S1M,0,0;"


# ------------------------------------------------------------------------------------------------ the sanitized host header

def test_the_host_header_under_sanitizers(tmp_path):
    """tests/cpp/split_pick_check.cpp, a program of its own around host/split_pick.h, built with -fsanitize=address,undefined
    and run: clean, and every line it prints -- 602 picks, the MAPQ table, 60 SA entries -- is what the restatements here give."""
    exe = str(tmp_path / "split_pick_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "split_pick_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split("\n")[:-1]
    kinds = [line[0] for line in lines]
    assert (kinds.count("P"), kinds.count("Q"), kinds.count("A")) == (602, 90, 60)
    chosen = rivals = 0
    for line in lines:
        if line[0] == "P":
            given, result = (part.split() for part in line[2:].split("|"))
            min_score, permille, ms, use_contig, n = (int(x) for x in given[:5])
            f = [[int(given[5 + 7 * a + k]) for a in range(n)] for k in range(7)]
            want = verify.select_segments(f[0], f[1], f[2], f[3], f[4], f[5], [0, n], min_score, permille, ms, f[6] if use_contig else None)
            assert int(result[0]) == int(want["n_seg"][0]), line
            assert [int(x) for x in result[1::2]] == want["seg"][0].tolist() and [int(x) for x in result[2::2]] == want["s2"][0].tolist(), line
            chosen += int(result[0])
            rivals += sum(int(x) != NONE for x in result[2::2])
        elif line[0] == "Q":
            s1, s2, mapq = (int(x) for x in line.split()[1:])
            assert verify.split_mapq(s1, s2) == mapq, line
        else:
            given, text = line[2:].split(" | ")
            g = given.split()
            assert verify.sa_entry(g[0], int(g[1]), g[2] == "1", [int(x) for x in g[6:6 + int(g[5])]], int(g[3]), int(g[4])) == text, line
    assert chosen > 600 and rivals > 100, "the random groups exercise little"


# ------------------------------------------------------------------------------------------------ the options

def test_the_options_of_bucketmap_align(tmp_path):
    def run(*extra):
        return subprocess.run([TOOLS["bucketmap_align"], "-i", "idx", *extra], cwd=str(tmp_path), capture_output=True, text=True)
    for ok in (["--split"], ["--split-min-score", "1"], ["--split-min-score=2147483648"], ["--split-overlap", "0"], ["--split-overlap", "1"],
               ["--split-overlap=0.25"], ["--split-max", "1"], ["--split-max", "16"], ["--split", "--clip-scores", "1,3", "--affine", "--left-align"],
               ["--split", "--clip", "--annotate"]):
        r = run(*ok)                                             # parsed; what fails next is the missing genome
        assert r.returncode != 0 and "Unknown option" not in r.stderr and "BM_GENOME_FILE is not found" in r.stderr, (ok, r.stderr)
    for opt, bad in (("--split-min-score", "0"), ("--split-min-score", "2147483649"), ("--split-min-score", "x"), ("--split-overlap", "-0.1"),
                     ("--split-overlap", "1.5"), ("--split-overlap", "half"), ("--split-max", "0"), ("--split-max", "17"), ("--split-max", "")):
        r = run(opt, bad)
        assert r.returncode != 0 and opt in r.stderr and "BM_GENOME_FILE" not in r.stderr, (opt, bad, r.stderr)
    # what --split refuses, however it was switched on, with the reason
    for first in (["--split"], ["--split-max", "4"], ["--split-overlap", "0.3"], ["--split-min-score", "50"]):
        for other, name in ((["--best"], "--best"), (["--best-margin", "0.1"], "--best"), (["--paired"], "--paired"),
                            (["--frag-range", "1,500"], "--paired"), (["--rescue"], "--rescue"), (["--max-edit-rate", "0.1"], "--max-edit-rate")):
            for args in (first + other, other + first):
                r = run(*args)
                assert r.returncode != 0 and "--split cannot be combined with " + name in r.stderr and "breakpoint" in r.stderr, (args, r.stderr)
                assert "BM_GENOME_FILE" not in r.stderr


def test_the_options_imply_clip_and_annotate():
    """cli.h compiled with and without BM_ALIGN into a program that prints what the parser set."""
    src = r'''
#include "cli.h"
#include <cstdio>
int main(int argc, char **argv) {
    try {
        const bm::cmd_arguments a = bm::parse_arguments(argc, argv);
        std::printf("%d %d %d %lu %u %u %u %u\n", a.split, a.clip, a.annotate, a.split_min_score, (unsigned)(a.split_overlap * 1000), a.split_max,
                    a.clip_match, a.clip_penalty);
    } catch (const bm::parser_error &e) {
        std::printf("error %s\n", e.what());
    }
}
'''
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.cpp"), "w").write(src)
        inc = os.path.join(ROOT, "bucket-map_amd", "host")
        for flag in ("-DBM_ALIGN", "-DBM_PLAIN"):
            r = subprocess.run(["g++", "-std=c++17", flag, "-I", inc, "-o", os.path.join(d, "p" + flag), os.path.join(d, "p.cpp")],
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]

        def out(flag, *args):
            return subprocess.run([os.path.join(d, "p" + flag), "-i", "idx", *args], capture_output=True, text=True).stdout.strip()
        assert out("-DBM_ALIGN") == "0 0 0 40 500 8 1 2"
        assert out("-DBM_ALIGN", "--split") == "1 1 1 40 500 8 1 2"
        assert out("-DBM_ALIGN", "--split-min-score", "55") == "1 1 1 55 500 8 1 2"
        assert out("-DBM_ALIGN", "--split-overlap", "0.25") == "1 1 1 40 250 8 1 2"
        assert out("-DBM_ALIGN", "--split-max=3", "--clip-scores", "2,5") == "1 1 1 40 500 3 2 5"
        for opt in (["--split"], ["--split-min-score", "50"], ["--split-overlap", "0.5"], ["--split-max", "2"]):
            text = out("-DBM_PLAIN", *opt)
            assert text.startswith("error") and opt[0] in text and "belongs to bucketmap_align" in text, text


@pytest.mark.parametrize("opt", [["--split"], ["--split-min-score", "50"], ["--split-overlap", "0.5"], ["--split-max", "2"]])
def test_bucketmap_refuses_the_options(opt, tmp_path):
    r = subprocess.run([TOOLS["bucketmap"], "-i", "idx", *opt], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode != 0 and opt[0] in r.stderr and "belongs to bucketmap_align" in r.stderr and "BM_GENOME_FILE" not in r.stderr, r.stderr
