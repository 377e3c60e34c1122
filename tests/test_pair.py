"""Paired-end reads without a GPU: the surface of bmv_pair / bmv_align_paired, the contract of the pair-aware pick restated in
numpy (verify.select_pairs) against an independent brute force, the MAPQ helper (verify.pair_mapq, host/pair_mapq.h), and the
tools' --paired through the oracle-backed tool, whose verifier takes alignment_verifier::paired's default (align everything,
pick on the host)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")
PLAIN_TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle")
BASES = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def test_header_binding_and_python_surface():
    from bucket_map_amd import verify
    text = open(os.path.join(ROOT, "include", "bmv.h")).read()
    assert re.search(r"#define\s+BMV_PAIR_NONE\s+UINT64_MAX", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = verify.lib()
    for name in ("bmv_pair", "bmv_pairs", "bmv_last_pair_stats", "bmv_align_paired"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
    decl = re.search(r"bmv_align_paired\s*\((.*?)\)", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")][-9:] == ["n", "group_offset", "n_groups", "margin", "hint", "contig",
                                                                       "min_frag", "max_frag", "total_cigar"]
    decl = re.search(r"bmv_pair\s*\((.*?)\)", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "text_start", "text_len", "text_rc", "query_len", "edits", "end",
                                                                   "contig", "n", "group_offset", "n_groups", "min_frag", "max_frag"]
    assert verify.PAIR_NONE == 2 ** 64 - 1
    for fn in ("pair", "align_paired", "pair_stats"):
        assert callable(getattr(verify.Verifier, fn))
    assert callable(verify.select_pairs) and callable(verify.pair_mapq)
    total = C.c_uint64()
    assert L.bmv_pair(None, None, None, None, None, None, None, None, 0, None, 0, 1, 1000) == 1
    assert b"bmv_pair" in L.bmv_last_error()
    assert L.bmv_align_paired(None, None, 0, None, None, None, None, None, 0, None, 0, None, None, None, 1, 1000, C.byref(total)) == 1
    assert b"bmv_align_paired" in L.bmv_last_error()
    assert L.bmv_pairs(None, None, None, None, None, None) == 1 and L.bmv_last_pair_stats(None, None, None) == 1


# ---- select_pairs against a brute force ----
def brute_pairs(ts, tl, trc, ql, edits, end, off, min_frag, max_frag, contig=None):
    """bmv_pair's definitions by the book: plain Python integers, every combination listed, one sort."""
    B, NONE = 2 ** 32 - 1, 2 ** 64 - 1
    n_groups = len(off) - 1

    def left(a):
        return int(ts[a]) + int(tl[a]) - int(end[a]) if trc[a] else int(ts[a]) + int(end[a]) - int(ql[a])

    def right(a):
        return left(a) + int(ql[a])

    def locus(a):
        return (bool(trc[a]), left(a) if trc[a] else right(a))

    def proper(i, j):
        if edits[i] == B or edits[j] == B or bool(trc[i]) == bool(trc[j]):
            return False
        if contig is not None and contig[i] != contig[j]:
            return False
        f, r = (j, i) if trc[i] else (i, j)
        return left(f) <= left(r) and right(f) <= right(r) and min_frag <= right(r) - left(f) <= max_frag

    winner = []
    for g in range(n_groups):
        known = sorted((int(edits[a]), a) for a in range(int(off[g]), int(off[g + 1])) if edits[a] != B)
        winner.append(known[0][1] if known else B)
    pick, prop, s1, s2 = list(winner), [], [], []
    for p in range(n_groups // 2):
        combos = sorted((int(edits[i]) + int(edits[j]), i, j) for i in range(int(off[2 * p]), int(off[2 * p + 1]))
                        for j in range(int(off[2 * p + 1]), int(off[2 * p + 2])) if proper(i, j))
        prop.append(1 if combos else 0)
        s1.append(combos[0][0] if combos else NONE)
        rest = []
        if combos:
            _, bi, bj = combos[0]
            pick[2 * p], pick[2 * p + 1] = bi, bj
            rest = [s for s, i, j in combos if locus(i) != locus(bi) or locus(j) != locus(bj)]
        s2.append(min(rest) if rest else NONE)
    return {"pick": pick, "proper": prop, "s1": s1, "s2": s2, "winner": winner}


def assert_pairs_equal(got, want, what=""):
    for key in ("pick", "proper", "s1", "s2", "winner"):
        g, w = np.asarray(got[key]).astype(np.uint64), np.asarray(want[key], np.uint64)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {key} differs at {bad[:8]}: got {g[bad[:8]]}, want {w[bad[:8]]}"


def random_pairs(rng, n_pairs, sizes=(0, 1, 2, 3, 5, 9), p_unknown=0.2, span=3000, mixed_contigs=True):
    """Groups of candidates around a few shared anchors: many combinations are proper, sums tie (edits 0 .. 3), loci repeat
    (the same alignment through two windows), strands and contigs mix."""
    ts, tl, trc, ql, ed, en, ctg, off = [], [], [], [], [], [], [], [0]
    for _ in range(n_pairs):
        anchor = int(rng.integers(2000, 100_000))
        for mate in range(2):
            m = int(rng.integers(30, 160))
            for _ in range(int(rng.choice(sizes))):
                rc = int(rng.integers(0, 2)) if rng.random() < 0.3 else mate
                width = m + int(rng.integers(1, 12))
                start = anchor + int(rng.integers(-span, span)) if rng.random() < 0.8 else anchor + 300 * mate
                e = int(rng.integers(max(m - 6, 0), width + 1))
                if ts and rng.random() < 0.25 and len(ts) > off[-1]:        # the alignment before through a shifted window
                    shift = int(rng.integers(1, 5))
                    start, width, rc, e = ts[-1] - shift, tl[-1] + shift, trc[-1], (en[-1] if trc[-1] else en[-1] + shift)
                    m = ql[-1]
                ts.append(max(start, 0)); tl.append(width); trc.append(rc); ql.append(m)
                ed.append(2 ** 32 - 1 if rng.random() < p_unknown else int(rng.integers(0, 4)))
                en.append(min(e, width))
                ctg.append(int(rng.integers(0, 2)) if mixed_contigs and rng.random() < 0.2 else 0)
            off.append(len(ts))
    return ts, tl, trc, ql, ed, en, ctg, off


def edge_cases():
    """Hand-built pairs, each a list of (text_start, text_len, text_rc, query_len, edits, end) per mate; min_frag = 200,
    max_frag = 500.  A forward alignment's L is text_start + end - query_len, a reverse one's L is text_start + text_len - end."""
    B = 2 ** 32 - 1
    f = lambda left, m=100, e=0, slack=10: (left - 5, m + slack + 5, 0, m, e, m + 5)                    # noqa: E731  L = left
    r = lambda right, m=100, e=0, slack=10: (right - m - slack, m + slack + 5, 1, m, e, m + 5)            # noqa: E731  R = right
    cases = {
        "plain": ([f(1000)], [r(1400)]),                                          # fragment 400
        "mate 2 forward": ([r(1400)], [f(1000)]),
        "exactly min_frag": ([f(1000)], [r(1200)]),
        "one below min_frag": ([f(1000)], [r(1199)]),
        "exactly max_frag": ([f(1000)], [r(1500)]),
        "one beyond max_frag": ([f(1000)], [r(1501)]),
        "same strand": ([f(1000)], [f(1300)]),
        "both reverse": ([r(1100)], [r(1400)]),
        "dovetailed: the reverse mate begins left of the forward one": ([f(1000)], [r(1099 + 200, m=300)]),
        "dovetailed: the forward mate ends right of the reverse one": ([f(1000, m=300)], [r(1250)]),
        "contained at both ends is proper": ([f(1000, m=250)], [r(1250, m=250)]),
        "empty first group": ([], [r(1400)]),
        "empty second group": ([f(1000)], []),
        "both empty": ([], []),
        "all unknown": ([f(1000, e=B)], [r(1400)]),
        "one unknown among known": ([f(1000, e=B), f(1010, e=2)], [r(1400, e=1)]),
        "tie in the sum: the lowest i, then the lowest j": ([f(1000, e=1), f(1003, e=0)], [r(1400, e=0), r(1405, e=1), r(1410, e=0)]),
        "the pick is not the own winners": ([f(5000, e=0), f(1000, e=2)], [r(1400, e=1)]),
        "duplicate locus does not make an s2": ([f(1000), (990, 125, 0, 100, 0, 110)], [r(1400)]),
        "a second locus makes an s2": ([f(1000), f(1050, e=3)], [r(1400)]),
        "negative L": ([(0, 120, 0, 100, 0, 60)], [r(300)]),                       # end < query_len at text_start 0: L = -40
        "negative L beyond max_frag": ([(0, 120, 0, 100, 0, 60)], [r(461)]),
    }
    return cases


def flatten(cases, contig_of=None):
    ts, tl, trc, ql, ed, en, off = [], [], [], [], [], [], [0]
    for mates in cases:
        for mate in mates:
            for (s, w, rc, m, e, x) in mate:
                ts.append(s); tl.append(w); trc.append(rc); ql.append(m); ed.append(e); en.append(x)
            off.append(len(ts))
    return ts, tl, trc, ql, ed, en, off


def test_select_pairs_edge_cases():
    from bucket_map_amd import verify
    cases = edge_cases()
    ts, tl, trc, ql, ed, en, off = flatten(cases.values())
    got = verify.select_pairs(ts, tl, trc, ql, ed, en, off, 200, 500)
    want = brute_pairs(ts, tl, trc, ql, ed, en, off, 200, 500)
    assert_pairs_equal(got, want, "edge cases")
    assert all(got[k].dtype == t for k, t in (("pick", np.uint32), ("winner", np.uint32), ("proper", np.uint8), ("s1", np.uint64),
                                              ("s2", np.uint64)))
    proper = dict(zip(cases, got["proper"].tolist()))
    expect = {"plain": 1, "mate 2 forward": 1, "exactly min_frag": 1, "one below min_frag": 0, "exactly max_frag": 1,
              "one beyond max_frag": 0, "same strand": 0, "both reverse": 0,
              "dovetailed: the reverse mate begins left of the forward one": 0,
              "dovetailed: the forward mate ends right of the reverse one": 0, "contained at both ends is proper": 1,
              "empty first group": 0, "empty second group": 0, "both empty": 0, "all unknown": 0, "one unknown among known": 1,
              "tie in the sum: the lowest i, then the lowest j": 1, "the pick is not the own winners": 1,
              "duplicate locus does not make an s2": 1, "a second locus makes an s2": 1, "negative L": 1,
              "negative L beyond max_frag": 0}
    assert proper == expect
    p = list(cases).index("tie in the sum: the lowest i, then the lowest j")
    a0, b0 = off[2 * p], off[2 * p + 1]
    assert got["pick"][2 * p] == a0 + 1 and got["pick"][2 * p + 1] == b0 and got["s1"][p] == 0 and got["s2"][p] == 0
    p = list(cases).index("the pick is not the own winners")
    assert got["winner"][2 * p] == off[2 * p] and got["pick"][2 * p] == off[2 * p] + 1 and got["s1"][p] == 3
    p = list(cases).index("duplicate locus does not make an s2")
    assert got["s2"][p] == verify.PAIR_NONE and got["s1"][p] == 0
    p = list(cases).index("a second locus makes an s2")
    assert got["s2"][p] == 3
    p = list(cases).index("all unknown")
    assert got["pick"][2 * p] == verify.BEYOND and got["pick"][2 * p + 1] == off[2 * p + 1] and got["s1"][p] == verify.PAIR_NONE
    p = list(cases).index("negative L")
    assert got["s1"][p] == 0                                   # fragment 300 - (-40) = 340
    # the contig decides: the plain pair on two contigs is not proper, contig=None means one contig
    n = len(ts)
    ctg = np.zeros(n, np.uint32)
    ctg[off[1]] = 7
    assert verify.select_pairs(ts, tl, trc, ql, ed, en, off, 200, 500, ctg)["proper"][0] == 0
    assert_pairs_equal(verify.select_pairs(ts, tl, trc, ql, ed, en, off, 200, 500, ctg), brute_pairs(ts, tl, trc, ql, ed, en, off, 200, 500, ctg))
    with pytest.raises(ValueError):
        verify.select_pairs(ts, tl, trc, ql, ed, en, off[:-1], 200, 500)          # an odd number of groups
    with pytest.raises(ValueError):
        verify.select_pairs(ts, tl, trc, ql, ed, en, off, 501, 500)


def test_select_pairs_against_a_brute_force():
    from bucket_map_amd import verify
    rng = np.random.default_rng(20251001)
    ts, tl, trc, ql, ed, en, ctg, off = random_pairs(rng, 400)
    sizes = np.diff(off)
    assert (sizes == 0).any() and (sizes >= 5).any()
    seen = {"proper": 0, "s2": 0, "tie": 0, "not winners": 0}
    for contig in (ctg, None):
        for lo, hi in ((1, 1000), (300, 600), (0, 2 ** 32 - 1)):
            got = verify.select_pairs(ts, tl, trc, ql, ed, en, off, lo, hi, contig)
            want = brute_pairs(ts, tl, trc, ql, ed, en, off, lo, hi, contig)
            assert_pairs_equal(got, want, f"frag {lo}..{hi}, contig {'given' if contig is not None else 'None'}")
            seen["proper"] += int(got["proper"].sum())
            seen["s2"] += int((got["s2"] != verify.PAIR_NONE).sum())
            seen["tie"] += int((got["s2"] == got["s1"])[got["proper"] != 0].sum())
            seen["not winners"] += int((got["pick"] != got["winner"]).sum())
    assert all(v > 20 for v in seen.values()), seen


def test_pair_mapq():
    from bucket_map_amd import verify
    B, NONE = verify.BEYOND, verify.PAIR_NONE
    one = lambda pick, winner, edits, starts, margin=7: dict(pick=pick, winner=winner, edits=edits, end=[150] * len(edits),  # noqa: E731
                                                             text_start=starts, text_len=[160] * len(edits),
                                                             text_rc=[0] * len(edits), margin=margin)
    unique = one(0, 0, [2], [1000])
    repeat = one(1, 0, [2, 2], [1000, 5000])                   # the pick is the second copy, the own winner the first
    # not proper: each mate is best_mapq's
    assert verify.pair_mapq(0, NONE, NONE, [unique, one(0, 0, [2, 2], [1000, 5000])]) == [(60, 1), (0, 2)]
    # proper, no second combination: 60 for both, whatever the single-read view says; X0 counts the mate's own loci
    assert verify.pair_mapq(1, 4, NONE, [repeat, unique]) == [(60, 2), (60, 1)]
    # proper, a second combination at the same sum: the pair says 0, a unique mate keeps its own 60
    assert verify.pair_mapq(1, 4, 4, [repeat, unique]) == [(0, 2), (60, 1)]
    # the integer formula: M = 7 + 7, (s2 - s1) * 60 // 15
    assert verify.pair_mapq(1, 4, 5, [repeat, repeat])[0] == (4, 2)
    assert verify.pair_mapq(1, 4, 11, [repeat, repeat])[0] == (28, 2)
    assert verify.pair_mapq(1, 4, 400, [repeat, repeat])[0] == (60, 2)
    # q_single counts only when the pick is the own winner: picking the worse copy of two unequal ones gives q_pair alone
    worse = one(1, 0, [2, 5, B], [1000, 5000, 9000])
    better = one(0, 0, [2, 5, B], [1000, 5000, 9000])
    assert verify.pair_mapq(1, 7, 8, [worse, better]) == [(4, 1), (max(4, 3 * 60 // 8), 1)]
    # the same locus through two windows is one locus for X0
    twice = dict(pick=0, winner=0, edits=[2, 2], end=[150, 160], text_start=[1000, 990], text_len=[160, 170], text_rc=[0, 0], margin=7)
    assert verify.pair_mapq(1, 4, NONE, [twice, unique])[0] == (60, 1)


# ---- the tool ----
FRAG = (300, 800)
ARGS = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "4096", "-r", "150", "-f", "1"]
DUP_AT, DUP_LEN, COPY_AT = 8000, 1200, 21_000


def _revcomp(b):
    return bytes(b).translate(COMP)[::-1]


def make_paired_fixture(d, seed=11):
    """chrA: 30 kbp of random bases in which the 1 200 bases from 8 000 stand a second time at 21 000 -- in another bucket --,
    chrB: 9 kbp holding a third copy.  24 pairs of 150-base reads, fragments of 450 .. 700 bases: mate 1 lies inside the
    duplicated segment, mate 2 in unique sequence beside it.  Even pairs come from the first copy and odd ones from the second;
    every third pair has mate 1 as the reverse read (the fragment then extends to the LEFT of the segment).  Returns the truth
    per pair: (mate 1 forward?, 1-based POS of mate 1, of mate 2)."""
    rng = np.random.default_rng(seed)
    a = BASES[rng.integers(0, 4, 30_000)]
    a[COPY_AT: COPY_AT + DUP_LEN] = a[DUP_AT: DUP_AT + DUP_LEN]
    b = BASES[rng.integers(0, 4, 9_000)]
    b[3000: 3000 + DUP_LEN] = a[DUP_AT: DUP_AT + DUP_LEN]
    with open(d / "g.fa", "w") as f:
        f.write(f">chrA\n{bytes(a).decode()}\n>chrB\n{bytes(b).decode()}\n")
    truth = []
    with open(d / "pairs.fastq", "w") as f:
        for p in range(24):
            base = COPY_AT if p % 2 else DUP_AT
            frag = int(rng.integers(450, 701))
            if p % 3 == 2:                                     # mate 1 reverse at the segment's left end, the fragment leftwards
                m1 = base + int(rng.integers(0, 200))
                lo = m1 + 150 - frag
                m2 = lo
                s1, s2 = _revcomp(a[m1: m1 + 150]), bytes(a[m2: m2 + 150])
            else:                                              # mate 1 forward at the segment's right end
                m1 = base + DUP_LEN - 150 - int(rng.integers(0, 200))
                m2 = m1 + frag - 150
                s1, s2 = bytes(a[m1: m1 + 150]), _revcomp(a[m2: m2 + 150])
            assert not (base <= m2 < base + DUP_LEN - 100) and m2 + 150 <= base + DUP_LEN + 700 and m2 >= base - 700
            truth.append((p % 3 != 2, m1 + 1, m2 + 1))
            f.write(f"@p{p}/1\n{s1.decode()}\n+\n{'I' * 150}\n@p{p}/2\n{s2.decode()}\n+\n{'I' * 150}\n")
    # pairs in unique sequence of chrA, one candidate each (checked by the test that uses them)
    with open(d / "unique.fastq", "w") as f:
        for p in range(20):
            m1 = int(rng.integers(11_000, 19_000))
            frag = int(rng.integers(350, 700))
            s1, s2 = bytes(a[m1: m1 + 150]), _revcomp(a[m1 + frag - 150: m1 + frag])
            if p % 2:
                s1, s2 = s2, s1
            f.write(f"@u{p}/1\n{s1.decode()}\n+\n{'I' * 150}\n@u{p}/2\n{s2.decode()}\n+\n{'I' * 150}\n")
    # one pair whose second mate is random bases, one whose first is
    with open(d / "lonely.fastq", "w") as f:
        m1 = 15_000
        junk = bytes(BASES[rng.integers(0, 4, 150)])
        f.write(f"@l0/1\n{bytes(a[m1: m1 + 150]).decode()}\n+\n{'I' * 150}\n@l0/2\n{junk.decode()}\n+\n{'I' * 150}\n")
        f.write(f"@l1/1\n{junk[::-1].decode()}\n+\n{'I' * 150}\n@l1/2\n{_revcomp(a[m1 + 400: m1 + 550]).decode()}\n+\n{'I' * 150}\n")
    return truth


@pytest.fixture(scope="module")
def paired(tmp_path_factory):
    d = tmp_path_factory.mktemp("pair")
    return d, make_paired_fixture(d)


def run_tool(exe, d, fastq, out, *extra, ok=True, block="5"):
    env = dict(os.environ, BM_VERIFY_BLOCK_READS=block)
    r = subprocess.run([exe, *ARGS, "-q", fastq, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def records(path):
    return [l.split("\t") for l in open(path).read().split("\n") if l and not l.startswith("@")]


def ref_len(cigar):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MDN=X")


def test_tool_places_the_repeat_mate_beside_its_partner(paired):
    d, truth = paired
    frag = ["--frag-range", f"{FRAG[0]},{FRAG[1]}"]
    run_tool(TOOL, d, "pairs.fastq", "best.sam", "--best")
    best = records(d / "best.sam")
    # the precondition: under --best the tool locates BOTH mates of every constructed pair ...
    assert [r[0] for r in best] == [f"p{p}/{k}" for p in range(24) for k in (1, 2)]
    # ... and a mate inside the duplicate is a tie it cannot break: MAPQ 0, three loci
    for p in range(24):
        m1, m2 = best[2 * p], best[2 * p + 1]
        assert m1[4] == "0" and m1[-1] == "X0:i:3", m1
        assert m2[4] == "60" and m2[-1] == "X0:i:1", m2
    run_tool(TOOL, d, "pairs.fastq", "paired.sam", *frag)
    got = records(d / "paired.sam")
    assert len(got) == 48
    for p, (m1_forward, pos1, pos2) in enumerate(truth):
        m1, m2 = got[2 * p], got[2 * p + 1]
        assert m1[0] == m2[0] == f"p{p}", "QNAME without /1 and /2"
        f1, f2 = int(m1[1]), int(m2[1])
        assert f1 == (0x1 | 0x2 | 0x40 | (0x20 if m1_forward else 0x10)), (p, f1)
        assert f2 == (0x1 | 0x2 | 0x80 | (0x10 if m1_forward else 0x20)), (p, f2)
        assert m1[2] == m2[2] == "chrA" and int(m1[3]) == pos1 and int(m2[3]) == pos2, (p, m1[:4], m2[:4])
        assert int(m1[4]) == 60 and int(m2[4]) == 60, "no second proper combination: the other copies have no mate in range"
        assert m1[6] == m2[6] == "=" and int(m1[7]) == pos2 and int(m2[7]) == pos1
        lo, hi = min(pos1, pos2), max(pos1 + ref_len(m1[5]), pos2 + ref_len(m2[5]))
        assert int(m1[8]) == (hi - lo if pos1 < pos2 else lo - hi) and int(m2[8]) == -int(m1[8])
        assert FRAG[0] <= abs(int(m1[8])) <= FRAG[1]
        assert m1[5] == m2[5] == "150=" and "NM:i:0" in m1 and m1[-1] == "X0:i:3" and m2[-1] == "X0:i:1"
    # --paired alone takes the default range 1,1000; blocks of any size are cut between pairs
    run_tool(TOOL, d, "pairs.fastq", "default.sam", "--paired", block="1")
    run_tool(TOOL, d, "pairs.fastq", "wide.sam", "--frag-range=1,1000", block="1000")
    assert open(d / "default.sam").read() == open(d / "wide.sam").read()
    assert [r[:9] for r in records(d / "default.sam")] == [r[:9] for r in got]
    # a range no fragment falls into: nothing is proper, every mate is what --best makes of it
    run_tool(TOOL, d, "pairs.fastq", "narrow.sam", "--frag-range", "1,100")
    for r in records(d / "narrow.sam"):
        assert int(r[1]) & 0x2 == 0 and int(r[1]) & 0x1
    assert [r[4] for r in records(d / "narrow.sam")] == [r[4] for r in best]


def test_tool_mate_without_a_record(paired):
    d, _ = paired
    run_tool(TOOL, d, "lonely.fastq", "lonely.sam", "--paired")
    got = records(d / "lonely.sam")
    assert [r[0] for r in got] == ["l0", "l1"]
    assert int(got[0][1]) == 0x1 | 0x8 | 0x40 and int(got[1][1]) == 0x1 | 0x8 | 0x80 | 0x10
    for r in got:
        assert r[6:9] == ["*", "0", "0"] and r[4] == "60"


def test_tool_refusals(paired):
    d, _ = paired
    lines = open(d / "unique.fastq").read().split("\n")
    open(d / "odd.fastq", "w").write("\n".join(lines[:12]) + "\n")                 # three records
    r = run_tool(TOOL, d, "odd.fastq", "never.sam", "--paired", ok=False)
    assert "odd.fastq" in r.stderr and "odd number" in r.stderr
    lines[4] = "@someone_else/2"
    open(d / "names.fastq", "w").write("\n".join(lines))
    r = run_tool(TOOL, d, "names.fastq", "never2.sam", "--paired", ok=False)
    assert "records 0 and 1" in r.stderr and "someone_else" in r.stderr and "not mates" in r.stderr
    for bad in (["--frag-range", "500,100"], ["--frag-range", "500"], ["--frag-range=a,b"]):
        r = run_tool(TOOL, d, "unique.fastq", "never3.sam", *bad, ok=False)
        assert "Value parse failed for --frag-range" in r.stderr and not os.path.exists(d / "never3.sam")
    # the tool without alignment refuses the flag as a parser error
    for flag in (["--paired"], ["--frag-range", "1,1000"]):
        r = run_tool(PLAIN_TOOL, d, "unique.fastq", "never4.sam", *flag, ok=False)
        assert r.returncode == 255 and "belongs to bucketmap_align" in r.stderr and not os.path.exists(d / "never4.sam")


def test_tool_without_the_flag_is_what_it_was(paired):
    """Pairs with exactly one candidate per mate: --paired differs from --best --annotate only in the pair fields (and the
    QNAME's /1, /2)."""
    d, _ = paired
    env = dict(os.environ, BM_DUMP_ALIGNMENTS=str(d / "u_dump.txt"))
    r = subprocess.run([TOOL, *ARGS, "-q", "unique.fastq", "-o", "u_all.sam"], cwd=str(d), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    per_read = [int(l.split()[0]) for l in open(d / "u_dump.txt").read().split("\n") if l]
    assert per_read == list(range(40)), "the fixture must give every mate exactly one candidate"
    run_tool(TOOL, d, "unique.fastq", "u_best.sam", "--best", "--annotate")
    run_tool(TOOL, d, "unique.fastq", "u_paired.sam", "--paired")
    best, pair = records(d / "u_best.sam"), records(d / "u_paired.sam")
    assert len(best) == len(pair) == 40
    for b, p in zip(best, pair):
        assert int(p[1]) & 0x3 == 0x3 and p[6] == "=" and int(p[8]) != 0
        stripped = [b[0][:-2], str(int(p[1]) & 0x10), *p[2:6], "*", "0", "0", *p[9:]]
        assert [b[0][:-2], *b[1:]] == stripped
    assert open(d / "u_best.sam").read().split("\n")[:3] == open(d / "u_paired.sam").read().split("\n")[:3]     # the header
