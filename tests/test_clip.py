"""The clipping pass without a GPU: the plain-Python restatement of bmv_clip's contract (include/bmv.h) that
tests/test_clip_gpu.py compares the device against -- built on test_annotate.restate, its range found by brute force over
all (l, r) and by a single pass that are held against each other --, hand-worked cases on both strands, the formatters with
S entries, the ABI surface, and the tools' --clip / --clip-scores options."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_annotate import D, EQ, I, M, X, pack, restate

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = {
    "bucketmap": os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle"),
    "bucketmap_align": os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle"),
}
S = 4


def range_brute(w):
    """(score, l, r) over all 0 <= l <= r <= C: the greatest P[r] - P[l], then the smallest r, then the largest l."""
    P = [0]
    for x in w:
        P.append(P[-1] + x)
    best = (0, 0, 0)
    for r in range(len(P)):
        for l in range(r + 1):
            s, (bs, bl, br) = P[r] - P[l], best
            if s > bs or (s == bs and (r < br or (r == br and l > bl))):
                best = (s, l, r)
    return best


def range_scan(w):
    """The same in one pass: the least P so far at its latest index, the best replaced only by a greater score."""
    p = low = low_at = best = best_l = best_r = 0
    for i, x in enumerate(w):
        p += x
        if p <= low:
            low, low_at = p, i + 1
        if p - low > best:
            best, best_l, best_r = p - low, low_at, i + 1
    return best, best_l, best_r


def _md(xc, ref):
    md, run, at = "", 0, 0
    for op, n in xc:
        if op == EQ:
            run += n
        elif op == X:
            for k in range(n):
                md += f"{run}{chr(ref[at + k])}"
                run = 0
            at += n
        elif op == D:
            md += f"{run}^{ref[at: at + n].decode()}"
            run = 0
            at += n
    return md + str(run)


def restate_clip(window, rc, query, begin, cigar, match=1, penalty=2, find=range_scan):
    """bmv_clip's outputs for one alignment, from test_annotate.restate's forward-strand entries: a dict of score,
    clip_left, clip_right, pos, ref_len, nm, xcigar ((op, length) pairs), ref_bases, md."""
    pos, _, xc, _, ref, _ = restate(window, rc, query, begin, cigar)
    none = dict(score=0, clip_left=0, clip_right=0, pos=0, ref_len=0, nm=0, xcigar=[], ref_bases=b"", md="0")
    if not cigar:
        return none
    cols = [op for op, n in xc for _ in range(n)]
    score, l, r = find([match if op == EQ else -penalty for op in cols])
    if l == r:
        return dict(none, clip_right=len(query), xcigar=[(S, len(query))] if len(query) else [])
    before, kept, after = cols[:l], cols[l:r], cols[r:]
    left, right = sum(1 for op in before if op != D), sum(1 for op in after if op != D)
    ref_at = sum(1 for op in before if op in (X, D))
    k_ref = ref[ref_at: ref_at + sum(1 for op in kept if op in (X, D))]
    runs = []
    for op in kept:
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    runs = [tuple(e) for e in runs]
    assert left + sum(1 for op in kept if op != D) + right == len(query)
    return dict(score=score, clip_left=left, clip_right=right, pos=pos + sum(1 for op in before if op != I),
                ref_len=sum(1 for op in kept if op != I), nm=sum(1 for op in kept if op != EQ),
                xcigar=([(S, left)] if left else []) + runs + ([(S, right)] if right else []), ref_bases=k_ref, md=_md(runs, k_ref))


# name, window (forward), rc, query, begin, M/I/D CIGAR, (match, penalty)
#   -> score, clip_left, clip_right, pos, ref_len, nm, xcigar, ref_bases, md: worked by hand
CASES = [
    ("clean: nothing clipped", b"ACGTACGTAC", 0, b"ACGTACGTAC", 0, [(M, 10)], (1, 2),
     10, 0, 0, 0, 10, 0, [(EQ, 10)], b"", "10"),
    ("an edit inside stays", b"ACGTACGTACGTAC", 0, b"ACGTACCTACGTAC", 0, [(M, 14)], (1, 2),
     11, 0, 0, 0, 14, 1, [(EQ, 6), (X, 1), (EQ, 7)], b"G", "6G7"),
    # X 8= X
    ("a leading and a trailing X clipped", b"ACGTACGTAC", 0, b"CCGTACGTAG", 0, [(M, 10)], (1, 2),
     8, 1, 1, 1, 8, 0, [(S, 1), (EQ, 8), (S, 1)], b"", "8"),
    ("a trailing I run clipped", b"ACGTAC", 0, b"ACGTACTTT", 0, [(M, 6), (I, 3)], (1, 2),
     6, 0, 3, 0, 6, 0, [(EQ, 6), (S, 3)], b"", "6"),
    ("a D at the border: pos shifts, no query base clipped", b"TTACGTAC", 0, b"ACGTAC", 0, [(D, 2), (M, 6)], (1, 2),
     6, 0, 0, 2, 6, 0, [(EQ, 6)], b"", "6"),
    # 4= 2D 1X 3=: P = 4, 0, -2, 1 at the run ends; [0, 4) scores 4, [7, 10) only 3
    ("cut before a D", b"GGGGACTGGG", 0, b"GGGGAGGG", 0, [(M, 4), (D, 2), (M, 4)], (1, 2),
     4, 0, 4, 0, 4, 0, [(EQ, 4), (S, 4)], b"", "4"),
    # the same under 2 / 1: 8 - 2 - 1 + 6 = 11, everything kept
    ("other scores keep the D", b"GGGGACTGGG", 0, b"GGGGAGGG", 0, [(M, 4), (D, 2), (M, 4)], (2, 1),
     11, 0, 0, 0, 10, 3, [(EQ, 4), (D, 2), (X, 1), (EQ, 3)], b"ACT", "4^AC0T3"),
    # = = X X = =: P = 0 1 2 0 -2 -1 0; [0, 2) and [4, 6) both score 2
    ("two equal maxima: the smallest r", b"ACGTAC", 0, b"ACTGAC", 0, [(M, 6)], (1, 2),
     2, 0, 4, 0, 2, 0, [(EQ, 2), (S, 4)], b"", "2"),
    # = = X = = =: P = 0 1 2 0 1 2 3; P[6] - P[0] = P[6] - P[3] = 3
    ("two equal minima: the largest l", b"ACGTAC", 0, b"ACTTAC", 0, [(M, 6)], (1, 2),
     3, 3, 0, 3, 3, 0, [(S, 3), (EQ, 3)], b"", "3"),
    ("all mismatches: the empty range, one S", b"AAAA", 0, b"CCCC", 0, [(M, 4)], (1, 2),
     0, 0, 4, 0, 0, 0, [(S, 4)], b"", "0"),
    ("a zero-length query", b"ACGT", 0, b"", 0, [], (1, 2),
     0, 0, 0, 0, 0, 0, [], b"", "0"),
    # reverse strand.  test_annotate's case: forward entries from pos 2 are = X = I = =, P = 0 1 -1 0 -2 -1 0: [4, 6) scores 2;
    # four query bases (=, X, =, I) and three reference bases lie before it
    ("reverse strand: the leading columns clipped", b"TTACGTCAGG", 1, b"GATCCT", 3, [(M, 2), (I, 1), (M, 3)], (1, 2),
     2, 4, 0, 5, 2, 0, [(S, 4), (EQ, 2)], b"", "2"),
    # the aligner saw GTACGT and a trailing insertion; along the forward strand the insertion comes first
    ("reverse strand: the read's trailing I run is the left clip", b"ACGTAC", 1, b"GTACGTAAA", 0, [(M, 6), (I, 3)], (1, 2),
     6, 3, 0, 0, 6, 0, [(S, 3), (EQ, 6)], b"", "6"),
    # revcomp(window) = GTACGTAA: 6 M then 2 D; forward D D 6=
    ("reverse strand: a D at the border", b"TTACGTAC", 1, b"GTACGT", 0, [(M, 6), (D, 2)], (1, 2),
     6, 0, 0, 2, 6, 0, [(EQ, 6)], b"", "6"),
    # the reads are the reverse complements of ACTGAC and ACTTAC: the forward columns of the two tie cases above
    ("reverse strand: two equal maxima", b"ACGTAC", 1, b"GTCAGT", 0, [(M, 6)], (1, 2),
     2, 0, 4, 0, 2, 0, [(EQ, 2), (S, 4)], b"", "2"),
    ("reverse strand: two equal minima", b"ACGTAC", 1, b"GTAAGT", 0, [(M, 6)], (1, 2),
     3, 3, 0, 3, 3, 0, [(S, 3), (EQ, 3)], b"", "3"),
    ("reverse strand: all mismatches", b"AAAA", 1, b"CCCC", 0, [(M, 4)], (1, 2),
     0, 0, 4, 0, 0, 0, [(S, 4)], b"", "0"),
    ("reverse strand: clean", b"ACGTACGTAC", 1, b"GTACGTACGT", 0, [(M, 10)], (1, 2),
     10, 0, 0, 0, 10, 0, [(EQ, 10)], b"", "10"),
]
KEYS = ("score", "clip_left", "clip_right", "pos", "ref_len", "nm", "xcigar", "ref_bases", "md")


@pytest.mark.parametrize("find", [range_brute, range_scan], ids=["brute force", "single pass"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_on_hand_worked_cases(case, find):
    """The yardstick of the GPU tests, held to the hand-worked answers with either range finder."""
    _, window, rc, query, begin, cigar, (match, penalty) = case[:7]
    got = restate_clip(window, rc, query, begin, cigar, match, penalty, find)
    assert got == dict(zip(KEYS, case[7:]))


def test_single_pass_agrees_with_brute_force():
    """A few hundred random small alignments under several scores: the single pass, which the large GPU cases are held
    to, finds the range brute force finds."""
    rng = np.random.default_rng(51)
    ties = 0
    for _ in range(400):
        cigar, last = [], None
        for _ in range(int(rng.integers(1, 6))):
            op = int(rng.choice([o for o in (M, I, D) if o != last]))
            cigar.append((op, int(rng.integers(1, 9 if op == M else 4))))
            last = op
        rc, begin = int(rng.integers(0, 2)), int(rng.integers(0, 3))
        window = bytes(rng.choice(list(b"AC"), begin + sum(n for op, n in cigar if op != I) + int(rng.integers(0, 3))).astype(np.uint8))
        query = bytes(rng.choice(list(b"ACgt"), sum(n for op, n in cigar if op != D)).astype(np.uint8))
        for match, penalty in ((1, 1), (1, 2), (3, 2), (1024, 1), (1, 1024)):
            a = restate_clip(window, rc, query, begin, cigar, match, penalty, range_brute)
            assert a == restate_clip(window, rc, query, begin, cigar, match, penalty, range_scan), (window, rc, query, begin, cigar)
            kept = [e for e in a["xcigar"] if e[0] != S]
            assert not kept or (kept[0][0] == EQ and kept[-1][0] == EQ), "a non-empty range begins and ends on an = column"
            assert a["pos"] + a["ref_len"] <= len(window)
            ties += a["score"] > 0 and len(kept) < len(restate(window, rc, query, begin, cigar)[2])
    assert ties > 100, "hardly any alignment was cut: the comparison shows little"


def test_formatters_with_soft_clips():
    from bucket_map_amd import verify
    for case in CASES:
        xc, ref, md = case[13], case[14], case[15]
        assert verify.md_string(pack(xc), ref) == md, case[0]
        assert verify.xcigar_string(pack(xc)) == "".join(f"{n}{'MIDNSHP=X'[op]}" for op, n in xc), case[0]
    assert verify.xcigar_string(pack([(S, 3), (EQ, 5), (X, 1), (I, 2), (D, 1), (EQ, 4), (S, 7)])) == "3S5=1X2I1D4=7S"
    assert verify.md_string(pack([(S, 3), (EQ, 5), (X, 1), (I, 2), (D, 2), (EQ, 4), (S, 7)]), b"GAC") == "5G0^AC4"
    assert verify.md_string(pack([(S, 9)]), b"") == "0"


def test_header_and_binding_agree_on_the_new_symbols():
    from bucket_map_amd import verify
    text = open(os.path.join(ROOT, "include", "bmv.h")).read()
    assert re.search(r"BMV_OP_S\s*=\s*4\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = verify.lib()
    for name in ("bmv_clip", "bmv_clipped", "bmv_last_clip_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
        n_args = len(re.search(rf"\b{name}\s*\((.*?)\)", text, flags=re.S).group(1).split(","))
        assert n_args == len(verify.SYMBOLS[name][1]), name
    assert callable(verify.Verifier.clip) and callable(verify.Verifier.clip_stats)


def test_entry_points_fail_cleanly_without_a_context():
    from bucket_map_amd import verify
    L = verify.lib()
    a, b = C.c_uint64(), C.c_uint64()
    assert L.bmv_clip(None, None, 0, None, None, None, None, None, None, None, None, 0, 1, 2, C.byref(a), C.byref(b)) == 1
    assert b"bmv_clip" in L.bmv_last_error()
    assert L.bmv_clipped(None, None, None, None, None, None, None, None, None, None, None) == 1
    assert b"bmv_clipped" in L.bmv_last_error()
    assert L.bmv_last_clip_stats(None, None, None) == 1
    assert b"bmv_last_clip_stats" in L.bmv_last_error()


@pytest.mark.parametrize("tool", ["bucketmap", "bucketmap_align"])
def test_options_are_parsed_by_both_tools(tool, tmp_path):
    def run(*extra):
        return subprocess.run([TOOLS[tool], "-i", "idx", *extra], cwd=str(tmp_path), capture_output=True, text=True)
    for ok in (["--clip"], ["--clip-scores", "2,3"], ["--clip-scores=2,3"], ["--clip", "--clip-scores", "1024,1", "--annotate"]):
        r = run(*ok)                                             # parsed; what fails next is the missing genome
        assert r.returncode != 0 and "Unknown option" not in r.stderr and "BM_GENOME_FILE is not found" in r.stderr, r.stderr
    for bad in ("0,1", "1,0", "1025,1", "1,1025", "2", "2,", "a,b"):
        r = run("--clip-scores", bad)
        assert r.returncode != 0 and "--clip-scores" in r.stderr and "BM_GENOME_FILE" not in r.stderr, (bad, r.stderr)
    r = run("--cli")
    assert r.returncode != 0 and "Unknown option --cli" in r.stderr
