"""The annotation pass without a GPU: the MD and CIGAR formatters on hand-worked cases, the plain-Python restatement of
bmv_annotate's contract (include/bmv.h) that tests/test_annotate_gpu.py compares the device against -- pinned here on the
same cases --, the ABI surface, and the tools' --annotate option.

The restatement shares nothing with the kernels: it builds the alignment column by column in the ALIGNER's frame (the
window reverse-complemented when text_rc), and only then turns the column list round for the forward strand; the
kernels walk forward from the start."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = {
    "bucketmap": os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle"),
    "bucketmap_align": os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle"),
}
M, I, D, EQ, X = 0, 1, 2, 7, 8
RANK = {**{c: 1 for c in b"CcYySsBb"}, **{c: 2 for c in b"GgKk"}, **{c: 3 for c in b"TtUu"}}     # every other byte: 0


def rank(c) -> int:
    return RANK.get(int(c), 0)


def pack(entries):
    return np.array([(n << 4) | op for op, n in entries], np.uint32)


def restate(window, rc, query, begin, cigar):
    """window: the text window as it lies in the genome (forward strand); query: the read as sequenced; begin and cigar
    ((op, length) pairs, M/I/D, 5' to 3' of the query) as the aligner returns them.
    Returns (pos, ref_len, xcigar as (op, length) pairs, nm, ref_bases as bytes, md)."""
    if not cigar:
        return 0, 0, [], 0, b"", "0"
    t = [rank(c) for c in window]
    if rc:
        t = [3 - r for r in reversed(t)]                     # what the aligner compared against
    q = [rank(c) for c in query]
    cols, ti, qi = [], begin, 0                              # (op, text rank under the column or None)
    for op, n in cigar:
        for _ in range(n):
            if op == I:
                cols.append((I, None))
                qi += 1
            elif op == D:
                cols.append((D, t[ti]))
                ti += 1
            else:
                cols.append((EQ if t[ti] == q[qi] else X, t[ti]))
                ti += 1
                qi += 1
    assert qi == len(query) and ti <= len(window)
    ref_len = ti - begin
    pos = begin
    if rc:                                                   # the same columns read along the forward strand
        cols = [(op, None if r is None else 3 - r) for op, r in reversed(cols)]
        pos = len(window) - begin - ref_len
    xc = []
    for op, _ in cols:
        if xc and xc[-1][0] == op:
            xc[-1][1] += 1
        else:
            xc.append([op, 1])
    nm = sum(1 for op, _ in cols if op != EQ)
    ref = bytes(b"ACGT"[r] for op, r in cols if op in (X, D))
    # MD: one count before every X base, one count and one '^' before every D entry
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
    md += str(run)
    return pos, ref_len, [tuple(e) for e in xc], nm, ref, md


#  name, window (forward), rc, query, begin, M/I/D CIGAR -> pos, xcigar, nm, ref_bases, md, CIGAR text: worked by hand
CASES = [
    ("all matches", b"ACGTACGTAC", 0, b"ACGTACGTAC", 0, [(M, 10)],
     0, [(EQ, 10)], 0, b"", "10", "10="),
    ("a mismatch at the first and at the last column", b"ACGTACGTAC", 0, b"CCGTACGTAG", 0, [(M, 10)],
     0, [(X, 1), (EQ, 8), (X, 1)], 2, b"AC", "0A8C0", "1X8=1X"),
    ("two adjacent mismatches", b"GGGACTTTTT", 0, b"GGGTGTTTTT", 0, [(M, 10)],
     0, [(EQ, 3), (X, 2), (EQ, 5)], 2, b"AC", "3A0C5", "3=2X5="),
    ("a deletion followed at once by a mismatch", b"GGGGACTGGG", 0, b"GGGGAGGG", 0, [(M, 4), (D, 2), (M, 4)],
     0, [(EQ, 4), (D, 2), (X, 1), (EQ, 3)], 3, b"ACT", "4^AC0T3", "4=2D1X3="),
    ("an insertion between matches", b"ACGTAC", 0, b"ACGTTTAC", 0, [(M, 4), (I, 2), (M, 2)],
     0, [(EQ, 4), (I, 2), (EQ, 2)], 2, b"", "6", "4=2I2="),
    ("a deletion after an insertion", b"TTACGTCAGG", 0, b"ACGGGAG", 2, [(M, 3), (I, 2), (D, 2), (M, 2)],
     2, [(EQ, 3), (I, 2), (D, 2), (EQ, 2)], 4, b"TC", "3^TC2", "3=2I2D2="),
    # reverse strand: the aligner saw revcomp(window) = CCTGACGTAA and, from begin 3, GA|CGT against the query GA T CCT:
    # = = I = X(G) =.  R = 5, pos = 10 - 3 - 5 = 2; along the forward strand the columns come in reverse, window[2:7] =
    # ACGTC against revcomp(query) = AGGATC: = X(C) = I = =
    ("reverse strand", b"TTACGTCAGG", 1, b"GATCCT", 3, [(M, 2), (I, 1), (M, 3)],
     2, [(EQ, 1), (X, 1), (EQ, 1), (I, 1), (EQ, 2)], 2, b"C", "1C3", "1=1X1=1I2="),
    ("N and lower case fold", b"ANgtRY", 0, b"aAGTAC", 0, [(M, 6)],
     0, [(EQ, 6)], 0, b"", "6", "6="),
    ("an N under X and under D is written A", b"CNCNC", 0, b"CCC", 0, [(M, 2), (D, 2), (M, 1)],
     0, [(EQ, 1), (X, 1), (D, 2), (EQ, 1)], 3, b"ACA", "1A0^CA1", "1=1X2D1="),
    ("empty CIGAR", b"ACGT", 1, b"ACGT", 0, [],
     0, [], 0, b"", "0", ""),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_formatters_on_hand_worked_cases(case):
    from bucket_map_amd import verify
    _, _, _, _, _, _, _, xc, _, ref, md, text = case
    assert verify.md_string(pack(xc), np.frombuffer(ref, np.uint8)) == md
    assert verify.xcigar_string(pack(xc)) == text
    assert verify.md_string(pack(xc), ref) == md              # bytes are taken too


def test_md_string_refuses_bases_that_do_not_fit():
    from bucket_map_amd import verify
    with pytest.raises(ValueError):
        verify.md_string(pack([(EQ, 3), (X, 1)]), b"AC")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_on_hand_worked_cases(case):
    """The yardstick of the GPU tests, held to the same hand-worked answers."""
    _, window, rc, query, begin, cigar, pos, xc, nm, ref, md, _ = case
    got = restate(window, rc, query, begin, cigar)
    ref_len = sum(n for op, n in cigar if op != I)
    assert got == (pos, ref_len, xc, nm, ref, md)


def test_reverse_strand_case_is_what_it_claims():
    """The hand-worked reverse-strand case, checked independently: the forward view of the alignment aligns
    revcomp(query) to window[pos:] with the reversed CIGAR."""
    window, query = b"TTACGTCAGG", b"GATCCT"
    rq = bytes(query.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1])
    assert rq == b"AGGATC"
    fwd = restate(window, 0, rq, 2, [(M, 3), (I, 1), (M, 2)])
    assert fwd == restate(window, 1, query, 3, [(M, 2), (I, 1), (M, 3)])


def test_header_and_binding_agree_on_the_new_symbols():
    from bucket_map_amd import verify
    text = open(os.path.join(ROOT, "include", "bmv.h")).read()
    assert re.search(r"BMV_OP_EQ\s*=\s*7\b", text) and re.search(r"BMV_OP_X\s*=\s*8\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = verify.lib()
    for name in ("bmv_annotate", "bmv_annotations", "bmv_last_annotate_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
        n_args = len(re.search(rf"\b{name}\s*\((.*?)\)", text, flags=re.S).group(1).split(","))
        assert n_args == len(verify.SYMBOLS[name][1]), name
    assert callable(verify.Verifier.annotate) and callable(verify.Verifier.annotate_stats)


def test_entry_points_fail_cleanly_without_a_context():
    from bucket_map_amd import verify
    L = verify.lib()
    a, b = C.c_uint64(), C.c_uint64()
    assert L.bmv_annotate(None, None, 0, None, None, None, None, None, None, None, None, 0, C.byref(a), C.byref(b)) == 1
    assert b"bmv_annotate" in L.bmv_last_error()
    assert L.bmv_annotations(None, None, None, None, None, None, None, None) == 1
    assert b"bmv_annotations" in L.bmv_last_error()
    assert L.bmv_last_annotate_stats(None, None, None) == 1
    assert b"bmv_last_annotate_stats" in L.bmv_last_error()


@pytest.mark.parametrize("tool", ["bucketmap", "bucketmap_align"])
def test_option_is_parsed_by_both_tools(tool, tmp_path):
    def run(*extra):
        return subprocess.run([TOOLS[tool], "-i", "idx", *extra], cwd=str(tmp_path), capture_output=True, text=True)
    r = run("--annotate")                                        # parsed; what fails next is the missing genome
    assert r.returncode != 0 and "Unknown option" not in r.stderr and "BM_GENOME_FILE is not found" in r.stderr, r.stderr
    r = run("--annotate", "--max-edit-rate=0.1")
    assert "Unknown option" not in r.stderr and "BM_GENOME_FILE is not found" in r.stderr, r.stderr
    r = run("--annotat")
    assert r.returncode != 0 and "Unknown option --annotat" in r.stderr
