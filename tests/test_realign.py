"""The affine-gap realignment pass without a GPU: the plain-Python restatement of bmv_realign's contract (include/bmv.h)
that tests/test_realign_gpu.py compares the device against -- a dictionary of present cells with the three states H, Ins
and Del --, a second, independent formulation held against it (H as a maximum over whole gaps of every length, no Ins / Del
matrices), hand-worked cases, the ABI surface, the tools' options, and `bucketmap_align --affine` through the oracle-backed
tool, whose verifier takes alignment_verifier::realign's default (host/affine_realign.h)."""
import ctypes as C
import os
import re
import subprocess
from functools import lru_cache

import numpy as np
import pytest

from test_annotate import D, I, M, rank

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = {
    "bucketmap": os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle"),
    "bucketmap_align": os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle"),
}
COMP = bytes.maketrans(b"ACGT", b"TGCA")
DEFAULT = (1, 4, 6, 1)


def _frame(window, rc, query):
    """Ranks of the text as the aligner saw it, and of the query."""
    t = [rank(c) for c in window]
    if rc:
        t = [3 - r for r in reversed(t)]
    return t, [rank(c) for c in query]


def path_rows(begin, cigar, m):
    """p(i) and q(i) of the given path: the first and the last column it visits in row i."""
    p, q, i, j = [begin] + [0] * m, [begin] + [0] * m, 0, begin
    for op, n in cigar:
        for _ in range(n):
            if op == D:
                j += 1
                q[i] = j
            else:
                i += 1
                j += op == M
                p[i] = q[i] = j
    assert i == m
    return p, q


def path_score(window, rc, query, begin, cigar, scores=DEFAULT):
    """The affine score of a path: +match per equal M column, -mismatch per unequal one, -(open + L ext) per I or D entry."""
    a, b, o, e = scores
    t, qr = _frame(window, rc, query)
    s, i, j = 0, 0, begin
    for op, n in cigar:
        if op == M:
            s += sum(a if t[j + x] == qr[i + x] else -b for x in range(n))
            i, j = i + n, j + n
        else:
            s -= o + n * e
            i, j = (i + n, j) if op == I else (i, j + n)
    return s


def _runs(ops_reversed):
    out = []
    for op in reversed(ops_reversed):
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    return [tuple(x) for x in out]


def _band(begin, cigar, m, n, w):
    p, q = path_rows(begin, cigar, m)
    return [(max(0, p[i] - w), min(n, q[i] + w)) for i in range(m + 1)], max(q[i] - p[i] for i in range(m + 1))


def restate_realign(window, rc, query, begin, cigar, scores=DEFAULT, band=16):
    """bmv_realign's outputs for one alignment: a dict of score, begin, realigned and cigar ((op, length) pairs).  The three
    matrices as dictionaries of present cells; an absent cell has no key."""
    a, b, o, e = scores
    m, n = len(query), len(window)
    if not cigar:
        return dict(score=0, begin=begin, realigned=0, cigar=[])
    rows, longest = _band(begin, cigar, m, n, band)
    if longest > 63 - 2 * band:
        return dict(score=path_score(window, rc, query, begin, cigar, scores), begin=begin, realigned=0, cigar=list(cigar))
    t, qr = _frame(window, rc, query)
    H, Ins, Del = {}, {}, {}
    for j in range(rows[0][0], rows[0][1] + 1):
        H[0, j] = 0
    for i in range(1, m + 1):
        for j in range(rows[i][0], rows[i][1] + 1):
            ins = [v for v in (H[i - 1, j] - o - e if (i - 1, j) in H else None, Ins[i - 1, j] - e if (i - 1, j) in Ins else None)
                   if v is not None]
            if ins:
                Ins[i, j] = max(ins)
            dele = [v for v in (H[i, j - 1] - o - e if (i, j - 1) in H else None, Del[i, j - 1] - e if (i, j - 1) in Del else None)
                    if v is not None]
            if dele:
                Del[i, j] = max(dele)
            h = [v for v in (H[i - 1, j - 1] + (a if qr[i - 1] == t[j - 1] else -b) if (i - 1, j - 1) in H else None,
                             Ins.get((i, j)), Del.get((i, j))) if v is not None]
            if h:
                H[i, j] = max(h)
    score = max(H[m, j] for j in range(rows[m][0], rows[m][1] + 1) if (m, j) in H)
    j = max(j for j in range(rows[m][0], rows[m][1] + 1) if H.get((m, j)) == score)      # tie rule (1): the last column
    i, state, ops = m, "H", []
    while not (state == "H" and i == 0):
        if state == "H":
            if (i - 1, j - 1) in H and H[i, j] == H[i - 1, j - 1] + (a if qr[i - 1] == t[j - 1] else -b):
                ops.append(M)
                i, j = i - 1, j - 1
            elif Ins.get((i, j)) == H[i, j]:
                state = "I"
            else:
                assert Del[i, j] == H[i, j]
                state = "D"
        elif state == "I":
            ops.append(I)
            opens = (i - 1, j) in H and Ins[i, j] == H[i - 1, j] - o - e                # a tie goes to "open"
            assert opens or Ins[i, j] == Ins[i - 1, j] - e
            i, state = i - 1, "H" if opens else "I"
        else:
            ops.append(D)
            opens = (i, j - 1) in H and Del[i, j] == H[i, j - 1] - o - e
            assert opens or Del[i, j] == Del[i, j - 1] - e
            j, state = j - 1, "H" if opens else "D"
    return dict(score=score, begin=j, realigned=1, cigar=_runs(ops))


def whole_gaps(window, rc, query, begin, cigar, scores=DEFAULT, band=16):
    """The same by another formulation: H(i, j) is the best of the diagonal step and of WHOLE gaps of every length k that end
    in (i, j) -- k rows up or k columns to the left, every cell the gap passes inside the band --, memoised; no Ins or Del
    matrix.  The traceback takes the diagonal first, then the shortest vertical gap that attains H, then the shortest
    horizontal one."""
    a, b, o, e = scores
    m, n = len(query), len(window)
    rows, longest = _band(begin, cigar, m, n, band)
    assert cigar and longest <= 63 - 2 * band
    t, qr = _frame(window, rc, query)
    inside = lambda i, j: 0 <= i <= m and rows[i][0] <= j <= rows[i][1]

    def options(i, j):
        """(value, kind, length) of every way into H(i, j), in tie order."""
        out = []
        if inside(i - 1, j - 1) and h(i - 1, j - 1) is not None:
            out.append((h(i - 1, j - 1) + (a if qr[i - 1] == t[j - 1] else -b), M, 1))
        for kind, di, dj in ((I, 1, 0), (D, 0, 1)):
            k = 1
            while inside(i - k * di, j - k * dj):
                v = h(i - k * di, j - k * dj)
                if v is not None:
                    out.append((v - o - k * e, kind, k))
                k += 1
        return out

    @lru_cache(maxsize=None)
    def h(i, j):
        if i == 0:
            return 0
        vals = options(i, j)
        return max(v for v, _, _ in vals) if vals else None

    last = [(j, h(m, j)) for j in range(rows[m][0], rows[m][1] + 1) if h(m, j) is not None]
    score = max(v for _, v in last)
    j = max(j for j, v in last if v == score)
    i, ops = m, []
    while i > 0:
        _, kind, k = next(x for x in options(i, j) if x[0] == h(i, j))
        ops += [kind] * k
        i, j = (i - k, j - k * (kind == M)) if kind != D else (i, j - k)
    return dict(score=score, begin=j, realigned=1, cigar=_runs(ops))


# ------------------------------------------------------------------------------------------------ hand-worked cases

LEFT, GONE, RIGHT = b"ACGTTGCAAGCTTACG", b"GGATCC", b"TTCAGACCTGATAGCA"


def test_a_scattered_deletion_is_merged():
    """Six deleted bases that the edit path spread over four gaps (unit costs: as good as one) come back as one 6D:
    32 matches - (6 + 6) = 20, against -7 - 7 - 8 - 8 + matches for the scattered path."""
    window, query = LEFT + GONE + RIGHT, LEFT + RIGHT
    given = [(M, 14), (D, 1), (M, 2), (D, 1), (M, 1), (D, 2), (M, 2), (D, 2), (M, 13)]
    for f in (restate_realign, whole_gaps):
        got = f(window, 0, query, 0, given)
        assert got == dict(score=20, begin=0, realigned=1, cigar=[(M, 16), (D, 6), (M, 16)]), f.__name__
    assert path_score(window, 0, query, 0, given) < 20


def test_gaps_in_a_homopolymer_go_to_the_start_of_the_text_as_the_aligner_saw_it():
    """One A of five deleted: every placement scores the same, the traceback (diagonal first, from the end) leaves the gap at
    the run's first base -- in the aligner's frame on either strand, so on the forward strand a reverse-strand alignment has
    it at the run's other end.  The same for an inserted A."""
    text, query = b"CGTCAAAAAGTCGTC", b"CGTCAAAAGTCGTC"
    for f in (restate_realign, whole_gaps):
        for given in ([(M, 8), (D, 1), (M, 6)], [(M, 4), (D, 1), (M, 10)], [(M, 6), (D, 1), (M, 8)]):
            want = dict(score=14 - 7, begin=0, realigned=1, cigar=[(M, 4), (D, 1), (M, 10)])
            assert f(text, 0, query, 0, given) == want
            assert f(text.translate(COMP)[::-1], 1, query, 0, given) == want
        more = b"CGTCAAAAAAGTCGTC"
        want = dict(score=15 - 7, begin=0, realigned=1, cigar=[(M, 4), (I, 1), (M, 11)])
        assert f(text, 0, more, 0, [(M, 9), (I, 1), (M, 6)]) == want
        assert f(text.translate(COMP)[::-1], 1, more, 0, [(M, 9), (I, 1), (M, 6)]) == want


def test_an_insertion_at_column_0_and_a_band_cut_at_both_ends_of_the_text():
    """The window is exactly the ten bases the read's tail matches: the band of 16 columns is cut to [0, 10] in every row, the
    two leading bases can only be inserted."""
    window, query = b"ACGTACGGTC", b"GGACGTACGGTC"
    for f in (restate_realign, whole_gaps):
        got = f(window, 0, query, 0, [(I, 2), (M, 10)])
        assert got == dict(score=10 - 8, begin=0, realigned=1, cigar=[(I, 2), (M, 10)])
        got = f(window, 0, query + b"TT", 0, [(I, 2), (M, 10), (I, 2)], band=1)
        assert got == dict(score=10 - 16, begin=0, realigned=1, cigar=[(I, 2), (M, 10), (I, 2)])
    # begin moves when the given path started a column late: band 3 reaches back to column 0
    assert restate_realign(b"TT" + window, 0, window, 3, [(I, 1), (M, 9)], band=3)["begin"] == 2


@pytest.mark.parametrize("band", [1, 8, 16, 31])
def test_the_longest_deletion_a_band_holds(band):
    """A D entry of 63 - 2w bases is realigned (and stays: 20 matches either side outweigh it), one of 64 - 2w is passed
    through with the given path's score."""
    rng = np.random.default_rng(band)
    left, right = bytes(rng.choice(list(b"ACGT"), 20).astype(np.uint8)), bytes(rng.choice(list(b"ACGT"), 20).astype(np.uint8))
    for length, realigned in ((63 - 2 * band, 1), (64 - 2 * band, 0)):
        gone = bytes(rng.choice(list(b"ACGT"), length).astype(np.uint8))
        given = [(M, 20), (D, length), (M, 20)]
        got = restate_realign(b"T" + left + gone + right + b"A", 0, left + right, 1, given, band=band)
        assert got["realigned"] == realigned and got["score"] >= 40 - 6 - length
        if realigned:
            assert got == whole_gaps(b"T" + left + gone + right + b"A", 0, left + right, 1, given, band=band)
            assert sum(n for op, n in got["cigar"] if op != D) == 40
        else:
            assert got == dict(score=40 - 6 - length, begin=1, realigned=0, cigar=given)


def test_an_empty_cigar():
    assert restate_realign(b"ACGT", 0, b"ACG", 2, []) == dict(score=0, begin=2, realigned=0, cigar=[])
    assert restate_realign(b"ACGT", 1, b"", 0, []) == dict(score=0, begin=0, realigned=0, cigar=[])


def random_case(rng, max_m=40, letters=b"AC"):
    """A valid alignment with a random, deliberately poor path over a small alphabet (many ties)."""
    cigar, last = [], None
    for _ in range(int(rng.integers(1, 7))):
        op = int(rng.choice([o for o in (M, I, D) if o != last]))
        cigar.append((op, int(rng.integers(1, 12 if op == M else 5))))
        last = op
    if sum(n for op, n in cigar if op != D) > max_m:
        return random_case(rng, max_m, letters)
    begin = int(rng.integers(0, 4))
    window = bytes(rng.choice(list(letters), begin + sum(n for op, n in cigar if op != I) + int(rng.integers(0, 4))).astype(np.uint8))
    query = bytes(rng.choice(list(letters), sum(n for op, n in cigar if op != D)).astype(np.uint8))
    return window, int(rng.integers(0, 2)), query, begin, cigar


def test_the_two_formulations_agree():
    """A few hundred random alignments of up to 40 query bases over a two-letter alphabet, where ties abound, under several
    scores and bands: score, begin and CIGAR agree, and the contract's invariants hold."""
    rng = np.random.default_rng(71)
    moved = 0
    for _ in range(300):
        window, rc, query, begin, cigar = random_case(rng)
        for scores, band in ((DEFAULT, 16), ((1, 1, 1, 1), 2), ((2, 3, 5, 2), 1), ((1024, 1, 1024, 1), 31), ((1, 1024, 1, 1024), 5)):
            got = restate_realign(window, rc, query, begin, cigar, scores, band)
            if any(op == D and n > 63 - 2 * band for op, n in cigar):        # (band 31 holds a D of one base)
                assert got == dict(score=path_score(window, rc, query, begin, cigar, scores), begin=begin, realigned=0, cigar=cigar)
                continue
            assert got["realigned"] == 1
            assert got == whole_gaps(window, rc, query, begin, cigar, scores, band), (window, rc, query, begin, cigar, scores, band)
            assert got["score"] >= path_score(window, rc, query, begin, cigar, scores)
            assert got["score"] == path_score(window, rc, query, got["begin"], got["cigar"], scores)
            ops = got["cigar"]
            assert sum(n for op, n in ops if op != D) == len(query)
            assert got["begin"] + sum(n for op, n in ops if op != I) <= len(window)
            assert all(x[0] != y[0] for x, y in zip(ops, ops[1:])) and (not ops or (ops[0][0] != D and ops[-1][0] != D))
            moved += ops != cigar
    assert moved > 500, "hardly any path changed: the comparison shows little"


# ------------------------------------------------------------------------------------------------ ABI and options

def test_header_and_binding_agree_on_the_new_symbols():
    from bucket_map_amd import verify
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmv.h")).read(), flags=re.S)
    L = verify.lib()
    for name in ("bmv_realign", "bmv_realigned", "bmv_last_realign_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
        n_args = len(re.search(rf"\b{name}\s*\((.*?)\)", text, flags=re.S).group(1).split(","))
        assert n_args == len(verify.SYMBOLS[name][1]), name
    assert callable(verify.Verifier.realign) and callable(verify.Verifier.realign_stats)


def test_entry_points_fail_cleanly_without_a_context():
    from bucket_map_amd import verify
    L = verify.lib()
    total = C.c_uint64()
    assert L.bmv_realign(None, None, 0, None, None, None, None, None, None, None, None, 0, 1, 4, 6, 1, 16, C.byref(total)) == 1
    assert b"bmv_realign" in L.bmv_last_error()
    assert L.bmv_realigned(None, None, None, None, None, None) == 1
    assert b"bmv_realigned" in L.bmv_last_error()
    assert L.bmv_last_realign_stats(None, None, None, None) == 1
    assert b"bmv_last_realign_stats" in L.bmv_last_error()


def test_options_belong_to_bucketmap_align(tmp_path):
    def run(tool, *extra):
        return subprocess.run([TOOLS[tool], "-i", "idx", *extra], cwd=str(tmp_path), capture_output=True, text=True)
    for ok in (["--affine"], ["--affine-scores", "2,3,5,2"], ["--affine-scores=1,4,6,1"], ["--affine-band", "8"],
               ["--affine", "--affine-band=31", "--clip"]):
        r = run("bucketmap_align", *ok)                          # parsed; what fails next is the missing genome
        assert r.returncode != 0 and "Unknown option" not in r.stderr and "BM_GENOME_FILE is not found" in r.stderr, r.stderr
    for refused in (["--affine"], ["--affine-scores", "1,4,6,1"], ["--affine-band=8"]):
        r = run("bucketmap", *refused)
        assert r.returncode != 0 and "belongs to bucketmap_align" in r.stderr and "BM_GENOME_FILE" not in r.stderr, r.stderr
    for bad in ("0,4,6,1", "1,4,6", "1,4,6,1,1", "1,4,6,1025", "1,,6,1", "a,b,c,d", "1"):
        r = run("bucketmap_align", "--affine-scores", bad)
        assert r.returncode != 0 and "--affine-scores" in r.stderr and "BM_GENOME_FILE" not in r.stderr, (bad, r.stderr)
    for bad in ("0", "32", "x"):
        r = run("bucketmap_align", "--affine-band", bad)
        assert r.returncode != 0 and "--affine-band" in r.stderr and "BM_GENOME_FILE" not in r.stderr, (bad, r.stderr)


# ------------------------------------------------------------------------------------------------ the oracle-backed tool

def sam_records(path):
    return [l.split("\t") for l in open(path).read().split("\n") if l and not l.startswith("@")]


def check_affine_records(recs, ref, reads, scores=DEFAULT):
    """Every record of an --affine run walked from POS over the forward FASTA with SEQ on folded letters: the =/X/I/D CIGAR
    holds, NM and MD are its own, and AS:i is the affine score recomputed from CIGAR and MD."""
    a, b, o, e = scores
    fold = lambda s: "".join("ACGT"[rank(ord(c))] for c in s)
    for f in recs:
        qname, flag, rname, pos, cigar, seq = f[0], int(f[1]), f[2], int(f[3]), f[5], f[9]
        tags = dict(t.split(":", 2)[::2] for t in f[11:])
        assert {"NM", "MD", "AS"} <= set(tags), f
        chrom, ti, qi = ref[rname], pos - 1, 0
        ops = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cigar)]
        assert "".join(f"{n}{op}" for n, op in ops) == cigar and ops, f"{qname}: CIGAR {cigar}"
        assert all(x[1] != y[1] for x, y in zip(ops, ops[1:])) and ops[0][1] != "D" and ops[-1][1] != "D", f"{qname}: {cigar}"
        nm, md, run, score = 0, "", 0, 0
        for n, op in ops:
            if op == "I":
                qi, nm, score = qi + n, nm + n, score - o - n * e
                continue
            assert ti + n <= len(chrom), f"{qname}: the CIGAR leaves {rname}"
            t = fold(chrom[ti: ti + n])
            if op == "D":
                md, run, nm, score = md + f"{run}^{t}", 0, nm + n, score - o - n * e
            else:
                same = [x == y for x, y in zip(t, seq[qi: qi + n])]
                assert len(same) == n and (all(same) if op == "=" else not any(same)), f"{qname}: {n}{op} at {ti} does not hold"
                if op == "=":
                    run, score = run + n, score + n * a
                else:
                    for c in t:
                        md, run = md + f"{run}{c}", 0
                    nm, score = nm + n, score - n * b
                qi += n
            ti += n
        md += str(run)
        assert qi == len(seq), f"{qname}: the CIGAR consumes {qi} of {len(seq)} bases"
        assert int(tags["NM"]) == nm and tags["MD"] == md, (qname, tags, nm, md)
        mismatches = len(re.findall(r"[ACGT]", re.sub(r"\^[ACGT]+", "", tags["MD"])))
        assert int(tags["AS"]) == score == a * sum(n for n, op in ops if op == "=") - b * mismatches - sum(
            o + n * e for n, op in ops if op in "ID"), (qname, tags, score)
        r_seq = reads[qname][0]
        assert seq == (fold(r_seq).translate(str.maketrans("ACGT", "TGCA"))[::-1] if flag & 16 else fold(r_seq)), qname


@pytest.fixture(scope="module")
def indel_job(tmp_path_factory):
    """A 40-kbp record; 120 reads of 150 bases with 2 % substitutions, every third one with a 5-base deletion and every
    fourth one with a 3-base insertion, every other one reverse-complemented."""
    d = tmp_path_factory.mktemp("affine")
    rng = np.random.default_rng(81)
    bases = np.frombuffer(b"ACGT", np.uint8)
    g = bases[rng.integers(0, 4, 40_000)]
    with open(d / "g.fa", "w") as f:
        f.write(f">chrA\n{bytes(g).decode()}\n")
    with open(d / "reads.fastq", "w") as f:
        for i in range(120):
            p = int(rng.integers(0, 40_000 - 170))
            s = g[p: p + 160].copy()
            hit = rng.random(len(s)) < 0.02
            s[hit] = bases[rng.integers(0, 4, int(hit.sum()))]
            if i % 3 == 0:
                s = np.concatenate([s[:70], s[75:]])
            if i % 4 == 0:
                s = np.concatenate([s[:40], bases[rng.integers(0, 4, 3)], s[40:]])
            s = bytes(s[:150])
            if i % 2:
                s = s.translate(COMP)[::-1]
            f.write(f"@r{i}\n{s.decode()}\n+\n{'I' * 150}\n")
    return d


ARGS = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "4096", "-r", "150", "-f", "1", "-q", "reads.fastq"]


def _tool(d, out, *extra):
    env = dict(os.environ, BM_VERIFY_BLOCK_READS="37")
    r = subprocess.run([TOOLS["bucketmap_align"], *ARGS, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_the_oracle_backed_tool_with_affine(indel_job):
    """--affine through alignment_verifier::realign's default: the records of the --annotate run, in the same order with the
    same MAPQ and flags; POS, CIGAR, NM and MD true against the FASTA; AS:i recomputed; indels merged.  Without the option the
    tool writes what it wrote, byte for byte, run after run."""
    from test_annotate_gpu import _fasta, _fastq
    d = indel_job
    _tool(d, "plain.sam")
    _tool(d, "ann.sam", "--annotate")
    _tool(d, "ann_again.sam", "--annotate")
    _tool(d, "aff.sam", "--affine")
    _tool(d, "aff_scores.sam", "--affine-scores", "2,3,5,2", "--affine-band", "8")
    assert (d / "ann.sam").read_bytes() == (d / "ann_again.sam").read_bytes()
    plain, ann, aff = sam_records(d / "plain.sam"), sam_records(d / "ann.sam"), sam_records(d / "aff.sam")
    assert all(len(f) == 11 for f in plain) and all(len(f) == 13 for f in ann) and all(len(f) == 14 for f in aff)
    assert not any(t.startswith("AS:") for f in ann for t in f[11:])
    key = lambda f: (f[0], f[1], f[2], f[4], f[9], f[10])
    assert [key(f) for f in ann] == [key(f) for f in aff] and len(aff) > 60
    ref, reads = _fasta(d / "g.fa"), _fastq(d / "reads.fastq")
    check_affine_records(aff, ref, reads)
    check_affine_records(sam_records(d / "aff_scores.sam"), ref, reads, (2, 3, 5, 2))
    gaps = lambda f: len(re.findall(r"[ID]", f[5]))
    assert sum(gaps(f) for f in aff) <= sum(gaps(f) for f in ann) and any("5D" in f[5] for f in aff) and any("3I" in f[5] for f in aff)
    assert any(x[5] != y[5] for x, y in zip(ann, aff)), "no CIGAR changed: the run shows little"


def test_the_oracle_backed_tool_with_pairs_and_rescue(tmp_path):
    """--affine under --rescue (which implies --paired and --best): the picks and the rescued mates are realigned -- the same
    records with the same flags, MAPQ, X0 and XR as without it, every one with AS:i, mates' PNEXT still mutual."""
    from test_pair import ARGS as PAIR_ARGS
    from test_rescue import N_LOST, make_rescue_fixture
    make_rescue_fixture(tmp_path)
    env = dict(os.environ, BM_VERIFY_BLOCK_READS="6")
    for out, extra in (("plain.sam", []), ("affine.sam", ["--affine"])):
        r = subprocess.run([TOOLS["bucketmap_align"], *PAIR_ARGS, "-q", "lost.fastq", "-o", out, "--rescue", *extra], cwd=str(tmp_path),
                           capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
    plain, aff = sam_records(tmp_path / "plain.sam"), sam_records(tmp_path / "affine.sam")
    rest = lambda f: [t for t in f[11:] if t[:2] in ("X0", "XR")]
    assert [(f[0], f[1], f[2], f[4], rest(f)) for f in plain] == [(f[0], f[1], f[2], f[4], rest(f)) for f in aff] and aff
    assert all(sum(t.startswith("AS:i:") for t in f[11:]) == 1 for f in aff) and not any("AS:i:" in "\t".join(f) for f in plain)
    assert sum("XR:i:1" in f for f in aff) >= N_LOST
    by_name = {}
    for f in aff:
        by_name.setdefault(f[0], []).append(f)
    both = [v for v in by_name.values() if len(v) == 2 and all(int(f[1]) & 8 == 0 for f in v)]
    assert both and all(x[7] == y[3] and y[7] == x[3] and int(x[8]) == -int(y[8]) for x, y in both), "PNEXT / TLEN do not follow the records"
