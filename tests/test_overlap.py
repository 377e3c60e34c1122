"""The overlap pass without a GPU: overlap_rule.overlap -- the plain-Python restatement of bmv_overlap's rule (include/bmv.h)
that tests/test_overlap_gpu.py compares the device with -- pinned on hand-worked cases; its two identities against
test_clip.restate_clip and test_annotate.restate; host/overlap_clip.h, fed random pairs by tests/cpp/overlap_check.cpp under
AddressSanitizer and UBSan, against the same rule; the ABI surface; and the tools' --clip-overlap option."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_rule
from overlap_rule import NO_MATE
from test_annotate import D, EQ, I, M, X, restate
from test_clip import CASES, S, restate_clip

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = {
    "bucketmap": os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle"),
    "bucketmap_align": os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle"),
}
COMP = bytes.maketrans(b"ACGT", b"TGCA")

#     0         10        20        30        40        50
G = b"ACGTACGGTCATGCCTAAGTCGATTGCAGCTAGGATCCATGCAAGTCTGAGCTTACGGAT"


def fwd(lo, hi):
    """G[lo, hi) read along the forward strand, without edits: (window, rc, query, begin, cigar, text_start)."""
    return G[lo:hi], 0, G[lo:hi], 0, [(M, hi - lo)], lo


def rev(lo, hi):
    """The same stretch sequenced from the other strand: the forward-strand record is the same."""
    return G[lo:hi], 1, G[lo:hi].translate(COMP)[::-1], 0, [(M, hi - lo)], lo


def rec(score, left, kept, right, pos, cut, nm=0, ref_len=None, ref_bases=b"", md=None):
    """A record: S left, the kept entries, S right."""
    if isinstance(kept, int):
        kept = [(EQ, kept)] if kept else []
    xc = ([(S, left)] if left else []) + kept + ([(S, right)] if right else [])
    span = sum(n for op, n in kept if op != I)
    return dict(score=score, clip_left=left, clip_right=right, pos=pos, ref_len=span if ref_len is None else ref_len, nm=nm,
                xcigar=xc, ref_bases=ref_bases, md=str(span) if md is None else md, cut=cut)


DEL = (G[0:16], 0, G[0:6] + G[10:16], 0, [(M, 6), (D, 4), (M, 6)], 0)      # 6= 4D 6=: g = 0..5, 6..9 under the D, 10..15
INS = (G[0:16], 0, G[0:8] + b"TTT" + G[8:16], 0, [(M, 8), (I, 3), (M, 8)], 0)      # 8= 3I 8=: the I columns carry g = 8
INS2 = (G[4:20], 0, G[4:12] + b"AAA" + G[12:20], 0, [(M, 8), (I, 3), (M, 8)], 4)   # the same from 4 on: the I columns carry g = 12
NOCOL = (G[0:9], 0, b"TTT" + G[5:9], 0, [(I, 3), (D, 5), (M, 4)], 0)       # 3I 5D 4=: its M columns carry g = 5..8
BAD = (G[0:10], 0, b"CATGCATTAG", 0, [(M, 10)], 0)                         # ten X columns: an empty range under scores

# name, alignments, contig, (match, penalty) -> records, pairs cut: worked by hand
HAND = [
    # G1(first) = 10, G0(second) = 9: m = 9 + 0; the first loses its last column, the second nothing
    ("o = 1", [fwd(0, 10), fwd(9, 20)], None, (1, 2), [rec(9, 0, 9, 1, 0, 1), rec(11, 0, 11, 0, 0, 0)], 1),
    ("o = 2", [fwd(0, 10), fwd(8, 20)], None, (1, 2), [rec(9, 0, 9, 1, 0, 1), rec(11, 1, 11, 0, 1, 1)], 1),
    # o = 5: m = 5 + 2 = 7
    ("odd o", [fwd(0, 10), fwd(5, 20)], None, (1, 2), [rec(7, 0, 7, 3, 0, 3), rec(13, 2, 13, 0, 2, 2)], 1),
    ("odd o, without scores", [fwd(0, 10), fwd(5, 20)], None, (0, 0), [rec(0, 0, 7, 3, 0, 3), rec(0, 2, 13, 0, 2, 2)], 1),
    ("odd o, the second first in the batch", [fwd(5, 20), fwd(0, 10)], None, (1, 2), [rec(13, 2, 13, 0, 2, 2), rec(7, 0, 7, 3, 0, 3)], 1),
    ("odd o, strands - +", [rev(0, 10), fwd(5, 20)], None, (1, 2), [rec(7, 0, 7, 3, 0, 3), rec(13, 2, 13, 0, 2, 2)], 1),
    ("odd o, strands + -", [fwd(0, 10), rev(5, 20)], None, (1, 2), [rec(7, 0, 7, 3, 0, 3), rec(13, 2, 13, 0, 2, 2)], 1),
    ("odd o, strands - -", [rev(0, 10), rev(5, 20)], None, (3, 1), [rec(21, 0, 7, 3, 0, 3), rec(39, 2, 13, 0, 2, 2)], 1),
    # both begin at 0: the index makes [0, 10) the first, o = 10, m = 5
    ("equal G0: the lower index is the first", [fwd(0, 10), fwd(0, 15)], None, (1, 2), [rec(5, 0, 5, 5, 0, 5), rec(10, 5, 10, 0, 5, 5)], 1),
    # ... and in the other order [0, 15) is the first and ends behind the second: containment
    ("equal G0: the other order is a containment", [fwd(0, 15), fwd(0, 10)], None, (1, 2), [rec(15, 0, 15, 0, 0, 0), rec(10, 0, 10, 0, 0, 0)], 0),
    ("containment", [fwd(0, 20), fwd(5, 15)], None, (1, 2), [rec(20, 0, 20, 0, 0, 0), rec(10, 0, 10, 0, 0, 0)], 0),
    ("adjacent", [fwd(0, 10), fwd(10, 20)], None, (1, 2), [rec(10, 0, 10, 0, 0, 0), rec(10, 0, 10, 0, 0, 0)], 0),
    ("another contig", [fwd(0, 10), fwd(5, 20)], [0, 1], (1, 2), [rec(10, 0, 10, 0, 0, 0), rec(15, 0, 15, 0, 0, 0)], 0),
    ("the same contig, named", [fwd(0, 10), fwd(5, 20)], [7, 7], (1, 2), [rec(7, 0, 7, 3, 0, 3), rec(13, 2, 13, 0, 2, 2)], 1),
    ("an empty base range", [BAD, fwd(5, 20)], None, (1, 2), [rec(0, 0, 0, 10, 0, 0, md="0"), rec(15, 0, 15, 0, 0, 0)], 0),
    # the second spans [2, 24): o = 14, m = 9, under the D.  The first keeps up to its last M column below 9 (g = 5), the
    # second from its column with g = 9: the positions 6, 7 and 8 lie under neither
    ("the cut inside a D entry", [DEL, fwd(2, 24)], None, (0, 0), [rec(0, 0, 6, 6, 0, 6), rec(0, 7, 15, 0, 7, 7)], 1),
    ("the cut inside a D entry, scores that keep it", [DEL, fwd(2, 24)], None, (2, 1), [rec(12, 0, 6, 6, 0, 6), rec(30, 7, 15, 0, 7, 7)], 1),
    # the second spans [4, 24): o = 12, m = 10, the first M column behind the D: the D goes with the clip
    ("the cut directly behind a D entry", [DEL, fwd(4, 24)], None, (0, 0), [rec(0, 0, 6, 6, 0, 6), rec(0, 6, 14, 0, 6, 6)], 1),
    # the second spans [6, 24): o = 10, m = 11: one column behind the D stays, and the D with it
    ("the cut one column behind a D entry", [DEL, fwd(6, 24)], None, (0, 0),
     [rec(0, 0, [(EQ, 6), (D, 4), (EQ, 1)], 5, 0, 5, nm=4, ref_bases=b"GGTC", md="6^GGTC1"), rec(0, 5, 13, 0, 5, 5)], 1),
    # the second spans [1, 24): o = 15, m = 8, the g of the first's I columns: they are clipped with what follows
    ("the cut at an I entry of the first", [INS, fwd(1, 24)], None, (0, 0), [rec(0, 0, 8, 11, 0, 11), rec(0, 7, 16, 0, 7, 7)], 1),
    # first [0, 20), second 8= 3I 8= from 4 on: o = 16, m = 12, the g of the second's I columns: clipped with what precedes
    ("the cut at an I entry of the second", [fwd(0, 20), INS2], None, (0, 0), [rec(0, 0, 12, 8, 0, 8), rec(0, 11, 8, 0, 8, 11)], 1),
    # the second spans [1, 12): o = 8, m = 5; no M column of the first lies below 5: neither mate changes
    ("a column that does not exist", [NOCOL, fwd(1, 12)], None, (0, 0),
     [rec(0, 0, [(I, 3), (D, 5), (EQ, 4)], 0, 0, 0, nm=8, ref_bases=b"ACGTA", md="0^ACGTA4"), rec(0, 0, 11, 0, 0, 0)], 0),
    ("an unpaired alignment between the mates", [fwd(0, 10), fwd(3, 12), fwd(5, 20)], None, (1, 2),
     [rec(7, 0, 7, 3, 0, 3), rec(9, 0, 9, 0, 0, 0), rec(13, 2, 13, 0, 2, 2)], 1),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_rule_on_hand_worked_cases(case):
    name, alns, contig, scores, want, pairs = case
    mate = [1, 0] if len(alns) == 2 else [2, NO_MATE, 0]
    got, info = overlap_rule.overlap(alns, mate, contig, *scores)
    assert got == want
    assert info["pairs_cut"] == pairs and info["bases_cut"] == sum(w["cut"] for w in want)
    if pairs:                                                    # no reference position under both, the outer ends where they were
        a, b = (0, len(alns) - 1) if info["role"][0] == "first" else (len(alns) - 1, 0)
        lo = lambda k: alns[k][5] + got[k]["pos"]
        assert lo(a) + got[a]["ref_len"] <= info["m"][a] <= lo(b)
        assert lo(a) == info["G0"][a] and lo(b) + got[b]["ref_len"] == info["G1"][b]


def test_without_mates_the_rule_is_clip_and_annotate():
    """The two identities, on test_clip's hand-worked cases and on this file's alignments."""
    singles = [(c[1], c[2], c[3], c[4], c[5], 1000) for c in CASES] + [a for c in HAND for a in c[1]]
    for match, penalty in ((1, 2), (2, 1), (1024, 1)):
        got, info = overlap_rule.overlap(singles, [NO_MATE] * len(singles), None, match, penalty)
        assert info["pairs_cut"] == info["bases_cut"] == 0
        for g, (window, rc, query, begin, cigar, _) in zip(got, singles):
            assert g == dict(restate_clip(window, rc, query, begin, cigar, match, penalty), cut=0)
    got, _ = overlap_rule.overlap(singles, [NO_MATE] * len(singles), None, 0, 0)
    for g, (window, rc, query, begin, cigar, _) in zip(got, singles):
        pos, ref_len, xc, nm, ref, md = restate(window, rc, query, begin, cigar)
        assert g == dict(score=0, clip_left=0, clip_right=0, pos=pos, ref_len=ref_len, nm=nm, xcigar=[tuple(e) for e in xc],
                         ref_bases=ref, md=md, cut=0)


def test_header_and_binding_agree_on_the_new_symbols():
    from bucket_map_amd import verify
    text = open(os.path.join(ROOT, "include", "bmv.h")).read()
    assert re.search(r"#define\s+BMV_NO_MATE\s+UINT32_MAX\b", text) and verify.NO_MATE == NO_MATE == 2 ** 32 - 1
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = verify.lib()
    for name in ("bmv_overlap", "bmv_overlapped", "bmv_last_overlap_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
        n_args = len(re.search(rf"\b{name}\s*\((.*?)\)", text, flags=re.S).group(1).split(","))
        assert n_args == len(verify.SYMBOLS[name][1]), name
    assert callable(verify.Verifier.overlap) and callable(verify.Verifier.overlap_stats)


def test_entry_points_fail_cleanly_without_a_context():
    from bucket_map_amd import verify
    L = verify.lib()
    a, b = C.c_uint64(), C.c_uint64()
    assert L.bmv_overlap(None, None, 0, None, None, None, None, None, None, None, None, None, None, 0, 1, 2, C.byref(a), C.byref(b)) == 1
    assert b"bmv_overlap" in L.bmv_last_error()
    assert L.bmv_overlapped(None, None, None, None, None, None, None, None, None, None, None, None) == 1
    assert b"bmv_overlapped" in L.bmv_last_error()
    assert L.bmv_last_overlap_stats(None, None, None, None, None) == 1
    assert b"bmv_last_overlap_stats" in L.bmv_last_error()


# ---- host/overlap_clip.h as a program of its own ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_check")
    exe = str(d / "overlap_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "overlap_check.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_check(checker, genome, alns, mate, contig, match, penalty, expect=0):
    """alns: (text_start, text_len, rc, query, begin, cigar).  Returns the program's records as the rule's dicts, and its counts."""
    d, exe = checker
    lines = [genome.decode(), f"{len(alns)} {match} {penalty} {int(contig is not None)}"]
    for a, (ts, tl, rc, query, begin, cigar) in enumerate(alns):
        lines.append(f"{ts} {tl} {rc} {begin} {mate[a]} {contig[a] if contig is not None else 0} {query.decode() or '-'} {len(cigar)} "
                     + " ".join(f"{op} {n}" for op, n in cigar))
    (d / "batch.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, "batch.txt"], cwd=str(d), capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode == expect, r.stderr[-3000:]
    if expect:
        return r.stdout
    out = r.stdout.split("\n")
    recs = []
    for line in out[: len(alns)]:
        f = line.split()
        xc = [("MIDNSHP=X".index(op), int(n)) for n, op in re.findall(r"(\d+)([=XIDS])", f[7])]
        recs.append(dict(score=int(f[0]), clip_left=int(f[1]), clip_right=int(f[2]), pos=int(f[3]), ref_len=int(f[4]), nm=int(f[5]),
                         cut=int(f[6]), xcigar=xc, ref_bases=b"" if f[8] == "-" else f[8].encode()))
    tail = out[len(alns)].split()
    return recs, int(tail[1]), int(tail[3])


def _random_pairs(rng, genome, n_pairs):
    """Pairs of short alignments with edits of every kind, placed so that about everything the rule tells apart happens:
    overlaps of every size, gaps, containments, equal starts, either strand, unpaired and empty alignments in between."""
    alns, mate, contig = [], [], []

    def one(at):
        cigar, last = [], None
        for _ in range(int(rng.integers(1, 7))):
            op = int(rng.choice([o for o in (M, I, D) if o != last]))
            cigar.append((op, int(rng.integers(1, 40 if op == M else 5))))
            last = op
        rc, begin, slack = int(rng.integers(0, 2)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
        width = begin + sum(n for op, n in cigar if op != I) + slack
        q = bytearray(rng.choice(list(b"ACGTacgtN"), sum(n for op, n in cigar if op != D)).astype(np.uint8))
        # most M columns match: copy the text under them (in the aligner's frame) into the query
        window = genome[at: at + width]
        t = window.translate(COMP)[::-1] if rc else window
        ti, qi = begin, 0
        for op, n in cigar:
            for _ in range(n):
                if op == M and rng.random() < 0.85:
                    q[qi] = t[ti]
                ti += op != I
                qi += op != D
        return at, width, rc, bytes(q), begin, cigar

    for _ in range(n_pairs):
        at = int(rng.integers(0, len(genome) - 400))
        a = len(alns)
        alns.append(one(at))
        alns.append(one(at + int(rng.integers(0, 25))))
        mate.extend([a + 1, a])
        c = int(rng.integers(0, 3))
        contig.extend([c, c if rng.random() < 0.9 else c + 1])
        if rng.random() < 0.2:
            alns.append(one(int(rng.integers(0, len(genome) - 400))))
            mate.append(NO_MATE)
            contig.append(0)
        if rng.random() < 0.05:
            alns.append((int(rng.integers(0, 100)), 20, 0, b"ACGT" if rng.random() < 0.5 else b"", 0, []))
            mate.append(NO_MATE)
            contig.append(0)
    order = rng.permutation(len(alns))
    where = np.empty(len(alns), np.int64)
    where[order] = np.arange(len(alns))
    return ([alns[k] for k in order], [NO_MATE if mate[k] == NO_MATE else int(where[mate[k]]) for k in order], [contig[k] for k in order])


@pytest.mark.parametrize("scores", [(0, 0), (1, 2), (1024, 1), (2, 3)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_host_restatement_against_the_rule(checker, scores):
    """1 500 random pairs through host/overlap_clip.h under the sanitizers: every number is the Python rule's."""
    rng = np.random.default_rng(81 + scores[0])
    genome = bytes(rng.choice(list(b"ACGT"), 5000).astype(np.uint8))
    alns, mate, contig = _random_pairs(rng, genome, 1500)
    use_contig = contig if scores != (2, 3) else None
    got, pairs, bases = run_check(checker, genome, alns, mate, use_contig, *scores)
    want, info = overlap_rule.overlap([(genome[ts: ts + tl], rc, q, begin, cigar, ts) for ts, tl, rc, q, begin, cigar in alns], mate,
                                      use_contig, *scores)
    assert 300 < info["pairs_cut"] < 1400, "the random pairs show little"
    for a, (g, w) in enumerate(zip(got, want)):
        assert g == {k: w[k] for k in g}, (a, alns[a], info["role"][a], info["m"][a])
    assert (pairs, bases) == (info["pairs_cut"], info["bases_cut"])


def test_host_restatement_on_the_hand_worked_cases_and_its_refusals(checker):
    for name, alns, contig, scores, want, pairs in HAND:
        mate = [1, 0] if len(alns) == 2 else [2, NO_MATE, 0]
        got, p, b = run_check(checker, G, [(ts, len(w), rc, q, begin, cigar) for w, rc, q, begin, cigar, ts in alns], mate, contig, *scores)
        assert got == [{k: x[k] for k in x if k != "md"} for x in want] and p == pairs, name
    two = [(0, 10, 0, G[0:10], 0, [(M, 10)]), (5, 15, 0, G[5:20], 0, [(M, 15)])]
    for mate, scores in (([1, 1], (1, 2)), ([0, 1], (1, 2)), ([2, 0], (1, 2)), ([1, 0], (0, 1)), ([1, 0], (1025, 1))):
        assert run_check(checker, G, two, mate, None, *scores, expect=3).startswith("refused")


# ---- the tools' option ----
def test_the_option_implies_paired_and_leaves_the_others_alone():
    """cli.h compiled with and without BM_ALIGN into a program that prints what the parser set."""
    src = r'''
#include "cli.h"
#include <cstdio>
int main(int argc, char **argv) {
    try {
        const bm::cmd_arguments a = bm::parse_arguments(argc, argv);
        std::printf("%d %d %d %d %d %d %d %d %d %u %u\n", a.clip_overlap, a.paired, a.best, a.annotate, a.clip, a.rescue, a.affine,
                    a.left_align, a.sort, a.frag_min, a.frag_max);
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
        assert out("-DBM_ALIGN") == "0 0 0 0 0 0 0 0 0 1 1000"
        assert out("-DBM_ALIGN", "--paired") == "0 1 1 1 0 0 0 0 0 1 1000"                  # the other options are what they were
        assert out("-DBM_ALIGN", "--clip", "--rescue") == "0 1 1 1 1 1 0 0 0 1 1000"
        assert out("-DBM_ALIGN", "--clip-overlap") == "1 1 1 1 0 0 0 0 0 1 1000"            # implies --paired, and what that implies
        assert out("-DBM_ALIGN", "--clip-overlap", "--paired", "--frag-range", "50,400") == "1 1 1 1 0 0 0 0 0 50 400"
        assert out("-DBM_ALIGN", "--clip-overlap", "--clip", "--rescue", "--affine", "--left-align", "-o", "x.bam", "--markdup",
                   "--depth", "x.bedgraph", "--pileup", "x.tsv", "--vcf", "x.vcf", "--vcf-indels") == "1 1 1 1 1 1 1 1 1 1 1000"
        assert out("-DBM_ALIGN", "--clip-overlap", "--frag-auto", "--best-margin", "0.1", "--max-edit-rate", "0.2") == "1 1 1 1 0 0 0 0 0 1 1000"
        for args in (["--split", "--clip-overlap"], ["--clip-overlap", "--split-max", "3"]):
            text = out("-DBM_ALIGN", *args)
            assert text.startswith("error") and "--split cannot be combined with --clip-overlap" in text, text
        text = out("-DBM_PLAIN", "--clip-overlap")
        assert text.startswith("error") and "--clip-overlap" in text and "belongs to bucketmap_align" in text, text


def test_both_tools_parse_or_refuse_the_option(tmp_path):
    def run(tool, *extra):
        return subprocess.run([TOOLS[tool], "-i", "idx", *extra], cwd=str(tmp_path), capture_output=True, text=True)
    r = run("bucketmap_align", "--clip-overlap")                 # parsed; what fails next is the missing genome
    assert r.returncode != 0 and "Unknown option" not in r.stderr and "BM_GENOME_FILE is not found" in r.stderr, r.stderr
    r = run("bucketmap_align", "--clip-overlap", "--split")
    assert r.returncode != 0 and "--split cannot be combined with --clip-overlap" in r.stderr and "BM_GENOME_FILE" not in r.stderr
    r = run("bucketmap", "--clip-overlap")
    assert r.returncode != 0 and "--clip-overlap" in r.stderr and "belongs to bucketmap_align" in r.stderr and "BM_GENOME_FILE" not in r.stderr
    r = run("bucketmap_align", "--clip-overla")
    assert r.returncode != 0 and "Unknown option --clip-overla" in r.stderr


def test_the_oracle_backed_tool_clips_on_the_host(tmp_path):
    """The whole tool without a GPU: the locator's default clip_overlap is host/overlap_clip.h.  300 simulated pairs on short
    fragments in several verifier blocks, written without and with the option: the rule applied to the records without gives the
    records with, and the blocks' counts add up in the one stderr line."""
    from test_overlap_cli_gpu import ARGS, _check_derivation, _records, _simulate
    _simulate(tmp_path, 99, 300, 120, 180, "r.fastq")
    exe = TOOLS["bucketmap_align"]
    for out, extra in (("a.sam", []), ("b.sam", ["--clip-overlap"])):
        r = subprocess.run([exe, *ARGS, "-q", "r.fastq", "-o", out, "--paired", *extra], cwd=str(tmp_path), capture_output=True, text=True,
                           env=dict(os.environ, BM_VERIFY_BLOCK_READS="64"))
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("Overlap:" in r.stderr) == bool(extra)
    told = re.search(r"Overlap: (\d+) of (\d+) pairs cut, (\d+) bases clipped", r.stderr)
    _check_derivation(_records((tmp_path / "a.sam").read_text()), _records((tmp_path / "b.sam").read_text()), r.stderr, 300, (0, 0), False)
    assert told and int(told.group(1)) > 150
