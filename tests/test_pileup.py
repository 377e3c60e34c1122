"""Pileup (-o x.bam --pileup FILE) without a GPU: the rule on cases worked out by hand, host/pileup.h as a program of its own
under ASan + UBSan, the oracle-backed tools (whose counting is the host default of block_compressor), the command line and
the bmp_* ABI surface.

The yardstick is the rule of include/bmp.h in plain Python (tests/pileup_rule.py), applied to the records decoded from the
x.bam the tool wrote and to the FASTA file: the table is a function of those alone.
"""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pileup_rule as P
from pileup_cases import EDGE_REFS, REF_LENS, edge_bases, edge_records, many_ops_record, parse_check_output, random_records, references
from test_bamsort import offsets_of, pair_of, records_of, run_tool
from test_depth import files_by_the_rule, full_record, header_refs
from test_markdup_gpu import rec, rec_ops
from test_sam_golden import ROOT, TOOLS

PILEUP = re.compile(r"Pileup: (\d+) sites on (\d+) bases from (\d+) records \((\d+) left out, (\d+) below MAPQ\)")
HEADER = "#rname\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\tlowq\tkind\n"
A, Cc, G, T, N, DEL, INS, LOWQ = range(8)
STRICT = dict(min_mapq=20, min_bq=13, min_alt=1, min_frac_ppm=250000)


# ---- the rule itself, on cases worked out by hand ----
def test_python_restatement_of_the_rule():
    recs, bases = edge_records(), edge_bases()
    by_name = {r[36: 36 + r[12] - 1]: i for i, r in enumerate(recs)}
    only = lambda *names, **th: P.pile([recs[by_name[n]] for n in names], EDGE_REFS, bases, **{**STRICT, **th})
    at = lambda res, r, p: res.counts[r][p].tolist()
    row = lambda **kw: [kw.get(k, 0) for k in ("A", "C", "G", "T", "N", "DEL", "INS", "LOWQ")]
    nothing = lambda res: not res.sites and all(not c.any() for c in res.counts)

    # quality at min_bq and a step below, 0xFF, 0; reference A C G T at 600 .. 603, the read says C C C C
    got = only(b"bq_steps")
    assert [at(got, 0, p) for p in range(600, 604)] == [row(C=1), row(LOWQ=1), row(C=1), row(LOWQ=1)]
    assert got.sites == [(0, 600, 0, *row(C=1), 1), (0, 602, 2, *row(C=1), 1)] and got.stats[0] == [1, 0, 0, 2, 2, 2]
    assert only(b"bq_steps", min_bq=12).stats[0][3:5] == [3, 1] and only(b"bq_steps", min_bq=0).stats[0][3:5] == [4, 0]
    assert only(b"bq_steps", min_bq=256).stats[0][3:5] == [1, 3]                    # 0xFF passes whatever the threshold
    # MAPQ at min_mapq and one below
    both = only(b"mapq_at", b"mapq_below")
    assert both.stats[0][:3] == [1, 1, 0] and at(both, 0, 610) == row(G=1)
    assert only(b"mapq_at", b"mapq_below", min_mapq=19).stats[0][:3] == [2, 0, 0]
    # an odd query offset: after 3S the block starts on a low nibble; A C G T A over C G T A C (620 .. 624)
    got = only(b"odd_after_3S")
    assert [at(got, 0, 620 + k) for k in range(5)] == [row(A=1), row(C=1), row(G=1), row(T=1), row(A=1)] and at(got, 0, 619) == row()
    got = only(b"odd_after_I")                           # G T, an inserted A, then A C G T at 632 .. 635
    assert [at(got, 0, 630 + k) for k in range(6)] == [row(G=1), row(T=1, INS=1), row(A=1), row(C=1), row(G=1), row(T=1)]
    got = only(b"odd_l_seq")
    assert [at(got, 0, 640 + k) for k in range(5)] == [row(A=1), row(C=1), row(G=1), row(T=1), row(T=1)] and got.stats[0][3] == 5
    got = only(b"other_codes")                           # codes 0 3 5 15 are N, then A C
    assert [at(got, 0, 650 + k) for k in range(6)] == [row(N=1)] * 4 + [row(A=1), row(C=1)]
    # insertions: leading and straight after S dropped; after D anchored on the last deleted position; after M and N counted
    for name, first in ((b"leading_I", 660), (b"I_after_S", 664)):
        got = only(name)
        assert sum(int(c[:, INS].sum()) for c in got.counts) == 0 and got.stats[0][3] == 4 and at(got, 0, first) != row(), name
    got = only(b"I_after_D")
    assert at(got, 0, 672) == row(DEL=1) and at(got, 0, 673) == row(DEL=1, INS=1) and at(got, 0, 671)[INS] == 0
    assert (0, 673, 1, *row(DEL=1, INS=1), 6) in got.sites
    assert at(only(b"I_after_MN"), 0, 684)[INS] == 1 and int(only(b"I_after_MN").counts[0][:, INS].sum()) == 1
    assert int(only(b"I_after_N_only").counts[0][:, INS].sum()) == 0 and only(b"I_after_N_only").stats[0][3] == 2
    got = only(b"I_on_the_last_base")
    assert at(got, 1, 49)[INS] == 1 and got.stats[1][3] == 2
    got = only(b"I_off_the_end")                         # the third base lies beyond the reference, and the anchor with it
    assert int(got.counts[1][:, INS].sum()) == 0 and got.stats[1][3] == 2
    got = only(b"D_over_the_end")
    assert got.counts[1][:, DEL].tolist() == [0] * 47 + [1] * 3 and got.stats[1][3] == 2
    # reference bytes: lower case counts as its letter, N n R give no allele -- no SNV there, a DEL site all the same
    got = only(b"on_odd_reference_a", b"on_odd_reference_b", min_alt=2)
    assert [s[:3] + s[-1:] for s in got.sites] == [(0, 100, 0, 1), (0, 102, 2, 1), (0, 103, 3, 1)]   # a c g t N n R under C x 7
    got = only(b"del_on_N_a", b"del_on_N_b", min_alt=2)
    assert [s[:3] + s[-1:] for s in got.sites] == [(0, 103, 3, 2), (0, 104, 4, 2)]
    assert at(got, 0, 105) == row(A=2) and at(got, 0, 106) == row(A=2) and all(s[1] != 106 for s in got.sites)
    # the fraction at equality and one count below it: one T of four reads is 250 000 ppm, one of five is not
    four, five = [b"frac4_%d" % k for k in range(4)], [b"frac5_%d" % k for k in range(5)]
    assert only(*four).sites == [(0, 700, 0, *row(A=3, T=1), 1)] and only(*five).sites == []
    assert only(*five, min_frac_ppm=200000).sites == [(0, 704, 0, *row(A=4, T=1), 1)]
    assert only(*four, min_frac_ppm=250001).sites == []
    # min_frac_ppm 0: min_alt alone decides; 1 000 000: every spanning read has to differ
    assert only(*five, min_frac_ppm=0).sites and only(*five, min_frac_ppm=0, min_alt=2).sites == []
    assert only(*five, min_frac_ppm=1000000).sites == [] and only(four[0], min_frac_ppm=1000000).sites == [(0, 700, 0, *row(T=1), 1)]
    assert only(b"one_base_t", b"one_base_t2", b"one_base_g", min_alt=2).sites == [(2, 0, 2, *row(G=1, T=2), 1)]
    # not placed, or left out
    for name in (b"pos_is_len", b"pos_negative", b"no_reference", b"no_cigar", b"flag4", b"flag100", b"flag200", b"flag400", b"placeholder_dup"):
        got = only(name)
        assert nothing(got) and got.stats == [[0] * 6] * 3, name
    for name, r in ((b"no_sequence", 0), (b"placeholder", 1), (b"pads_only", 0)):
        got = only(name)
        assert nothing(got) and got.stats[r] == [0, 0, 1, 0, 0, 0], name
    for name in (b"clips_only", b"hard_and_soft", b"insert_only"):                   # counted records that add nothing
        got = only(name)
        assert nothing(got) and got.stats[0] == [1, 0, 0, 0, 0, 0], name
    assert only(b"no_placeholder").counts[1][:, DEL].tolist() == [0] * 7 + [1] * 43 and only(b"no_placeholder").stats[1][0] == 1
    assert only(b"flag800").stats[1][0] == 1
    # clipping: 10M one past the end counts nine bases, a block beyond the end none
    assert only(b"one_past").stats[0][3] + only(b"one_past").stats[0][4] == 9
    got = only(b"block_beyond")
    assert got.stats[0][3] + got.stats[0][4] == 3 and got.counts[0][:, DEL].tolist()[998:] == [1, 1]
    got = only(b"insert_then_clip")                      # 2M 2I 4M at 996: the anchor is 997, the last two bases lie beyond
    assert at(got, 0, 997)[INS] == 1 and got.stats[0][3] + got.stats[0][4] == 4
    got = only(b"gaps")                                  # 4M 3D 4M 2N 4M: D counts as DEL, N as nothing
    assert got.counts[0][300:317, DEL].tolist() == [0] * 4 + [1] * 3 + [0] * 10 and got.stats[0][3] + got.stats[0][4] == 12
    assert got.counts[0][311:313].sum() == 0
    # everything together
    res = P.pile(recs, EDGE_REFS, bases, **STRICT)
    kinds = [sum(1 for s in res.sites if s[11] & b) for b in (1, 2, 4)]
    assert all(kinds) and len(res.sites) < sum(EDGE_REFS) and [s[:2] for s in res.sites] == sorted(s[:2] for s in res.sites)
    assert sum(int(c[:, :5].sum()) for c in res.counts) == sum(s[3] for s in res.stats)
    assert {len(r) % 16 for r in recs} == set(range(16))
    text = P.pileup_text(only(*four), ["a", "b", "c"])
    assert text == HEADER + "a\t701\tA\t3\t0\t0\t1\t0\t0\t0\t0\tS\n"
    assert P.pileup_text(only(b"I_after_D"), "abc").split("\n")[-2] == "a\t674\tC\t0\t0\t0\t0\t0\t1\t1\t0\tDI"
    assert P.pileup_text(only(b"del_on_N_a", b"del_on_N_b"), "abc").split("\n")[2].startswith("a\t105\t.\t")
    assert P.summary_line(only(*four)) == "Pileup: 1 sites on 4 bases from 4 records (0 left out, 0 below MAPQ)"
    assert P.refused([rec_ops(0, 1, 0, [3 << 4 | 9], b"")], 3) and P.refused([rec(0, 1, 0, "3M", b"ab")], 3)


def test_random_cases_have_sites_of_every_kind_but_not_everywhere():
    """What the other tests rely on: their site lists are neither empty nor everything."""
    bases = references()
    for n in (257, 1025, 20001):
        want = P.pile(random_records(n, 300 + n, bases=bases), REF_LENS, bases)
        kinds = [sum(1 for s in want.sites if s[11] & b) for b in (1, 2, 4)]
        assert all(kinds) and len(want.sites) < sum(REF_LENS) // 10, (n, kinds)
        assert all(s[0] for s in want.stats[1:]) and sum(s[2] for s in want.stats) > 0 and sum(s[4] for s in want.stats) > 0


# ---- host/pileup.h as a program of its own ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("pileup_check")
    exe = str(d / "pileup_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "pileup_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_check(checker, recs, ref_len, bases, n_calls=1, seed=0, skip=None, expect=0, **thresholds):
    d, exe = checker
    th = {**P.DEFAULTS, **thresholds}
    (d / "records.bin").write_bytes(b"".join(recs))
    (d / "bases.bin").write_bytes(b"".join(bases))
    if skip is not None:
        (d / "skip.bin").write_bytes(bytes(skip))
    r = subprocess.run([exe, "records.bin", "skip.bin" if skip is not None else "-", "bases.bin", str(n_calls), str(seed),
                        *[str(th[k]) for k in ("min_mapq", "min_bq", "min_alt", "min_frac_ppm")], *[str(x) for x in ref_len]],
                       cwd=str(d), capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode == expect, r.stderr[-3000:]
    return r.stdout


def same_as_rule(out, want):
    sites, stats, counts = parse_check_output(out)
    assert stats == want.stats
    assert all(np.array_equal(a, b) for a, b in zip(counts, want.counts))
    assert sites == want.sites


@pytest.fixture(scope="module")
def ref_bases():
    return references()


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1025, 20001])
def test_host_rule_is_the_python_rule(checker, ref_bases, n):
    recs = random_records(n, 300 + n, bases=ref_bases)
    want = P.pile(recs, REF_LENS, ref_bases)
    one = run_check(checker, recs, REF_LENS, ref_bases)
    same_as_rule(one, want)
    if n in (2, 65, 1025):                               # order and cutting do not matter
        assert run_check(checker, recs, REF_LENS, ref_bases, n_calls=3, seed=1 + n) == one
        assert run_check(checker, recs, REF_LENS, ref_bases, n_calls=7, seed=n) == one
    if n == 1025:                                        # other thresholds
        same_as_rule(run_check(checker, recs, REF_LENS, ref_bases, **STRICT), P.pile(recs, REF_LENS, ref_bases, **STRICT))


def test_host_rule_on_the_edges_and_a_record_of_many_ops(checker):
    recs, bases = edge_records(), edge_bases()
    for th in ({}, STRICT, dict(min_frac_ppm=0, min_alt=1), dict(min_frac_ppm=1000000, min_bq=0)):
        one = run_check(checker, recs, EDGE_REFS, bases, **th)
        same_as_rule(one, P.pile(recs, EDGE_REFS, bases, **th))
        assert run_check(checker, recs, EDGE_REFS, bases, n_calls=3, seed=3, **th) == one
        assert run_check(checker, recs, EDGE_REFS, bases, n_calls=7, seed=5, **th) == one
    refs = [90000, 300]
    bases = references(refs, 4)
    recs = random_records(40, 5, refs, bases) + [many_ops_record(0, 17)] + random_records(40, 6, refs, bases)
    want = P.pile(recs, refs, bases)
    assert want.stats[0][3] > 30000 and int(want.counts[0][:, DEL].sum()) > 5000 and int(want.counts[0][:, INS].sum()) > 3000
    same_as_rule(run_check(checker, recs, refs, bases), want)


def test_host_skip_bytes_equal_removing_the_records(checker, ref_bases):
    recs = random_records(500, 77, bases=ref_bases)
    skip = [int(k % 3 == 1) for k in range(500)]
    want = P.pile(recs, REF_LENS, ref_bases, skip)
    assert want.stats != P.pile(recs, REF_LENS, ref_bases).stats
    kept = [r for r, s in zip(recs, skip) if not s]
    assert P.pile(kept, REF_LENS, ref_bases).sites == want.sites and P.pile(kept, REF_LENS, ref_bases).stats == want.stats
    same_as_rule(run_check(checker, recs, REF_LENS, ref_bases, skip=skip), want)
    assert run_check(checker, recs, REF_LENS, ref_bases, n_calls=4, seed=9, skip=skip) == run_check(checker, kept, REF_LENS, ref_bases)


def test_host_rule_refuses_what_the_abi_refuses(checker, ref_bases):
    good = random_records(10, 1, bases=ref_bases)
    for bad in (rec_ops(0, 0, 0, [3 << 4 | 9], b""), rec(1, 5, 0, "3M", b"ab"), rec(6, 5, 0, "3M", b""), rec(1, 5, 0, "3M2I", b"abcd")):
        assert P.refused([bad], len(REF_LENS))
        assert run_check(checker, good + [bad], REF_LENS, ref_bases, expect=3).startswith("refused ")
    assert "sites" in run_check(checker, good + [rec(6, 5, 4, "3M", b"")], REF_LENS, ref_bases)      # unmapped: its reference is not looked at
    assert run_check(checker, good, [5, 0, 5], [b"ACGTA", b"", b"ACGTA"], expect=3).startswith("refused ")   # a reference without bases
    assert run_check(checker, good, REF_LENS, ref_bases, expect=3, min_alt=0).startswith("refused ")
    assert run_check(checker, good, REF_LENS, ref_bases, expect=3, min_frac_ppm=1000001).startswith("refused ")
    assert "sites" in run_check(checker, good, REF_LENS, ref_bases, min_frac_ppm=1000000)


@pytest.mark.parametrize("text,ppm", [("0", 0), ("1", 1000000), ("0.2", 200000), ("0.000001", 1), ("1.0000000", None), ("1.1", None), ("-0", None),
                                      ("2e-1", None), ("0.1234567", None), ("1.000000", 1000000), ("0.999999", 999999), ("0.5", 500000),
                                      ("", None), (".5", None), ("0.", None), ("00.5", None), ("2", None), ("1.000001", None), ("+0.5", None),
                                      (" 0.5", None), ("0.5 ", None), ("0,5", None)])
def test_fraction_parser(checker, text, ppm):
    d, exe = checker
    r = subprocess.run([exe, "ppm", text], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error:" not in r.stderr and r.stdout.strip() == ("refused" if ppm is None else str(ppm))


# ---- the oracle-backed tools ----
def fasta_bases(path, refs, bucket_len, read_len):
    """The references' bases as the tools see them.  read_fasta folds every letter but A C G T (in either case) to A -- so a
    reference N reads as A.  A reference of the header is a run of kept buckets of one name, bucket_len positions each: a
    record is cut every bucket_len bases, a piece that with the read_len bases behind it is no longer than read_len is not
    kept, and records whose names agree up to the first blank share a reference.  What no sequence fills is N."""
    records = []
    for line in open(path).read().split("\n"):
        if line.startswith(">"):
            records.append([line[1:].split(" ")[0], ""])
        elif records:
            records[-1][1] += "".join(ch.upper() if ch.upper() in "ACGT" else "A" for ch in line.strip())
    out = []
    for name, seq in records:
        for start in range(0, len(seq), bucket_len):
            if min(start + bucket_len + read_len, len(seq)) - start <= read_len:
                continue
            piece = seq[start: start + bucket_len].ljust(bucket_len, "N")
            if out and out[-1][0] == name:
                out[-1][1] += piece
            else:
                out.append([name, piece])
    assert [(n, len(b)) for n, b in out] == refs
    return [b.encode() for _, b in out]


def pileup_by_the_rule(bam_path, args, **thresholds):
    """(the --pileup text, the stderr line, the rule's result) for the records of a BAM file and the FASTA file of the tool's
    arguments."""
    fasta = os.path.join(os.path.dirname(bam_path), args[args.index("--genome") + 1])
    cut = int(args[args.index("--bucket-len") + 1]), int(args[args.index("-r") + 1])
    raw = gzip.decompress(open(bam_path, "rb").read())
    refs = header_refs(raw)
    recs = [r for _, r in records_of(raw)[0]]
    res = P.pile(recs, [l for _, l in refs], fasta_bases(fasta, refs, *cut), **thresholds)
    return P.pileup_text(res, [n for n, _ in refs]), P.summary_line(res), res


def pileup_line(err):
    found = [l.split("\t")[-1] for l in err.split("\n") if "Pileup:" in l]
    assert len(found) == 1 and PILEUP.fullmatch(found[0]), err
    return found[0]


def pileup_jobs(tmp_path_factory):
    """markdup_jobs with variants put into its reads, which are exact copies of the genome and would give no site at all: by a
    read's checksum (so the copies of a read, the duplicates, agree) a substitution near base 40, a deleted base near 70, an
    inserted G near 100."""
    import zlib
    from test_markdup import markdup_jobs
    out = []
    for name, which, d, args, extra in markdup_jobs(tmp_path_factory):
        lines = (d / args[args.index("-q") + 1]).read_text().split("\n")
        with open(d / "pile.fastq", "w") as f:
            for i in range(0, len(lines) - 1, 4):
                seq, qual, h = lines[i + 1], lines[i + 3], zlib.crc32(lines[i + 1].encode())
                if h % 5 == 0 and len(seq) > 120:
                    at = 100 + h % 11
                    seq, qual = seq[:at] + "G" + seq[at:], qual[:at] + qual[at] + qual[at:]
                if h % 3 == 0 and len(seq) > 90:
                    at = 70 + h % 5
                    seq, qual = seq[:at] + seq[at + 1:], qual[:at] + qual[at + 1:]
                if h % 2 == 0 and len(seq) > 60:
                    at = 40 + h % 7
                    seq = seq[:at] + "ACGTA"["ACGT".find(seq[at]) + 1] + seq[at + 1:]
                f.write(f"{lines[i]}\n{seq}\n+\n{qual}\n")
        args = list(args)
        args[args.index("-q") + 1] = "pile.fastq"
        out.append((name, which, d, args, extra))
    return out


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    return pileup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", range(3))
def test_oracle_tool_writes_what_the_rule_says(jobs, k):
    name, which, d, args, extra = jobs[k]
    exe = TOOLS[(which, "oracle")]
    implied = ["--annotate"] if which == "bucketmap_align" else []               # what --pileup implies beside --sort
    err = run_tool(exe, d, args, f"{name}.ps.bam", [*extra, *implied, "--sort"])
    assert "Pileup:" not in err
    err = run_tool(exe, d, args, f"{name}.p.bam", [*extra, "--pileup", f"{name}.p.tsv"])
    assert re.search(r"Sorted \d+ records by coordinate in 1 run", err)
    assert pair_of(d, f"{name}.p") == pair_of(d, f"{name}.ps")                   # the BAM and its index are what they were
    text, line, res = pileup_by_the_rule(d / f"{name}.p.bam", args)
    assert (d / f"{name}.p.tsv").read_text() == text and pileup_line(err) == line
    aligned = name != "plain"                            # the plain tool writes no CIGAR: no counted record, only the header line
    if aligned:
        assert sum(s[0] for s in res.stats) > 10 and sum(s[3] for s in res.stats) > 1000
        assert 3 < len(res.sites) < sum(len(c) for c in res.counts) // 10 and all(any(s[11] & b for s in res.sites) for b in (1, 2, 4))
    else:
        assert text == HEADER and not any(any(s) for s in res.stats)
    # looser thresholds: more sites, of the same records
    loose = dict(min_bq=0, min_mapq=0, min_alt=1, min_frac_ppm=1)
    err = run_tool(exe, d, args, f"{name}.pl.bam", [*extra, "--pileup", f"{name}.pl.tsv", "--pileup-min-bq", "0", "--pileup-min-mapq=0",
                                                   "--pileup-min-alt", "1", "--pileup-min-frac", "0.000001"])
    l_text, l_line, l_res = pileup_by_the_rule(d / f"{name}.pl.bam", args, **loose)
    assert (d / f"{name}.pl.tsv").read_text() == l_text and pileup_line(err) == l_line and pair_of(d, f"{name}.pl") == pair_of(d, f"{name}.ps")
    assert not aligned or (len(l_res.sites) > len(res.sites) and len(l_res.sites) > 5)
    err = run_tool(exe, d, args, f"{name}.pq.bam", [*extra, "--pileup", f"{name}.pq.tsv", "--pileup-min-mapq", "61", "--pileup-min-bq", "41"])
    q_text, q_line, q_res = pileup_by_the_rule(d / f"{name}.pq.bam", args, min_mapq=61, min_bq=41)
    assert (d / f"{name}.pq.tsv").read_text() == q_text and pileup_line(err) == q_line
    assert not aligned or sum(s[1] for s in q_res.stats) > 0
    # several runs: the same file
    err = run_tool(exe, d, args, f"{name}.pr.bam", [*extra, "--pileup", f"{name}.pr.tsv", "--pileup-min-alt", "1", "--pileup-min-frac", "0.000001",
                                                   "--pileup-min-bq", "0"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1
    assert (d / f"{name}.pr.tsv").read_text() == l_text and pileup_line(err) == l_line and pair_of(d, f"{name}.pr") == pair_of(d, f"{name}.ps")
    # with --markdup the duplicates are left out: the rule on the marked records
    run_tool(exe, d, args, f"{name}.pm0.bam", [*extra, *implied, "--markdup"])
    loose_opts = ["--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--pileup-min-bq", "0"]
    err = run_tool(exe, d, args, f"{name}.pm.bam", [*extra, "--markdup", "--pileup", f"{name}.pm.tsv", *loose_opts])
    assert pair_of(d, f"{name}.pm") == pair_of(d, f"{name}.pm0")
    m_text, m_line, m_res = pileup_by_the_rule(d / f"{name}.pm.bam", args, **loose)
    assert (d / f"{name}.pm.tsv").read_text() == m_text and pileup_line(err) == m_line
    assert not aligned or (m_text != l_text and sum(s[0] for s in m_res.stats) < sum(s[0] for s in l_res.stats))
    err = run_tool(exe, d, args, f"{name}.pmr.bam", [*extra, "--markdup", "--pileup", f"{name}.pmr.tsv", *loose_opts], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1
    assert (d / f"{name}.pmr.tsv").read_text() == m_text and pair_of(d, f"{name}.pmr") == pair_of(d, f"{name}.pm0")
    # together with --depth and --coverage: their files are what they are without --pileup
    run_tool(exe, d, args, f"{name}.pd0.bam", [*extra, *implied, "--depth", f"{name}.pd0.bedgraph", "--coverage", f"{name}.pd0.cov"])
    err = run_tool(exe, d, args, f"{name}.pd.bam", [*extra, "--depth", f"{name}.pd.bedgraph", "--coverage", f"{name}.pd.cov", "--pileup", f"{name}.pd.tsv"])
    assert "Coverage:" in err and pileup_line(err) == line and (d / f"{name}.pd.tsv").read_text() == text
    for ext in ("bedgraph", "cov"):
        assert (d / f"{name}.pd.{ext}").read_text() == (d / f"{name}.pd0.{ext}").read_text()
    depth, cov, _ = files_by_the_rule(d / f"{name}.pd.bam")
    assert (d / f"{name}.pd.bedgraph").read_text() == depth and (d / f"{name}.pd.cov").read_text() == cov
    assert pair_of(d, f"{name}.pd") == pair_of(d, f"{name}.ps") == pair_of(d, f"{name}.pd0")
    err = run_tool(exe, d, args, f"{name}.pdr.bam", [*extra, "--depth", f"{name}.pdr.bedgraph", "--pileup", f"{name}.pdr.tsv"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert (d / f"{name}.pdr.tsv").read_text() == text and (d / f"{name}.pdr.bedgraph").read_text() == depth


# ---- the command line ----
def test_cli_refusals(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        run = lambda *opts: subprocess.run([exe, "-i", "idx", *opts], cwd=str(tmp_path), capture_output=True, text=True)
        r = run("--pileup", "p.tsv", "-o", "x.sam")
        assert r.returncode != 0 and "x.bam" in r.stderr and "--pileup" in r.stderr and not os.listdir(tmp_path), r.stderr
        assert "only BAM output is sorted and indexed" in r.stderr
        r = run("--pileup", "p.tsv")
        assert r.returncode != 0 and "-o x.bam" in r.stderr and "--pileup" in r.stderr and not os.listdir(tmp_path), r.stderr
        r = run("--pileup")
        assert r.returncode != 0 and "Missing value" in r.stderr
        r = run("-o", "x.bam", "--pileup", "p.tsv")
        assert "Validation failed" not in r.stderr and "Unknown option" not in r.stderr and "Value parse failed" not in r.stderr
        for opt, value in (("--pileup-min-bq", "20"), ("--pileup-min-mapq", "20"), ("--pileup-min-alt", "3"), ("--pileup-min-frac", "0.5")):
            r = run("-o", "x.bam", opt, value)                                    # a threshold without --pileup
            assert r.returncode != 0 and opt in r.stderr and "--pileup FILE" in r.stderr and "Validation failed" in r.stderr, r.stderr
            r = run("-o", "x.bam", opt, value, "--pileup", "p.tsv")
            assert "Validation failed" not in r.stderr and "Value parse failed" not in r.stderr and "Unknown option" not in r.stderr
            r = run("-o", "x.bam", "--pileup", "p.tsv", opt)
            assert r.returncode != 0 and "Missing value" in r.stderr
            for bad in ("x", "-1", "", "1.5x", "4294967296" if "frac" not in opt else "1.0000000"):
                r = run("-o", "x.bam", "--pileup", "p.tsv", opt, bad)
                assert r.returncode != 0 and "Value parse failed for " + opt in r.stderr, (opt, bad, r.stderr)
        r = run("-o", "x.bam", "--pileup", "p.tsv", "--pileup-min-alt", "0")
        assert r.returncode != 0 and "Value parse failed for --pileup-min-alt" in r.stderr
        for bad in ("1.1", "-0", "2e-1", "0.1234567"):
            r = run("-o", "x.bam", "--pileup", "p.tsv", "--pileup-min-frac", bad)
            assert r.returncode != 0 and "Value parse failed for --pileup-min-frac" in r.stderr and "six fractional digits" in r.stderr
        for good in ("0", "1", "0.2", "0.000001"):
            r = run("-o", "x.bam", "--pileup", "p.tsv", "--pileup-min-frac", good)
            assert "Value parse failed" not in r.stderr and "Validation failed" not in r.stderr
        for other in ("--depth", "--coverage"):
            r = run("-o", "x.bam", other, "d.txt", "--pileup", "d.txt")
            assert r.returncode != 0 and "--pileup" in r.stderr and other in r.stderr and "Validation failed" in r.stderr
        assert not os.listdir(tmp_path)


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import pileup
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmp.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bmp_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(pileup.SYMBOLS) and len(names) == 9
    L = pileup.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    for n in ("bmp_create", "bmp_destroy", "bmp_last_error", "bmp_begin", "bmp_add", "bmp_finish", "bmp_sites", "bmp_counts_at", "bmp_last_stats"):
        assert n in names
    assert (pileup.N_COUNTERS, pileup.N_STATS, pileup.SITE_WORDS) == (8, 6, 12) and pileup.DEFAULTS == P.DEFAULTS


def test_argument_errors_need_no_device():
    from bucket_map_amd import pileup
    L = pileup.lib()
    u8p, u32p, u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64))
    recs = [full_record(ops=[4 << 4]), full_record(3, 2, 7, 5, ops=[3 << 4 | 4, 4 << 4 | 7])]
    good, good_off = b"".join(recs), offsets_of(recs)
    short = struct.pack("<I", 31) + bytes(31)
    lying = bytearray(good)
    lying[0] += 1
    unfit = {}
    for what, at, fmt, v in (("name", 12, "<B", 200), ("cigar", 16, "<H", 9), ("seq", 20, "<I", 40)):
        b = bytearray(good)
        struct.pack_into(fmt, b, good_off[1] + at, v)
        unfit[what] = bytes(b)
    cases = {
        "first offset": (good, [1, good_off[1], good_off[2]], 2, "rec_offset[0]"),
        "descending": (good, [0, good_off[2], good_off[1]], 2, "ascending"),
        "equal": (good, [0, good_off[1], good_off[1]], 2, "ascending"),
        "last offset": (good, [0, good_off[1]], 1, "the stream has"),
        "beyond": (good, [0, good_off[1], good_off[2] + 4], 2, "beyond"),
        "short record": (short, [0, 35], 1, "35 bytes"),
        "block_size": (bytes(lying), good_off, 2, "block_size"),
        "too many": (good, good_off, 2 ** 31, "2^31"),
        "name": (unfit["name"], good_off, 2, "do not fit"),
        "cigar": (unfit["cigar"], good_off, 2, "do not fit"),
        "seq": (unfit["seq"], good_off, 2, "do not fit"),
        "op code": (recs[0] + full_record(ops=[4 << 4 | 9]), offsets_of([recs[0]] * 2), 2, "a CIGAR op is 0 .. 8"),
        "op code 15": (full_record(2, 2, 4, ops=[4 << 4, 15]) + recs[0], offsets_of([full_record(2, 2, 4, ops=[4 << 4, 15]), recs[0]]), 2, "record 0"),
        "query short": (full_record(ops=[3 << 4]), offsets_of([recs[0]]), 1, "query bases"),
        "query long": (full_record(ops=[5 << 4 | 8]), offsets_of([recs[0]]), 1, "query bases"),
        "query by I and S": (full_record(2, 2, 4, ops=[2 << 4 | 1, 3 << 4 | 4]), offsets_of([full_record(2, 2, 4)]), 1, "5 query bases"),
    }

    def add(stream, off, n, null=(), skip=True):
        a = np.frombuffer(stream, np.uint8)
        o = np.asarray(off, np.uint64)
        s = np.zeros(8, np.uint8)
        p = dict(a=a.ctypes.data_as(u8p), o=o.ctypes.data_as(u64p))
        for k in null:
            p[k] = None
        return L.bmp_add(None, p["a"], len(stream), p["o"], n, s.ctypes.data_as(u8p) if skip else None)

    err = lambda: L.bmp_last_error().decode()
    for name, (stream, off, n, word) in cases.items():
        assert add(stream, off, n) == pileup.BMP_ERR_ARG, name
        assert word in err() and "bmp_add" in err(), (name, err())
    for null in ("a", "o"):
        assert add(good, good_off, 2, null=(null,)) == pileup.BMP_ERR_ARG and "null argument" in err()
    for skip in (True, False):                           # good data: only the context is missing
        assert add(good, good_off, 2, skip=skip) == pileup.BMP_ERR_ARG and "null context" in err()
    assert add(b"", [0], 0) == pileup.BMP_ERR_ARG and "null context" in err()
    fine = [full_record(2, 3, 4, ops=[4 << 4, 900 << 4 | 2, 7 << 4 | 5]), full_record(2, 0, 4), full_record(2, 1, 0, ops=[9 << 4])]
    assert add(b"".join(fine), offsets_of(fine), 3) == pileup.BMP_ERR_ARG and "null context" in err()

    def begin(lens, n=None, null=(), th=(0, 13, 2, 200000), bases=None):
        a = np.asarray(lens, np.uint32)
        t = np.asarray(th, np.uint32)
        # one shared byte for every reference: the checks that come before the context never read the bases
        one = np.zeros(8, np.uint8)
        ptrs = (C.c_void_p * len(lens))(*([one.ctypes.data] * len(lens) if bases is None else bases))
        p = dict(lens=a.ctypes.data_as(u32p), bases=ptrs, th=t.ctypes.data_as(u32p))
        for k in null:
            p[k] = None
        return L.bmp_begin(None, p["lens"], len(lens) if n is None else n, p["bases"], p["th"])

    assert begin([5], n=0) == pileup.BMP_ERR_ARG and "n_ref is 0" in err()
    assert begin([5, 0, 7]) == pileup.BMP_ERR_ARG and "reference 1 has the length 0" in err()
    assert begin([2 ** 32 - 2 ** 20, 1]) == pileup.BMP_ERR_ARG and "2^32 - 2^20" in err()
    assert begin([2 ** 31, 2 ** 31]) == pileup.BMP_ERR_ARG and "2^32 - 2^20" in err()
    for null in ("lens", "bases", "th"):
        assert begin([5], null=(null,)) == pileup.BMP_ERR_ARG and "null argument" in err()
    assert begin([5], th=(0, 13, 0, 200000)) == pileup.BMP_ERR_ARG and "min_alt" in err()
    assert begin([5], th=(0, 13, 2, 1000001)) == pileup.BMP_ERR_ARG and "min_frac_ppm" in err()
    one = np.zeros(8, np.uint8)
    assert begin([5, 5], bases=[one.ctypes.data, None]) == pileup.BMP_ERR_ARG and "reference 1 has no bases" in err()
    assert begin([2 ** 32 - 2 ** 20]) == pileup.BMP_ERR_ARG and "null context" in err()
    assert begin([1], th=(255, 255, 1, 1000000)) == pileup.BMP_ERR_ARG and "null context" in err()
    assert begin([1], th=(0, 0, 2 ** 32 - 1, 0)) == pileup.BMP_ERR_ARG and "null context" in err()
    n_sites, stats, out = C.c_uint64(0), np.zeros(6, np.uint64), np.zeros(12, np.uint32)
    assert L.bmp_finish(None, None, stats.ctypes.data_as(u64p)) == pileup.BMP_ERR_ARG and "null argument" in err()
    assert L.bmp_finish(None, C.byref(n_sites), None) == pileup.BMP_ERR_ARG and "null argument" in err()
    assert L.bmp_finish(None, C.byref(n_sites), stats.ctypes.data_as(u64p)) == pileup.BMP_ERR_ARG and "null context" in err()
    assert L.bmp_sites(None, 0, 1, None) == pileup.BMP_ERR_ARG and "null argument" in err()
    assert L.bmp_sites(None, 0, 1, out.ctypes.data_as(u32p)) == pileup.BMP_ERR_ARG and "null context" in err()
    assert L.bmp_counts_at(None, 0, 0, 1, None) == pileup.BMP_ERR_ARG and "null argument" in err()
    assert L.bmp_counts_at(None, 0, 0, 1, out.ctypes.data_as(u32p)) == pileup.BMP_ERR_ARG and "null context" in err()
    assert L.bmp_create(0, None) == pileup.BMP_ERR_ARG and L.bmp_last_stats(None, None, None) == pileup.BMP_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import pileup
    with pytest.raises(pileup.BmpError) as e:
        pileup.Pileup(0)
    assert e.value.code == pileup.BMP_ERR_HIP
