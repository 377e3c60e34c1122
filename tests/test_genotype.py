"""Genotypes (-o x.bam --vcf FILE) without a GPU: the rule on cases worked out by hand, host/genotype.h as a program of its own
under ASan + UBSan, the oracle-backed tools (whose calling is the host default of block_compressor), the command line and the
bmg_* ABI surface.

The yardstick is the rule of include/bmg.h in plain Python (tests/genotype_rule.py) at the sites of tests/pileup_rule.py,
applied to the records decoded from the x.bam the tool wrote and to the FASTA file: the VCF is a function of those alone.
"""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import genotype_rule as G
import pileup_rule as P
from pileup_cases import EDGE_REFS, REF_LENS, edge_bases, edge_records, many_ops_record, random_records, rec_letters, references
from test_bamsort import offsets_of, pair_of, records_of, run_tool
from test_depth import full_record, header_refs
from test_markdup_gpu import rec, rec_ops
from test_pileup import fasta_bases, pileup_line
from test_sam_golden import ROOT, TOOLS

GENOTYPES = re.compile(r"Genotypes: (\d+) variants \((\d+) het, (\d+) hom, (\d+) below QUAL\) at (\d+) SNV sites")
STRICT = dict(min_mapq=20, min_bq=13)
PARAM_SETS = ({}, dict(STRICT, q_cap=40, q_absent=0, prior=0), dict(min_bq=0, q_cap=93, q_absent=93, prior=100000), dict(min_bq=256, q_cap=1, q_absent=1))


def site(ref, pos, R, kind=1):
    return (ref, pos, R, 0, 0, 0, 0, 0, 0, 0, 0, kind)


def pile_at(letters_and_quals, R=0, **params):
    """The call at one position (reference 0, position 3, reference allele R) of one-base reads: [(letter, quality, times)]."""
    recs = [rec_letters(0, 3, "1M", letter, [q], name=b"%s%d_%d" % (letter.encode(), q, k)) for letter, q, times in letters_and_quals for k in range(times)]
    n, Q, called = G.genotype(recs, [8], [site(0, 3, R)], **params)
    return n[0][3].tolist(), Q[0][3].tolist(), called[0]


# ---- the rule itself, on cases worked out by hand ----
def test_python_restatement_of_the_rule():
    # ten A and ten C at q40 on an A: M(A) = M(C) = 100 * 400 + 477 * 10 = 44770, T = 3010.
    # L'(AA) = M(C) = 44770, L'(AC) = 6020 + 3000 = 9020, L'(CC) = 44770 + 3000; every other genotype pays both M
    n, Q, c = pile_at([("A", 40, 10), ("C", 40, 10)])
    assert n == [10, 10, 0, 0] and Q == [400, 400, 0, 0]
    assert c[:8] == (0, 3, 0, 3, 0, 1, 99, 35750) and c[8:12] == (10, 10, 0, 0) and c[22:] == (20, 0)
    assert c[12:15] == (35750, 0, 38750) and c[12 + 3] == 3010 + 44770 + 3000 - 9020              # AG: T(A) + T(G) + M(C) + one prior
    # eight A and two C: L'(AA) = M(C) = 8000 + 954, L'(AC) = 3010 + 3000
    n, Q, c = pile_at([("A", 40, 8), ("C", 40, 2)])
    assert c[3:8] == (3, 0, 1, 29, 2944) and c[12:15] == (2944, 0, 32000 + 3816 + 3000 - 6010)
    # twenty-eight A and two C: L'(AC) = 301 * 30 + 3000 = 12030 > 8954
    n, Q, c = pile_at([("A", 40, 28), ("C", 40, 2)])
    assert c[3:8] == (1, 0, 0, 30, 0) and c[12] == 0 and c[13] == 12030 - 8954
    # two letters other than the reference's and none of it: five C and five G on an A.  M = 22385 each, L'(CG) = 3010 + 6000,
    # L'(CC) = L'(GG) = 22385 + 3000, L'(AA) = 44770
    n, Q, c = pile_at([("C", 40, 5), ("G", 40, 5)])
    assert c[3:8] == (3, 1, 2, 99, 44770 - 9010) and c[12:22] == (35760, 22385 + 1505 + 3000 - 9010, 16375, 22385 + 1505 + 3000 - 9010, 0, 16375,
                                                                  44770 + 3000 - 9010, 22385 + 1505 + 6000 - 9010, 22385 + 1505 + 6000 - 9010, 44770 + 3000 - 9010)
    line = G.vcf_lines([c], ["chr"])[0].split("\t")
    assert line == ["chr", "4", ".", "A", "C,G", "357.60", "PASS", "DP=10", "GT:DP:AD:GQ:PL", "1/2:10:0,5,5:99:357,178,163,178,0,163"]
    # an exact tie of RR with a het: one A and one C at q40, M(C) = 4477 = 301 * 2 + prior at prior 3875 -- RR wins it
    assert pile_at([("A", 40, 1), ("C", 40, 1)], prior=3875)[2][3:8] == (1, 0, 0, 0, 0)
    assert pile_at([("A", 40, 1), ("C", 40, 1)], prior=3874)[2][3:8] == (3, 0, 1, 0, 1)
    # a tie without RR goes to the smallest index: one C and one G on a T at that prior.  CG = 602 + 2 * 3875 and CC = GG =
    # 4477 + 3875 are all 8352, TT is 8954: CC has the smallest index (2 < 4 < 5), and GQ is 0
    n, Q, c = pile_at([("C", 40, 1), ("G", 40, 1)], R=3, prior=3875)
    assert c[3:8] == (3, 1, 1, 0, 8954 - 8352)
    # quality: above q_cap counts as q_cap, 0xFF as q_absent, one below min_bq not at all, min_bq itself does
    assert pile_at([("C", 93, 1)])[1] == [0, 60, 0, 0] and pile_at([("C", 93, 1)], q_cap=93)[1] == [0, 93, 0, 0]
    assert pile_at([("C", 255, 2)])[:2] == ([0, 2, 0, 0], [0, 60, 0, 0]) and pile_at([("C", 255, 1)], q_absent=0, min_bq=256)[:2] == ([0, 1, 0, 0], [0, 0, 0, 0])
    assert pile_at([("C", 12, 3), ("G", 13, 1)])[:2] == ([0, 0, 1, 0], [0, 0, 13, 0])
    assert pile_at([("C", 12, 3)])[2] == (0, 3, 0) + (0,) * 21                 # nothing counted: not genotyped
    assert pile_at([("N", 40, 3), ("=", 40, 1), ("T", 40, 1)])[0] == [0, 0, 0, 1]
    # a site without the SNV bit, and one without a reference allele: the n all the same
    recs = [rec_letters(0, 3, "1M", "C", name=b"c%d" % k) for k in range(4)]
    n, Q, called = G.genotype(recs, [8], [site(0, 3, 0, kind=6), site(0, 3, 4), site(0, 3, 1), site(0, 2, 0)])
    assert called[0] == (0, 3, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0) + (0,) * 12 and called[1] == (0, 3, 4, 0, 0, 0, 0, 0, 0, 4, 0, 0) + (0,) * 12
    assert called[2][3:8] == (1, 1, 1, 42, 0) and called[3] == (0, 2, 0) + (0,) * 21      # CC on a C is RR, the next is a het at 1204 + 3000; no base at 2
    # prior 0: the likelihoods alone -- one C among three A at q40 is a het (M(C) = 4477 > 301 * 4)
    assert pile_at([("A", 40, 3), ("C", 40, 1)], prior=0)[2][3:8] == (3, 0, 1, 32, 4477 - 1204)
    assert pile_at([("A", 40, 3), ("C", 40, 1)])[2][3:8] == (3, 0, 1, 2, 4477 - 4204)    # ... at the default prior by a little
    assert pile_at([("A", 40, 3), ("C", 40, 1)], prior=3274)[2][3:8] == (1, 0, 0, 0, 0)  # ... and no longer one step beyond the tie
    # MAPQ below min_mapq: not counted
    low = [rec_letters(0, 3, "1M", "C", name=b"m19", mapq=19), rec_letters(0, 3, "1M", "G", name=b"m20", mapq=20)]
    assert G.cells(low, [8], min_mapq=20)[0][0][3].tolist() == [0, 0, 1, 0] and G.cells(low, [8])[0][0][3].tolist() == [0, 1, 1, 0]


def test_cells_agree_with_the_pileup_on_the_edge_list():
    recs, bases = edge_records(), edge_bases()
    for th in ({}, STRICT, dict(min_bq=0), dict(min_bq=256, min_mapq=31), dict(min_bq=41)):
        n, Q = G.cells(recs, EDGE_REFS, **th)
        want = P.pile(recs, EDGE_REFS, bases, **th)
        for r in range(len(EDGE_REFS)):
            assert np.array_equal(n[r], want.counts[r][:, :4]), (th, r)
            assert ((Q[r] > 0) <= (n[r] > 0)).all() and (Q[r] <= 60 * n[r]).all()
    assert sum(int(x.sum()) for x in n) > 0


# ---- host/genotype.h as a program of its own ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("genotype_check")
    exe = str(d / "genotype_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "genotype_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def clean(r, expect=0):
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode == expect, r.stderr[-3000:]
    return r.stdout


def run_check(checker, recs, ref_len, sites, n_calls=1, seed=0, skip=None, expect=0, **params):
    d, exe = checker
    pr = {**G.DEFAULTS, **params}
    (d / "records.bin").write_bytes(b"".join(recs))
    (d / "sites.bin").write_bytes(np.asarray(sites, np.uint32).tobytes())
    if skip is not None:
        (d / "skip.bin").write_bytes(bytes(skip))
    r = subprocess.run([exe, "records.bin", "skip.bin" if skip is not None else "-", "sites.bin", str(n_calls), str(seed),
                        *[str(pr[k]) for k in ("min_mapq", "min_bq", "q_absent", "q_cap", "prior")], *[str(x) for x in ref_len]],
                       cwd=str(d), capture_output=True, text=True)
    return clean(r, expect)


def same_as_rule(out, n, Q, called):
    lines = out.split("\n")
    count = int(lines[0].split()[1])
    assert [tuple(int(x) for x in l.split()) for l in lines[1: 1 + count]] == called
    cells = [np.array([int(x) for x in l.split()[1:]], np.uint64).reshape(-1, 4) for l in lines[1 + count:] if l.startswith("cells")]
    assert len(cells) == len(n) and all(np.array_equal(c, G.packed(a, b)) for c, a, b in zip(cells, n, Q))


def sites_for(recs, ref_len, bases, **pile_th):
    """The pileup's sites under loose thresholds, so that many are no variant, with a few that are no SNV site or have no
    reference allele put between them."""
    sites = P.pile(recs, ref_len, bases, **{**dict(min_alt=1, min_frac_ppm=0), **pile_th}).sites
    assert sites
    extra = [site(s[0], s[1], 4) for s in sites[::7]] + [site(s[0], s[1], s[2], kind=6) for s in sites[::5]]
    return sites + extra


@pytest.fixture(scope="module")
def ref_bases():
    return references()


@pytest.mark.parametrize("size", [0, 1, 65, 1025, 20001])
def test_host_rule_is_the_python_rule(checker, ref_bases, size):
    recs = random_records(size, 300 + size, bases=ref_bases)
    sites = sites_for(recs, REF_LENS, ref_bases) if size > 1 else [site(0, 0, 0), site(5, REF_LENS[5] - 1, 2)]
    n, Q, called = G.genotype(recs, REF_LENS, sites)
    one = run_check(checker, recs, REF_LENS, sites)
    same_as_rule(one, n, Q, called)
    if size >= 1025:
        assert sum(1 for c in called if c[3] & 2) > 20 and sum(1 for c in called if c[3] == 1) > 20 and any(c[4] != c[5] for c in called)
    if size in (65, 1025):                               # order and cutting do not matter; other parameters
        assert run_check(checker, recs, REF_LENS, sites, n_calls=3, seed=1 + size) == one
        assert run_check(checker, recs, REF_LENS, sites, n_calls=7, seed=size) == one
        for pr in PARAM_SETS[1:]:
            same_as_rule(run_check(checker, recs, REF_LENS, sites, **pr), *G.genotype(recs, REF_LENS, sites, **pr))


def test_host_rule_on_the_edges_and_a_record_of_many_ops(checker):
    recs, bases = edge_records(), edge_bases()
    sites = sites_for(recs, EDGE_REFS, bases, min_bq=0) + [site(r, p, p % 4) for r, length in enumerate(EDGE_REFS) for p in (0, length - 1)]
    for pr in PARAM_SETS:
        one = run_check(checker, recs, EDGE_REFS, sites, **pr)
        same_as_rule(one, *G.genotype(recs, EDGE_REFS, sites, **pr))
        assert run_check(checker, recs, EDGE_REFS, sites, n_calls=3, seed=3, **pr) == one
    assert run_check(checker, recs, EDGE_REFS, sites[::-1]).split("\n")[1: 1 + len(sites)] == run_check(checker, recs, EDGE_REFS, sites).split("\n")[len(sites):0:-1]
    refs = [90000, 300]
    bases = references(refs, 4)
    recs = random_records(40, 5, refs, bases) + [many_ops_record(0, 17)] + random_records(40, 6, refs, bases)
    sites = sites_for(recs, refs, bases)
    n, Q, called = G.genotype(recs, refs, sites)
    assert int(n[0].sum()) > 30000 and sum(1 for c in called if c[3] & 2) > 100
    same_as_rule(run_check(checker, recs, refs, sites), n, Q, called)
    skip = [int(k % 3 == 1) for k in range(len(recs))]
    same_as_rule(run_check(checker, recs, refs, sites, skip=skip), *G.genotype(recs, refs, sites, skip))
    assert run_check(checker, recs, refs, sites, skip=skip) == run_check(checker, [r for r, s in zip(recs, skip) if not s], refs, sites)


def test_host_rule_refuses_what_the_abi_refuses(checker, ref_bases):
    good = random_records(10, 1, bases=ref_bases)
    ok = [site(0, 0, 0)]
    for bad in (rec_ops(0, 0, 0, [3 << 4 | 9], b""), rec(1, 5, 0, "3M", b"ab"), rec(6, 5, 0, "3M", b""), rec(1, 5, 0, "3M2I", b"abcd")):
        assert G.refused([bad], len(REF_LENS))
        assert run_check(checker, good + [bad], REF_LENS, ok, expect=3).startswith("refused ")
    assert run_check(checker, good + [rec(6, 5, 4, "3M", b"")], REF_LENS, ok).startswith("calls 1")   # unmapped: its reference is not looked at
    assert run_check(checker, good, [5, 0, 5], ok, expect=3).startswith("refused ")
    for pr in (dict(q_cap=0), dict(q_cap=94), dict(q_absent=61)):
        assert run_check(checker, good, REF_LENS, ok, expect=3, **pr).startswith("refused ")
    assert run_check(checker, good, REF_LENS, ok, q_cap=93, q_absent=93).startswith("calls 1")
    for bad_site in (site(len(REF_LENS), 0, 0), site(0, REF_LENS[0], 0)):
        assert run_check(checker, good, REF_LENS, ok + [bad_site], expect=3).startswith("refused ")
    assert run_check(checker, good, REF_LENS, []).startswith("calls 0\n")


def test_vcf_writer_is_the_python_text(checker):
    d, exe = checker
    recs, bases = edge_records(), edge_bases()
    refs = [90000, 300]
    big = references(refs, 4)
    more = random_records(400, 5, refs, big)
    bodies = []
    for rs, lens, bs, names in ((recs, EDGE_REFS, bases, ["one", "two", "three"]), (more, refs, big, ["chr1", "chr 2"])):
        sites = sites_for(rs, lens, bs, min_bq=0)
        for pr, min_qual, sample in (({}, 20, "sample"), (dict(prior=0, min_bq=0), 0, "a b"), (dict(prior=25500), 1000, "x")):
            called = G.genotype(rs, lens, sites, **pr)[2]
            (d / "calls.bin").write_bytes(np.asarray(called, np.uint32).tobytes())
            r = subprocess.run([exe, "vcf", "calls.bin", str(min_qual), sample, *[f"{n}:{l}" for n, l in zip(names, lens)]], cwd=str(d), capture_output=True, text=True)
            body = G.check_vcf_header(clean(r), list(zip(names, lens)), sample)
            assert body == G.vcf_lines(called, names, min_qual)
            assert "Genotypes: %s variants (%s het, %s hom, %s below QUAL)" % tuple(r.stderr.split()[1:]) in G.summary_line(called, sites, min_qual)
            bodies.append(body)
    assert all(len(b) >= 5 for b in bodies) and sum("," in l.split("\t")[4] for l in bodies[0]) > 10             # two ALT letters too
    assert [{l.split("\t")[6] for l in b} for b in bodies[:3]] == [{"PASS", "LowQual"}, {"PASS"}, {"LowQual"}]


# ---- the oracle-backed tools ----
def genotypes_by_the_rule(bam_path, args, sample="sample", min_qual=20, pile_th=None, **params):
    """(the lines of the --vcf file below its header, the stderr line, the references, the pileup's result) for the records of
    a BAM file and the FASTA file of the tool's arguments."""
    fasta = os.path.join(os.path.dirname(bam_path), args[args.index("--genome") + 1])
    cut = int(args[args.index("--bucket-len") + 1]), int(args[args.index("-r") + 1])
    raw = gzip.decompress(open(bam_path, "rb").read())
    refs = header_refs(raw)
    recs = [r for _, r in records_of(raw)[0]]
    lens = [l for _, l in refs]
    pile_th = {**P.DEFAULTS, **(pile_th or {})}
    res = P.pile(recs, lens, fasta_bases(fasta, refs, *cut), **pile_th)
    called = G.genotype(recs, lens, res.sites, min_mapq=pile_th["min_mapq"], min_bq=pile_th["min_bq"], **params)[2]
    return G.vcf_lines(called, [n for n, _ in refs], min_qual), G.summary_line(called, res.sites, min_qual), refs, res


def genotypes_line(err):
    found = [l.split("\t")[-1] for l in err.split("\n") if "Genotypes:" in l]
    assert len(found) == 1 and GENOTYPES.fullmatch(found[0]), err
    return found[0]


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_pileup import pileup_jobs
    return pileup_jobs(tmp_path_factory)


LOOSE_OPTS = ["--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--pileup-min-bq", "0"]
LOOSE = dict(min_bq=0, min_alt=1, min_frac_ppm=1)


@pytest.mark.parametrize("k", range(3))
def test_oracle_tool_writes_what_the_rule_says(jobs, k):
    name, which, d, args, extra = jobs[k]
    exe = TOOLS[(which, "oracle")]
    implied = ["--annotate"] if which == "bucketmap_align" else []               # what --vcf implies beside --sort
    err = run_tool(exe, d, args, f"{name}.vs.bam", [*extra, *implied, "--sort"])
    assert "Genotypes:" not in err
    # --vcf alone: the pileup is counted, its file is not written and its line is not printed
    err = run_tool(exe, d, args, f"{name}.v.bam", [*extra, "--vcf", f"{name}.v.vcf"])
    assert re.search(r"Sorted \d+ records by coordinate in 1 run", err) and "Pileup:" not in err
    assert pair_of(d, f"{name}.v") == pair_of(d, f"{name}.vs")                   # the BAM and its index are what they were
    assert not [f for f in os.listdir(d) if f.startswith(f"{name}.v.") and f not in (f"{name}.v.bam", f"{name}.v.bam.bai", f"{name}.v.vcf")]
    lines, told, refs, res = genotypes_by_the_rule(d / f"{name}.v.bam", args)
    text = (d / f"{name}.v.vcf").read_text()
    assert G.check_vcf_header(text, refs) == lines and genotypes_line(err) == told
    aligned = name != "plain"                            # the plain tool writes no CIGAR: no counted record, only the header
    assert (len(lines) > 3 and any("0/1" in l for l in lines) and any("1/1" in l for l in lines)) if aligned else (lines == [] and " 0 SNV sites" in told)
    # with --pileup: both files, the pileup's as without --vcf, the VCF the same
    run_tool(exe, d, args, f"{name}.vp0.bam", [*extra, "--pileup", f"{name}.vp0.tsv"])
    err = run_tool(exe, d, args, f"{name}.vp.bam", [*extra, "--vcf", f"{name}.vp.vcf", "--pileup", f"{name}.vp.tsv"])
    assert (d / f"{name}.vp.vcf").read_text() == text and (d / f"{name}.vp.tsv").read_text() == (d / f"{name}.vp0.tsv").read_text()
    assert genotypes_line(err) == told and pileup_line(err) and pair_of(d, f"{name}.vp") == pair_of(d, f"{name}.vs")
    # looser pileup thresholds without --pileup, the three options of --vcf, in one run and in several
    opts = [*LOOSE_OPTS, "--vcf-prior", "0", "--vcf-min-qual=50", "--vcf-sample", "NA 1"]
    err = run_tool(exe, d, args, f"{name}.vl.bam", [*extra, "--vcf", f"{name}.vl.vcf", *opts])
    l_lines, l_told, _, l_res = genotypes_by_the_rule(d / f"{name}.vl.bam", args, pile_th=LOOSE, prior=0, min_qual=50)
    l_text = (d / f"{name}.vl.vcf").read_text()
    assert G.check_vcf_header(l_text, refs, "NA 1") == l_lines and genotypes_line(err) == l_told
    assert not aligned or (len(l_lines) > len(lines) and any(l.split("\t")[6] == "LowQual" for l in l_lines) and any(l.split("\t")[6] == "PASS" for l in l_lines))
    err = run_tool(exe, d, args, f"{name}.vr.bam", [*extra, "--vcf", f"{name}.vr.vcf", *opts], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1
    assert (d / f"{name}.vr.vcf").read_text() == l_text and genotypes_line(err) == l_told and pair_of(d, f"{name}.vr") == pair_of(d, f"{name}.vs")
    # with --markdup the duplicates are left out: the rule on the marked records
    run_tool(exe, d, args, f"{name}.vm0.bam", [*extra, *implied, "--markdup"])
    err = run_tool(exe, d, args, f"{name}.vm.bam", [*extra, "--markdup", "--vcf", f"{name}.vm.vcf", *LOOSE_OPTS, "--vcf-prior", "255"])
    assert pair_of(d, f"{name}.vm") == pair_of(d, f"{name}.vm0")
    m_lines, m_told, _, m_res = genotypes_by_the_rule(d / f"{name}.vm.bam", args, pile_th=LOOSE, prior=25500)
    m_text = (d / f"{name}.vm.vcf").read_text()
    assert G.check_vcf_header(m_text, refs) == m_lines and genotypes_line(err) == m_told
    assert not aligned or sum(s[0] for s in m_res.stats) < sum(s[0] for s in l_res.stats)
    err = run_tool(exe, d, args, f"{name}.vmr.bam", [*extra, "--markdup", "--vcf", f"{name}.vmr.vcf", *LOOSE_OPTS, "--vcf-prior", "255"],
                   env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1 and (d / f"{name}.vmr.vcf").read_text() == m_text
    # beside --depth and --coverage
    err = run_tool(exe, d, args, f"{name}.vd.bam", [*extra, "--depth", f"{name}.vd.bedgraph", "--coverage", f"{name}.vd.cov", "--vcf", f"{name}.vd.vcf"])
    assert "Coverage:" in err and genotypes_line(err) == told and (d / f"{name}.vd.vcf").read_text() == text


# ---- the command line ----
def test_cli_refusals(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        run = lambda *opts: subprocess.run([exe, "-i", "idx", *opts], cwd=str(tmp_path), capture_output=True, text=True)
        fine = lambda r: "Validation failed" not in r.stderr and "Unknown option" not in r.stderr and "Value parse failed" not in r.stderr
        r = run("--vcf", "v.vcf", "-o", "x.sam")
        assert r.returncode != 0 and "x.bam" in r.stderr and "--vcf" in r.stderr and "only BAM output is sorted and indexed" in r.stderr, r.stderr
        r = run("--vcf", "v.vcf")
        assert r.returncode != 0 and "-o x.bam" in r.stderr and "--vcf" in r.stderr, r.stderr
        r = run("--vcf")
        assert r.returncode != 0 and "Missing value" in r.stderr
        assert fine(run("-o", "x.bam", "--vcf", "v.vcf")) and fine(run("-o", "x.bam", "--vcf", "v.vcf", "--pileup", "p.tsv", "--markdup", "--depth", "d.txt"))
        for opt, value in (("--vcf-prior", "20"), ("--vcf-min-qual", "30"), ("--vcf-sample", "NA12878")):
            r = run("-o", "x.bam", opt, value)                                    # an option of --vcf without it
            assert r.returncode != 0 and opt in r.stderr and "--vcf FILE" in r.stderr and "Validation failed" in r.stderr, r.stderr
            r = run("-o", "x.bam", "--pileup", "p.tsv", opt, value)
            assert r.returncode != 0 and "--vcf FILE" in r.stderr
            assert fine(run("-o", "x.bam", opt, value, "--vcf", "v.vcf"))
            r = run("-o", "x.bam", "--vcf", "v.vcf", opt)
            assert r.returncode != 0 and "Missing value" in r.stderr
        for opt, bads in (("--vcf-prior", ("x", "-1", "", "256", "1.5")), ("--vcf-min-qual", ("x", "-1", "", "4294967296", "2e1")),
                          ("--vcf-sample", ("a\tb", "a\nb", ""))):
            for bad in bads:
                r = run("-o", "x.bam", "--vcf", "v.vcf", opt, bad)
                assert r.returncode != 0 and "Value parse failed for " + opt in r.stderr, (opt, bad, r.stderr)
        assert fine(run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-prior", "0")) and fine(run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-prior", "255"))
        # the pileup's thresholds: accepted with --vcf alone, refused as before without either
        for opt, value in (("--pileup-min-bq", "20"), ("--pileup-min-mapq", "20"), ("--pileup-min-alt", "3"), ("--pileup-min-frac", "0.5")):
            assert fine(run("-o", "x.bam", "--vcf", "v.vcf", opt, value))
            r = run("-o", "x.bam", opt, value)
            assert r.returncode != 0 and opt in r.stderr and "it is a threshold of --pileup FILE, which is not given." in r.stderr
        for other in ("--pileup", "--depth", "--coverage"):
            r = run("-o", "x.bam", other, "same.txt", "--vcf", "same.txt")
            assert r.returncode != 0 and "--vcf" in r.stderr and other in r.stderr and "Validation failed" in r.stderr and "same.txt" in r.stderr
        assert not os.listdir(tmp_path)


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import genotype
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmg.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bmg_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(genotype.SYMBOLS) and len(names) == 8
    L = genotype.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    for n in ("bmg_create", "bmg_destroy", "bmg_last_error", "bmg_begin", "bmg_add", "bmg_call", "bmg_cells_at", "bmg_last_stats"):
        assert n in names
    assert (genotype.N_CELLS, genotype.SITE_WORDS, genotype.CALL_WORDS) == (4, 12, 24) and genotype.DEFAULTS == G.DEFAULTS
    assert list(genotype.PARAMS) == list(G.DEFAULTS) and [G.GENOTYPES.index((a, b)) for b in range(4) for a in range(b + 1)] == list(range(10))
    assert "".join(genotype.GENOTYPES) == "".join("ACGT"[a] + "ACGT"[b] for a, b in G.GENOTYPES)
    for word in ("BMG_CALL_WORDS = 24", "BMG_N_PARAMS = 5", "202 GB", "65 bytes per base"):
        assert word in open(os.path.join(ROOT, "include", "bmg.h")).read()


def test_argument_errors_need_no_device():
    from bucket_map_amd import genotype
    L = genotype.lib()
    u8p, u32p, u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64))
    recs = [full_record(ops=[4 << 4]), full_record(3, 2, 7, 5, ops=[3 << 4 | 4, 4 << 4 | 7])]
    good, good_off = b"".join(recs), offsets_of(recs)
    lying = bytearray(good)
    lying[0] += 1
    unfit = bytearray(good)
    struct.pack_into("<I", unfit, good_off[1] + 20, 40)
    cases = {                                            # bmp_add's checks, in its order
        "first offset": (good, [1, good_off[1], good_off[2]], 2, "rec_offset[0]"),
        "descending": (good, [0, good_off[2], good_off[1]], 2, "ascending"),
        "last offset": (good, [0, good_off[1]], 1, "the stream has"),
        "block_size": (bytes(lying), good_off, 2, "block_size"),
        "too many": (good, good_off, 2 ** 31, "2^31"),
        "seq": (bytes(unfit), good_off, 2, "do not fit"),
        "op code": (recs[0] + full_record(ops=[4 << 4 | 9]), offsets_of([recs[0]] * 2), 2, "a CIGAR op is 0 .. 8"),
        "query short": (full_record(ops=[3 << 4]), offsets_of([recs[0]]), 1, "query bases"),
        "stream before records": (bytes(unfit), [0, good_off[2], good_off[1]], 2, "ascending"),
        "fit before op code": (bytes(unfit[: good_off[1]]) + bytes(unfit[good_off[1]:]), good_off, 2, "do not fit"),
    }

    def add(stream, off, n, null=(), skip=True):
        a = np.frombuffer(stream, np.uint8)
        o = np.asarray(off, np.uint64)
        s = np.zeros(8, np.uint8)
        p = dict(a=a.ctypes.data_as(u8p), o=o.ctypes.data_as(u64p))
        for k in null:
            p[k] = None
        return L.bmg_add(None, p["a"], len(stream), p["o"], n, s.ctypes.data_as(u8p) if skip else None)

    err = lambda: L.bmg_last_error().decode()
    for name, (stream, off, n, word) in cases.items():
        assert add(stream, off, n) == genotype.BMG_ERR_ARG, name
        assert word in err() and "bmg_add" in err(), (name, err())
    for null in ("a", "o"):
        assert add(good, good_off, 2, null=(null,)) == genotype.BMG_ERR_ARG and "null argument" in err()
    for skip in (True, False):                           # good data: only the context is missing
        assert add(good, good_off, 2, skip=skip) == genotype.BMG_ERR_ARG and "null context" in err()
    assert add(b"", [0], 0) == genotype.BMG_ERR_ARG and "null context" in err()

    def begin(lens, n=None, null=(), pr=(0, 13, 30, 60, 3000)):
        a, t = np.asarray(lens, np.uint32), np.asarray(pr, np.uint32)
        p = dict(lens=a.ctypes.data_as(u32p), pr=t.ctypes.data_as(u32p))
        for k in null:
            p[k] = None
        return L.bmg_begin(None, p["lens"], len(lens) if n is None else n, p["pr"])

    assert begin([5], n=0) == genotype.BMG_ERR_ARG and "n_ref is 0" in err()
    assert begin([5, 0, 7]) == genotype.BMG_ERR_ARG and "reference 1 has the length 0" in err()
    assert begin([2 ** 32 - 2 ** 20, 1]) == genotype.BMG_ERR_ARG and "2^32 - 2^20" in err()
    for null in ("lens", "pr"):
        assert begin([5], null=(null,)) == genotype.BMG_ERR_ARG and "null argument" in err()
    assert begin([5], pr=(0, 13, 0, 0, 3000)) == genotype.BMG_ERR_ARG and "q_cap" in err()
    assert begin([5], pr=(0, 13, 30, 94, 3000)) == genotype.BMG_ERR_ARG and "q_cap" in err()
    assert begin([5], pr=(0, 13, 61, 60, 3000)) == genotype.BMG_ERR_ARG and "q_absent" in err()
    assert begin([2 ** 32 - 2 ** 20]) == genotype.BMG_ERR_ARG and "null context" in err()
    assert begin([1], pr=(255, 255, 93, 93, 2 ** 32 - 1)) == genotype.BMG_ERR_ARG and "null context" in err()
    sites, out, cells = np.zeros(12, np.uint32), np.zeros(24, np.uint32), np.zeros(4, np.uint64)
    assert L.bmg_call(None, None, 1, out.ctypes.data_as(u32p)) == genotype.BMG_ERR_ARG and "null argument" in err()
    assert L.bmg_call(None, sites.ctypes.data_as(u32p), 1, None) == genotype.BMG_ERR_ARG and "null argument" in err()
    assert L.bmg_call(None, sites.ctypes.data_as(u32p), 1, out.ctypes.data_as(u32p)) == genotype.BMG_ERR_ARG and "null context" in err()
    assert L.bmg_call(None, None, 0, None) == genotype.BMG_ERR_ARG and "null context" in err()
    assert L.bmg_cells_at(None, 0, 0, 1, None) == genotype.BMG_ERR_ARG and "null argument" in err()
    assert L.bmg_cells_at(None, 0, 0, 1, cells.ctypes.data_as(u64p)) == genotype.BMG_ERR_ARG and "null context" in err()
    assert L.bmg_create(0, None) == genotype.BMG_ERR_ARG and L.bmg_last_stats(None, None, None) == genotype.BMG_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import genotype
    with pytest.raises(genotype.BmgError) as e:
        genotype.Genotype(0)
    assert e.value.code == genotype.BMG_ERR_HIP
