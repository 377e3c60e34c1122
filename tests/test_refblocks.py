"""Reference blocks (-o x.bam --gvcf FILE) without a GPU: the rule on cases worked out by hand, host/refblocks.h as a program of
its own against the Python rule, the gVCF writer, the oracle-backed tools (whose blocks are the host default of
block_compressor), the command line and the bmr_* ABI surface.

The yardstick is the rule of include/bmr.h in plain Python (tests/refblocks_rule.py) over the cells of tests/genotype_rule.py,
applied to the records decoded from the x.bam the tool wrote and to the FASTA file."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import genotype_rule as G
import refblocks_rule as R
from pileup_cases import EDGE_REFS, REF_LENS, edge_bases, edge_records, random_records, rec_letters, references
from test_bamsort import pair_of, records_of, run_tool
from test_depth import header_refs
from test_pileup import fasta_bases
from test_sam_golden import ROOT, TOOLS

BLOCKS = re.compile(r"Blocks: (\d+) blocks on (\d+) of (\d+) bases \((\d+) in band 0, (\d+) under variant lines, (\d+) without a reference allele\)")


def blocks_line(err):
    found = [l.split("\t")[-1] for l in err.split("\n") if "Blocks:" in l]
    assert len(found) == 1 and BLOCKS.fullmatch(found[0]), err
    return found[0]


def gq_of(letters_and_quals, R_allele=0):
    """gq at one position of one-base reads [(letter, quality, times)] on the reference allele R, through the cells."""
    recs = [rec_letters(0, 3, "1M", letter, [q], name=b"%s%d_%d" % (letter.encode(), q, k)) for letter, q, times in letters_and_quals for k in range(times)]
    n, Q = G.cells(recs, [8])
    one = R.gq_one(n[0][3], Q[0][3], R_allele)
    word0, dp, blks = R.run(n, Q, [b"ACGT"[R_allele: R_allele + 1] * 8])
    assert int(word0[0][3]) & 0xFF == one and int(dp[0][3]) == sum(t for _, q, t in letters_and_quals if q >= 13)
    return one


# ---- the rule itself, on cases worked out by hand ----
def test_python_restatement_of_the_rule():
    assert gq_of([]) == 0                                 # no base: every cost is 0
    assert gq_of([("A", 30, 10)]) == 30                   # L(RR) = 0, h = L(AC) = 301 * 10
    assert gq_of([("A", 30, 40)]) == 99                   # 120 without the cap
    assert gq_of([("A", 30, 5), ("C", 30, 5)]) == 0       # L(AA) = M(C) = 15000 + 2385 > L(AC) = 3010: RR loses
    # nine A and one C of quality 20: L(AA) = M(C) = 2000 + 477, h = L(AC) = 301 * 10
    assert R.costs([9, 1, 0, 0], [270, 20, 0, 0])[:2] == [2477, 3010] and gq_of([("A", 30, 9), ("C", 20, 1)]) == 5
    assert gq_of([("C", 30, 10)], R_allele=1) == 30 and gq_of([("C", 30, 10)], R_allele=0) == 0
    assert gq_of([("A", 30, 10), ("C", 12, 7)]) == 30     # below min_bq: not counted
    # bands, states and blocks: 12 positions, the reads of depth 10 over 2 .. 5, an N at 7, an interval over 9 .. 10
    recs = [rec_letters(0, 2, "4M", "AAAA", [30] * 4, name=b"r%d" % k) for k in range(10)]
    n, Q = G.cells(recs, [12, 2])
    word0, dp, blks = R.run(n, Q, [b"AAAAAAANAAAa", b"CC"], (1, 10, 30, 31), [(0, 9, 11)])
    assert blks == [(0, 0, 2, 0, 0, 0, 0, 0), (0, 2, 6, 3, 30, 10, 40, 0), (0, 6, 7, 0, 0, 0, 0, 0), (0, 8, 9, 0, 0, 0, 0, 0), (0, 11, 12, 0, 0, 0, 0, 0),
                    (1, 0, 2, 0, 0, 0, 0, 0)]
    assert word0[0].tolist() == [R.IN] * 2 + [R.IN | 3 << 8 | 30] * 4 + [R.IN, R.NO_ALLELE, R.IN, R.EXCLUDED, R.EXCLUDED, R.IN]
    R.check_tiling(blks, word0)
    assert R.run(n, Q, [b"AAAAAAANAAAa", b"CC"], (), [(0, 7, 8)])[0][0][7] == R.EXCLUDED          # excluded even if R = 4
    assert [b[:4] for b in R.run(n, Q, [b"AAAAAAAAAAAA", b"CC"], ())[2]] == [(0, 0, 12, 0), (1, 0, 2, 0)]   # no bands: one per reference
    names = ["one", "two"]
    assert R.block_lines(blks, names, [b"AAAAAAANAAAa", b"CC"])[1][2] == "one\t3\t.\tA\t<NON_REF>\t.\t.\tEND=6\tGT:DP:GQ:MIN_DP\t0/0:10:30:10"
    assert R.summary_line(blks, word0) == "Blocks: 6 blocks on 11 of 14 bases (7 in band 0, 2 under variant lines, 1 without a reference allele)"


# ---- host/refblocks.h as a program of its own ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("refblocks_check")
    exe = str(d / "refblocks_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "refblocks_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def clean(r, expect=0):
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode == expect, r.stderr[-3000:]
    return r.stdout


def run_check(checker, recs, ref_len, bases, bands=R.DEFAULT_BANDS, exclude=(), n_calls=1, expect=0, **params):
    d, exe = checker
    pr = {**G.DEFAULTS, **params}
    (d / "records.bin").write_bytes(b"".join(recs))
    (d / "bases.bin").write_bytes(b"".join(bases))
    (d / "exclude.bin").write_bytes(np.asarray(exclude, np.uint32).tobytes())
    r = subprocess.run([exe, "records.bin", "bases.bin", ",".join(str(b) for b in bands) or "-", "exclude.bin" if len(exclude) else "-", str(n_calls),
                        *[str(pr[k]) for k in ("min_mapq", "min_bq", "q_absent", "q_cap")], *[str(x) for x in ref_len]],
                       cwd=str(d), capture_output=True, text=True)
    return clean(r, expect)


def same_as_rule(out, word0, dp, blks):
    lines = out.split("\n")
    count = int(lines[0].split()[1])
    assert count == len(blks) and [tuple(int(x) for x in l.split()) for l in lines[1: 1 + count]] == blks
    under = sum(int(((w & R.EXCLUDED) != 0).sum()) for w in word0)
    none = sum(int(((w & R.NO_ALLELE) != 0).sum()) for w in word0)
    assert lines[1 + count] == f"counts {under} {none}"
    conf = [np.array([int(x) for x in l.split()[1:]], np.uint32).reshape(-1, 2) for l in lines[2 + count:] if l.startswith("conf")]
    assert len(conf) == len(word0) and all(np.array_equal(c, R.conf_words(w, d)) for c, w, d in zip(conf, word0, dp))
    R.check_tiling(blks, word0)


SIXTEEN = tuple(range(3, 99, 6))


@pytest.mark.parametrize("size", [0, 1, 64, 257])
def test_host_rule_is_the_python_rule(checker, size):
    bases = references()
    recs = random_records(size, 300 + size, bases=bases)
    n, Q = G.cells(recs, REF_LENS)
    rng = np.random.default_rng(size)
    exclude = [(0, 0, 1), (1, 0, 1), (1, 5, 9), (1, 7, 30), (1, 30, 31), (len(REF_LENS) - 1, REF_LENS[-1] - 1, REF_LENS[-1])]
    exclude += [(int(r), int(p), min(int(p) + 1 + int(p) % 3, REF_LENS[r])) for r in rng.integers(0, len(REF_LENS), 50) for p in rng.integers(0, REF_LENS[r], 1)]
    for bands, ex in ((R.DEFAULT_BANDS, ()), ((), exclude), (SIXTEEN, exclude[::-1])):
        one = run_check(checker, recs, REF_LENS, bases, bands, ex)
        same_as_rule(one, *R.run(n, Q, bases, bands, ex))
        if size == 257:
            assert run_check(checker, recs, REF_LENS, bases, bands, ex, n_calls=5) == one     # however the records are cut
    if size == 257:
        blks = R.run(n, Q, bases)[2]
        assert len({b[3] for b in blks}) > 3 and any(b[2] - b[1] == 1 for b in blks)


def test_host_rule_on_the_edge_list(checker):
    from test_genotype import PARAM_SETS
    recs, bases = edge_records(), edge_bases()
    for pr in PARAM_SETS:
        n, Q = G.cells(recs, EDGE_REFS, **pr)
        same_as_rule(run_check(checker, recs, EDGE_REFS, bases, **pr), *R.run(n, Q, bases))
    n, Q = G.cells(recs, EDGE_REFS)
    odd = [(0, p, p + 1) for p in range(1, EDGE_REFS[0], 2)]
    same_as_rule(run_check(checker, recs, EDGE_REFS, bases, exclude=odd), *R.run(n, Q, bases, exclude=odd))
    whole = [(r, 0, length) for r, length in enumerate(EDGE_REFS)]
    assert run_check(checker, recs, EDGE_REFS, bases, exclude=whole).startswith("blocks 0\ncounts %d 0\n" % sum(EDGE_REFS))
    for bad_bands in ((0, 5), (5, 100), (5, 5), (9, 5), tuple(range(1, 18))):
        assert run_check(checker, recs, EDGE_REFS, bases, bands=bad_bands, expect=3).startswith("refused ")
    for bad in ((len(EDGE_REFS), 0, 1), (0, 5, 5), (0, 6, 5), (1, 0, EDGE_REFS[1] + 1)):
        assert run_check(checker, recs, EDGE_REFS, bases, exclude=[(0, 0, 1), bad], expect=3).startswith("refused ")


def test_gvcf_writer_is_the_python_text(checker):
    from test_genotype import sites_for
    d, exe = checker
    refs = [9000, 300]
    names = ["chr1", "chr 2"]
    bases = references(refs, 4)
    recs = random_records(400, 5, refs, bases)
    sites = sites_for(recs, refs, bases)
    for pr, min_qual, sample, bands in (({}, 20, "sample", R.DEFAULT_BANDS), (dict(prior=0, min_bq=0), 0, "a b", (50,))):
        n, Q, called = G.genotype(recs, refs, sites, **pr)
        variant_lines = G.vcf_lines(called, names, min_qual)
        exclude = R.excluded_by(variant_lines, names, refs)
        word0, dp, blks = R.run(n, Q, bases, bands, exclude)
        (d / "calls.bin").write_bytes(np.asarray(called, np.uint32).tobytes())
        (d / "blocks.bin").write_bytes(np.asarray(blks, np.uint32).tobytes())
        (d / "bases.bin").write_bytes(b"".join(bases))
        r = subprocess.run([exe, "gvcf", "calls.bin", "blocks.bin", "bases.bin", str(min_qual), sample, *[f"{n}:{l}" for n, l in zip(names, refs)]],
                           cwd=str(d), capture_output=True, text=True)
        text = clean(r)
        got_variants, got_blocks, body = R.split_gvcf(text, list(zip(names, refs)), sample)
        assert got_variants == variant_lines and len(variant_lines) > 5 and body == R.merged(variant_lines, blks, names, bases)
        assert r.stderr.strip() == R.summary_line(blks, word0)
        assert G.check_vcf_header("\n".join(R.vcf_header_of(text)) + "\n", list(zip(names, refs)), sample) == []


# ---- the oracle-backed tools ----
def gvcf_by_the_rule(d, tag, args, gvcf_text, bands=R.DEFAULT_BANDS, sample="sample", **params):
    """The body and the stderr line the rule gives for the records of the BAM file the run wrote, the FASTA file of its arguments
    and the variant lines of its own --gvcf file (whose positions are the excluded intervals)."""
    fasta = os.path.join(str(d), args[args.index("--genome") + 1])
    cut = int(args[args.index("--bucket-len") + 1]), int(args[args.index("-r") + 1])
    raw = gzip.decompress(open(d / f"{tag}.bam", "rb").read())
    refs = header_refs(raw)
    recs = [r for _, r in records_of(raw)[0]]
    names, lens = [n for n, _ in refs], [l for _, l in refs]
    bases = fasta_bases(fasta, refs, *cut)
    variants, block_lines, body = R.split_gvcf(gvcf_text, refs, sample)
    n, Q = G.cells(recs, lens, **params)
    word0, dp, blks = R.run(n, Q, bases, bands, R.excluded_by(variants, names, lens))
    R.check_tiling(blks, word0)
    assert body == R.merged(variants, blks, names, bases)
    # the file alone tiles every reference: the blocks by POS and END, the variant lines by POS and the length of REF
    for r, name in enumerate(names):
        covered = np.zeros(lens[r], np.int64)
        for l in block_lines:
            f = l.split("\t")
            if f[0] == name:
                covered[int(f[1]) - 1: int(f[7][4:])] += 1
        rest = np.frombuffer(bases[r], np.uint8) == ord("N")   # the excluded spans and the positions without a reference allele
        for a, b, c in R.excluded_by(variants, names, lens):
            if a == r:
                rest[b:c] = True
        assert (covered + rest == 1).all(), (name, np.flatnonzero(covered + rest != 1)[:10])
    return variants, blks, R.summary_line(blks, word0)


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_pileup import pileup_jobs
    return pileup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", range(3))
def test_oracle_tool_writes_what_the_rule_says(jobs, k):
    name, which, d, args, extra = jobs[k]
    exe = TOOLS[(which, "oracle")]
    aligned = name != "plain"                            # the plain tool writes no CIGAR: nothing is counted, every reference is band 0
    implied = ["--annotate"] if which == "bucketmap_align" else []
    run_tool(exe, d, args, f"{name}.bs.bam", [*extra, *implied, "--sort"])
    # alone
    err = run_tool(exe, d, args, f"{name}.b.bam", [*extra, "--gvcf", f"{name}.b.g.vcf"])
    assert re.search(r"Sorted \d+ records by coordinate in 1 run", err) and "Pileup:" not in err and err.index("Genotypes:") < err.index("Blocks:")
    assert pair_of(d, f"{name}.b") == pair_of(d, f"{name}.bs")                   # the BAM and its index are what they were
    assert not [f for f in os.listdir(d) if f.startswith(f"{name}.b.") and f not in (f"{name}.b.bam", f"{name}.b.bam.bai", f"{name}.b.g.vcf")]
    text = (d / f"{name}.b.g.vcf").read_text()
    variants, blks, told = gvcf_by_the_rule(d, f"{name}.b", args, text)
    assert blocks_line(err) == told
    if aligned:
        assert len(variants) > 3 and len({b[3] for b in blks}) > 2
    else:
        assert variants == [] and all(b[3:] == (0, 0, 0, 0, 0) for b in blks) and len(blks) >= 1
    # with --vcf: the two files' shared lines are equal, and the gVCF is what it was
    err = run_tool(exe, d, args, f"{name}.bv.bam", [*extra, "--gvcf", f"{name}.bv.g.vcf", "--vcf", f"{name}.bv.vcf"])
    assert (d / f"{name}.bv.g.vcf").read_text() == text and blocks_line(err) == told
    vcf = (d / f"{name}.bv.vcf").read_text()
    assert vcf.split("\n")[:-1] == R.vcf_header_of(text) + variants
    run_tool(exe, d, args, f"{name}.bv0.bam", [*extra, "--vcf", f"{name}.bv0.vcf"])
    assert (d / f"{name}.bv0.vcf").read_text() == vcf                            # --gvcf changes nothing in the file of --vcf
    # with the indel calls, realigned and left-aligned; other bands
    more = ["--affine", "--left-align"] if which == "bucketmap_align" else []
    opts = [*extra, *more, "--vcf-indels", "--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--gvcf-bands", "5,20"]
    err = run_tool(exe, d, args, f"{name}.bi.bam", [*opts, "--gvcf", f"{name}.bi.g.vcf", "--vcf", f"{name}.bi.vcf"])
    i_text = (d / f"{name}.bi.g.vcf").read_text()
    i_variants, i_blks, i_told = gvcf_by_the_rule(d, f"{name}.bi", args, i_text, bands=(5, 20))
    assert blocks_line(err) == i_told and (d / f"{name}.bi.vcf").read_text().split("\n")[:-1] == R.vcf_header_of(i_text) + i_variants
    assert not aligned or (any("INDEL" in l for l in i_variants) and any(len(l.split("\t")[3]) > 1 for l in i_variants) and {0, 1} <= {b[3] for b in i_blks} <= {0, 1, 2})
    # with --markdup the duplicates are left out; in several runs the same file
    err = run_tool(exe, d, args, f"{name}.bm.bam", [*extra, "--markdup", "--gvcf", f"{name}.bm.g.vcf"])
    m_text = (d / f"{name}.bm.g.vcf").read_text()
    assert blocks_line(err) == gvcf_by_the_rule(d, f"{name}.bm", args, m_text)[2] and (not aligned or m_text != text)
    err = run_tool(exe, d, args, f"{name}.br.bam", [*extra, "--gvcf", f"{name}.br.g.vcf"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1 and (d / f"{name}.br.g.vcf").read_text() == text and blocks_line(err) == told


# ---- the command line ----
def test_cli_refusals(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        run = lambda *opts: subprocess.run([exe, "-i", "idx", *opts], cwd=str(tmp_path), capture_output=True, text=True)
        fine = lambda r: "Validation failed" not in r.stderr and "Unknown option" not in r.stderr and "Value parse failed" not in r.stderr
        r = run("--gvcf", "g.vcf", "-o", "x.sam")
        assert r.returncode != 0 and "x.bam" in r.stderr and "--gvcf" in r.stderr and "only BAM output is sorted and indexed" in r.stderr, r.stderr
        r = run("--gvcf", "g.vcf")
        assert r.returncode != 0 and "-o x.bam" in r.stderr and "--gvcf" in r.stderr, r.stderr
        r = run("--gvcf")
        assert r.returncode != 0 and "Missing value" in r.stderr
        assert fine(run("-o", "x.bam", "--gvcf", "g.vcf")) and fine(run("-o", "x.bam", "--gvcf", "g.vcf", "--vcf", "v.vcf", "--pileup", "p.tsv", "--markdup"))
        for other in ("--vcf", "--pileup", "--depth", "--coverage"):
            r = run("-o", "x.bam", other, "same.txt", "--gvcf", "same.txt")
            assert r.returncode != 0 and "--gvcf" in r.stderr and other in r.stderr and "Validation failed" in r.stderr and "same.txt is the file of" in r.stderr
        # the options of --vcf and the pileup's thresholds: accepted with --gvcf alone, refused as before without either
        for opt, value in (("--vcf-prior", "20"), ("--vcf-min-qual", "30"), ("--vcf-sample", "NA12878"), ("--vcf-indels", None), ("--pileup-min-bq", "20"),
                           ("--pileup-min-alt", "3")):
            given = [opt] if value is None else [opt, value]
            assert fine(run("-o", "x.bam", "--gvcf", "g.vcf", *given))
            r = run("-o", "x.bam", *given)
            wording = "it is a threshold of --pileup FILE, which is not given." if opt.startswith("--pileup") else "it is an option of --vcf FILE, which is not given."
            assert r.returncode != 0 and opt in r.stderr and wording in r.stderr
        assert fine(run("-o", "x.bam", "--gvcf", "g.vcf", "--vcf-indels", "--vcf-indel-qual", "20"))
        r = run("-o", "x.bam", "--gvcf", "g.vcf", "--vcf-indel-qual", "20")
        assert r.returncode != 0 and "it is an option of --vcf-indels, which is not given." in r.stderr
        # the bands
        r = run("-o", "x.bam", "--gvcf-bands", "20,60")
        assert r.returncode != 0 and "--gvcf-bands" in r.stderr and "it is an option of --gvcf FILE, which is not given." in r.stderr
        r = run("-o", "x.bam", "--vcf", "v.vcf", "--gvcf-bands", "20,60")
        assert r.returncode != 0 and "--gvcf FILE" in r.stderr
        for good in ("20,60", "1", "99", ",".join(str(b) for b in SIXTEEN)):
            assert fine(run("-o", "x.bam", "--gvcf", "g.vcf", "--gvcf-bands", good)), good
        for bad in ("", "0", "100", "5,5", "9,5", "x", "5,", ",5", "5,,6", "-1", "1.5", ",".join(str(b) for b in range(1, 18))):
            r = run("-o", "x.bam", "--gvcf", "g.vcf", "--gvcf-bands", bad)
            assert r.returncode != 0 and "Value parse failed for --gvcf-bands" in r.stderr, (bad, r.stderr)
        r = run("-o", "x.bam", "--gvcf", "g.vcf", "--gvcf-bands")
        assert r.returncode != 0 and "Missing value" in r.stderr
        assert not os.listdir(tmp_path)


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import refblocks
    text = open(os.path.join(ROOT, "include", "bmr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(bmr_[a-z0-9_]+)\s*\(", code)))
    assert names == sorted(refblocks.SYMBOLS) and len(names) == 7
    L = refblocks.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    assert (refblocks.MAX_BANDS, refblocks.BLOCK_WORDS, refblocks.CONF_WORDS, refblocks.EXCLUDE_WORDS) == (16, 8, 2, 3)
    assert (refblocks.IN, refblocks.EXCLUDED, refblocks.NO_ALLELE) == (R.IN, R.EXCLUDED, R.NO_ALLELE) and refblocks.DEFAULT_BANDS == R.DEFAULT_BANDS
    for word in ("BMR_BLOCK_WORDS = 8", "BMR_MAX_BANDS = 16", "17 bytes per base", "LEFT OUT, on purpose", "<NON_REF> likelihoods", "PL in the blocks",
                 "a median DP", "a maximal block length", "strand and position bias", "several samples", "windows for genomes"):
        assert word in text, word
    # bmg.h is what it was: the reference blocks reach a bmg_ctx through an internal header, not through a new bmg_* symbol
    bmg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmg.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(bmg_[a-z0-9_]+)\s*\(", bmg))) == 8
    assert not [s for s in subprocess.run(["nm", "-D", "--defined-only", L._name], capture_output=True, text=True).stdout.split() if s.startswith("bmg_")
                and s not in ("bmg_last_error", "bmg_create", "bmg_destroy", "bmg_begin", "bmg_add", "bmg_call", "bmg_cells_at", "bmg_last_stats")]


def test_argument_errors_need_no_device():
    from bucket_map_amd import refblocks
    L = refblocks.lib()
    err = lambda: L.bmr_last_error().decode()
    count, out = C.c_uint64(0), np.zeros(8, np.uint32)
    ptrs = (C.c_void_p * 1)(None)
    assert L.bmr_create(0, None) == refblocks.BMR_ERR_ARG and "null argument" in err()
    assert L.bmr_run(None, None, ptrs, None, 0, None, 0, C.byref(count)) == refblocks.BMR_ERR_ARG and "bmr_run: null argument" in err()
    assert L.bmr_blocks(None, 0, 1, None) == refblocks.BMR_ERR_ARG and "null argument" in err()
    assert L.bmr_blocks(None, 0, 1, out.ctypes.data_as(refblocks._u32p)) == refblocks.BMR_ERR_ARG and "null context" in err()
    assert L.bmr_conf_at(None, 0, 0, 1, None) == refblocks.BMR_ERR_ARG and "null argument" in err()
    assert L.bmr_conf_at(None, 0, 0, 1, out.ctypes.data_as(refblocks._u32p)) == refblocks.BMR_ERR_ARG and "null context" in err()
    assert L.bmr_last_stats(None, None, None) == refblocks.BMR_ERR_ARG
    L.bmr_destroy(None)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import refblocks
    with pytest.raises(refblocks.BmrError) as e:
        refblocks.RefBlocks(0)
    assert e.value.code == refblocks.BMR_ERR_HIP
