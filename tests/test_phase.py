"""Read-backed phasing (--vcf FILE --vcf-phase) without a GPU: the rule on cases worked out by hand, on two planted haplotypes
and against host/phase.h as a program of its own under ASan + UBSan, the writer, the sorter's second pass in one run and in
several, with and without --markdup, through the oracle-backed tools (whose phasing is the host default of block_compressor),
the command line and the bmk_* ABI surface.

The yardstick is the rule of include/bmk.h in plain Python (tests/phase_rule.py)."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import genotype_rule as G
import phase_rule as K
import pileup_rule as P
from phase_cases import DESIGNED, chain, het, hom, no_variant, planted_calls, reads_over
from pileup_cases import EDGE_REFS, REF_LENS, edge_records, many_ops_record, random_records, rec_letters, references
from test_bamsort import offsets_of, pair_of, records_of, run_tool
from test_bias import variant_lines
from test_depth import full_record, header_refs
from test_genotype import genotypes_line, sites_for
from test_pileup import fasta_bases
from test_sam_golden import ROOT, TOOLS

PHASE = re.compile(r"Phase: (\d+) of (\d+) het SNVs phased in (\d+) blocks \(longest (\d+) bases, (\d+) observations\)")
STRICT = dict(min_mapq=20, min_bq=14)


# ---- two planted haplotypes ----
def two_haplotypes(seed=5, n=3000, read=100, step=5):
    """(records, reference bases, het positions, which haplotype carries the alternative letter, the letters): error-free reads
    of `read` bases every `step` bases, alternately from either haplotype."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, n)
    at, p = [], 150
    while p < n - 150:
        at.append(p)
        p += int(rng.integers(20, 61)) if len(at) % 9 else int(rng.integers(read + 1, read + 40))   # every ninth gap is wider than a read
    alt = {p: int((ref[p] + 1 + rng.integers(0, 3)) % 4) for p in at}
    on = {p: int(rng.integers(0, 2)) for p in at}        # the haplotype with the alternative letter
    haps = [ref.copy(), ref.copy()]
    for p in at:
        haps[on[p]][p] = alt[p]
    recs = [rec_letters(0, s, f"{read}M", "".join("ACGT"[x] for x in haps[k % 2][s: s + read]), name=b"h%d" % k, flag=16 * (k // 2 % 2))
            for k, s in enumerate(range(0, n - read + 1, step))]
    return recs, bytes(b"ACGT"[x] for x in ref), at, on, alt


def truth_case(rule):
    """The engine `rule` (as phase_cases' designed cases take it) on two planted haplotypes: every block equals the planted phase
    up to one flip, and there are as many blocks as connected runs of spanned sites."""
    recs, bases, at, on, alt = two_haplotypes()
    sites = sites_for(recs, [len(bases)], [bases])
    called = G.genotype(recs, [len(bases)], sites)[2]
    hets = [c for c in called if c[3] & G.VARIANT and c[4] != c[5]]
    assert [c[1] for c in hets] == at and len(at) > 50   # the existing genotype rule calls every planted het, and nothing else
    # the condition, from the reads and the Python rule alone: every neighbouring pair inside a run is spanned by >= min_links
    # reads of either haplotype, no read spans a wide gap, and error-free reads make every counter of a link all cis or all trans
    spans = lambda a, b: sum(1 for r in recs if K.fields(r)[1] <= a and b < K.fields(r)[1] + 100)
    spanned = [spans(a, b) for a, b in zip(at, at[1:])]
    assert all(s == 0 or s >= 2 * K.DEFAULTS["min_links"] for s in spanned) and spanned.count(0) >= 5
    for cell in K.run(recs, [len(bases)], called)[1].reshape(-1, 4).tolist():
        assert (cell[0] + cell[3] == 0) or (cell[1] + cell[2] == 0)
    link, words, sums = rule(recs, called, ref_len=(len(bases),))
    runs = 1 + spanned.count(0)
    assert sums[:3] == [len(at), len(at), runs]          # as many blocks as connected runs of spanned sites, every site in one
    run_of = np.concatenate([[0], np.cumsum(np.asarray(spanned) == 0)]).tolist()
    roots = [w[K.W_ROOT] for w in words]
    assert [roots.index(r) for r in roots] == [run_of.index(x) for x in run_of]      # the blocks are the runs
    # haplotype 1 carries allele hap(j): equal to the planted haplotypes up to one flip per block
    letter_h1 = [(c[4], c[5])[w[K.W_HAP]] for c, w in zip(hets, words)]
    planted0 = [alt[p] if on[p] == 0 else int("ACGT".index(chr(bases[p]))) for p in at]
    agrees = [int(a == b) for a, b in zip(letter_h1, planted0)]
    for r in set(roots):
        assert len({agrees[j] for j in range(len(at)) if roots[j] == r}) == 1


# ---- host/phase.h as a program of its own ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("phase_check")
    exe = str(d / "phase_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "phase_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def clean(r, expect=0):
    """expect None: the program may refuse (3) or not (0)."""
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode in ((0, 3) if expect is None else (expect,)), r.stderr[-3000:]
    return r.stdout


def run_check(checker, recs, ref_len, called, n_adds=1, seed=0, skip=None, expect=0, **params):
    d, exe = checker
    pr = {**K.DEFAULTS, **params}
    (d / "records.bin").write_bytes(b"".join(recs))
    (d / "calls.bin").write_bytes(np.asarray(called, np.uint32).tobytes())
    if skip is not None:
        (d / "skip.bin").write_bytes(bytes(skip))
    r = subprocess.run([exe, "records.bin", "skip.bin" if skip is not None else "-", "calls.bin", str(n_adds), str(seed),
                        *[str(pr[k]) for k in ("min_mapq", "min_bq", "min_links", "min_frac_ppm", "reach")], *[str(x) for x in ref_len]],
                       cwd=str(d), capture_output=True, text=True)
    return clean(r, expect)


def same_as_rule(out, want):
    sites, link, words, sums = want
    lines = out.split("\n")
    H = int(lines[0].split()[1])
    assert H == len(sites) and [tuple(int(x) for x in l.split()) for l in lines[1: 1 + H]] == words
    assert lines[1 + H].split() == ["stats", *[str(x) for x in sums]] and lines[2 + H] == "links"
    got = [[int(x) for x in l.split()] for l in lines[3 + H: 3 + 2 * H]]
    assert got == link.reshape(H, -1).tolist()


def parsed(out):
    """(link, words, sums) of the checker's output."""
    lines = out.split("\n")
    H = int(lines[0].split()[1])
    words = [tuple(int(x) for x in l.split()) for l in lines[1: 1 + H]]
    sums = [int(x) for x in lines[1 + H].split()[1:]]
    link = np.array([[int(x) for x in l.split()] for l in lines[3 + H: 3 + 2 * H]], np.int64).reshape(H, -1, 4)
    return link, words, sums


def host_rule(checker):
    """host/phase.h as the engine of the designed cases: what it prints, after it has been compared with the Python rule too."""
    def rule(reads, calls, ref_len=(16,), **params):
        out = run_check(checker, reads, list(ref_len), calls, expect=None, **params)
        if out.startswith("refused"):
            with pytest.raises(K.Refused):               # ... and the Python rule refuses the same
                K.run(reads, list(ref_len), calls, **params)
            raise K.Refused(out)
        same_as_rule(out, K.run(reads, list(ref_len), calls, **params))
        return parsed(out)
    return rule


@pytest.mark.parametrize("case", DESIGNED, ids=lambda f: f.__name__[5:])
def test_host_rule_on_the_designed_cases(checker, case):
    case(host_rule(checker))


def test_host_rule_truth_two_planted_haplotypes(checker):
    truth_case(host_rule(checker))


@pytest.fixture(scope="module")
def ref_bases():
    return references()


@pytest.mark.parametrize("size", [0, 1, 65, 1025, 8001])
def test_host_rule_is_the_python_rule(checker, ref_bases, size):
    recs = random_records(size, 300 + size, bases=ref_bases)
    called = planted_calls(REF_LENS, ref_bases, 7 + size)
    want = K.run(recs, REF_LENS, called)
    one = run_check(checker, recs, REF_LENS, called)
    same_as_rule(one, want)
    if size >= 1025:
        flags = [w[K.W_FLAGS] for w in want[2]]
        assert flags.count(K.PHASED) > 20 and flags.count(K.ROOT) > 20 and flags.count(K.PHASED | K.ROOT) > 5 and want[3][3] > 2000
        assert len({w[K.W_D] for w in want[2]}) >= 4 and {w[K.W_HAP] for w in want[2]} == {0, 1}
    if size in (65, 1025):                               # order and cutting do not matter; other parameters
        assert run_check(checker, recs, REF_LENS, called, n_adds=3, seed=1 + size) == one
        assert run_check(checker, recs, REF_LENS, called, n_adds=7, seed=size) == one
        for pr in (STRICT, dict(min_bq=0, reach=1, min_links=1), dict(reach=8, min_frac_ppm=1000000), dict(min_bq=256, min_mapq=200, min_frac_ppm=500001)):
            same_as_rule(run_check(checker, recs, REF_LENS, called, **pr), K.run(recs, REF_LENS, called, **pr))
        skip = [int(k % 3 == 1) for k in range(size)]
        same_as_rule(run_check(checker, recs, REF_LENS, called, skip=skip), K.run(recs, REF_LENS, called, skip))


def edge_calls():
    """Sites over pileup_cases.edge_records: every base of the stretches its designed records lie on, of 2 alternating kinds."""
    spots = [(0, p) for p in [*range(0, 12), *range(96, 110), *range(598, 712)]] + [(1, p) for p in range(40, 50)] + [(2, 0)]
    return [het(r, p, p % 4, (p + 1 + r) % 4) if (p + r) % 5 else het(r, p, (p + 2) % 4, p % 4) for r, p in spots]


def test_host_rule_on_the_edges_designed_cases_and_a_record_of_many_ops(checker):
    recs = edge_records()
    for pr in ({}, STRICT, dict(min_bq=0, reach=8), dict(min_bq=256, min_mapq=31, reach=1)):
        want = K.run(recs, EDGE_REFS, edge_calls(), **pr)
        same_as_rule(run_check(checker, recs, EDGE_REFS, edge_calls(), **pr), want)
    assert sum(1 for w in K.run(recs, EDGE_REFS, edge_calls())[2] if w[K.W_FLAGS] & K.PHASED) > 10
    calls = [het(0, 0), het(0, 1), het(0, 2)]
    reads = reads_over([("AAA", 2), ("ACA", 2), ("CAC", 2), ("CCC", 2)])
    same_as_rule(run_check(checker, reads, [16], calls), K.run(reads, [16], calls))
    for H in (2, 65, 300):
        for bridged in (False, True):
            recs, ref_len, calls, haps = chain(H, H, bridged)
            want = K.run(recs, ref_len, calls)
            assert want[3][:3] == [H, H, 1] and [w[K.W_HAP] ^ haps[0] for w in want[2]] == haps
            assert not bridged or H == 2 or {w[K.W_D] for w in want[2]} == {0, 1, 2}
            same_as_rule(run_check(checker, recs, ref_len, calls, n_adds=2), want)
    refs = [90000, 300]
    bases = references(refs, 4)
    recs = random_records(100, 5, refs, bases) + [many_ops_record(0, 17)] + [many_ops_record(0, 0, 60001, seed=8)]
    called = planted_calls(refs, bases, 3, gap=40)
    want = K.run(recs, refs, called)
    assert want[3][3] > 1000
    same_as_rule(run_check(checker, recs, refs, called), want)


def test_host_rule_refuses_what_the_abi_refuses(checker):
    refs = [100, 50]
    recs = random_records(20, 9, refs, references(refs, 2))
    ok = [het(0, 3), het(0, 9), het(1, 49)]
    assert run_check(checker, recs, refs, ok).startswith("sites 3\n")
    for pr in (dict(reach=0), dict(reach=9), dict(min_links=0), dict(min_frac_ppm=500000), dict(min_frac_ppm=1000001)):
        assert run_check(checker, recs, refs, ok, expect=3, **pr).startswith("refused")
    for bad in ([het(2, 0)], [het(0, 100)], [het(1, 50)], [het(0, 1, 4, 0)], [het(0, 1, 0, 5)], [het(0, 9), het(0, 3)], [het(1, 0), het(0, 5)], [het(0, 4), het(0, 4)]):
        assert run_check(checker, recs, refs, bad, expect=3).startswith("refused"), bad
    assert run_check(checker, recs, refs, [hom(9, 9, 7), no_variant(50, 1), het(0, 2)]).startswith("sites 1\n")   # what is no phase site is not looked at
    assert run_check(checker, recs, [5, 0], [het(0, 3)], expect=3).startswith("refused")
    from test_markdup_gpu import rec, rec_ops
    for stream in ([rec_ops(0, 0, 0, [3 << 4 | 9], b"")], [rec(0, 5, 0, "3M", b"ab")], [rec(2, 5, 0, "3M", b"")]):
        assert run_check(checker, stream, refs, ok, expect=3).startswith("refused")


# ---- the writer ----
def write_vcf(checker, called, words, n_obs, names_lens, notes=None, min_qual=20):
    d, exe = checker
    (d / "calls.bin").write_bytes(np.asarray(called, np.uint32).tobytes())
    if words is not None:
        (d / "sites.bin").write_bytes(np.asarray(words, np.uint32).tobytes())
    if notes is not None:
        (d / "notes.bin").write_bytes(np.asarray(notes, np.uint32).tobytes())
    r = subprocess.run([exe, "vcf", "calls.bin", "sites.bin" if words is not None else "-", "notes.bin" if notes is not None else "-", str(n_obs), str(min_qual), "sample",
                        *[f"{n}:{l}" for n, l in names_lens]], cwd=str(d), capture_output=True, text=True)
    return clean(r), r.stderr


def test_vcf_writer_is_the_python_text(checker):
    recs, bases, at, on, alt = two_haplotypes(seed=6, n=1500)
    recs += [rec_letters(0, at[3] - 2, "5M", "TTTTT", name=b"third%d" % k) for k in range(9)]     # a third letter: some 1/2 or R/alt mixes
    sites = sites_for(recs, [len(bases)], [bases])
    called = G.genotype(recs, [len(bases)], sites)[2]
    psites, link, words, sums = K.run(recs, [len(bases)], called)
    names = [("chr one", len(bases))]
    plain, _ = write_vcf(checker, called, None, 0, names)
    assert G.check_vcf_header(plain, names) == G.vcf_lines(called, ["chr one"])          # without the phase: the file of --vcf
    text, err = write_vcf(checker, called, words, sums[3], names)
    K.same_as_phased(text, K.phased_vcf(plain, called, words))
    assert K.unphased_vcf(text) == plain and text != plain and text.count("|") == sums[1] > 10 and text.count(":PS\t") == sums[1]
    assert err.strip() == K.summary_line(words, sums, called)
    # an unphased het, a root of one site, keeps its line byte for byte
    lone = [w if w[K.W_ROOT] != words[5][K.W_ROOT] else (*w[:4], w[4] & ~K.PHASED, *w[5:]) for w in words]
    text_lone, _ = write_vcf(checker, called, lone, sums[3], names)
    assert K.unphased_vcf(text_lone) == plain and text_lone.count("|") < sums[1]
    K.same_as_phased(text_lone, K.phased_vcf(plain, called, lone))
    # with the annotations of --vcf-bias the keys end GT:DP:AD:ADF:ADR:GQ:PL:PS
    notes = [(1, 2, 3, 4, 5, 6, 7, 8, 3000, 123, 1, 9, 1, 2, 3, 4) if c[3] & G.VARIANT else (0,) * 16 for c in called]
    d, exe = checker
    both, _ = write_vcf(checker, called, words, sums[3], names, notes)
    assert both.count("GT:DP:AD:ADF:ADR:GQ:PL:PS\t") == sums[1]
    none, _ = write_vcf(checker, called, None, 0, names, notes)
    empty, _ = write_vcf(checker, called, [], 0, names, notes)                            # the option given and nothing phased: the header line only
    assert K.unphased_vcf(empty) == none and empty.count("\n") == none.count("\n") + 1
    assert K.unphased_vcf(both) == none


# ---- the oracle-backed tools ----
HETS = (15000, 15020, 15045, 15300, 15330)


def planted_haplotypes(d):
    """Single reads on the paired fixture's genome, in unique sequence of chrA: two haplotypes with five hets, the first three
    within a read of each other, then 255 bases further the other two.  150-base reads every 6 bases, alternately from either
    haplotype, every other two from the reverse strand; every fourth read stands twice (a duplicate for --markdup)."""
    from test_pair import ARGS as PAIR_ARGS, COMP, make_paired_fixture
    make_paired_fixture(d)
    a = (d / "g.fa").read_text().split("\n")[1].encode()
    haps = [bytearray(a), bytearray(a)]
    for k, p in enumerate(HETS):
        haps[k % 2][p] = b"ACGTA"[b"ACGT".index(a[p]) + 1]
    with open(d / "hap.fastq", "w") as f:
        for k, m in enumerate(range(14860, 15340, 6)):
            s = bytes(haps[k % 2][m: m + 150])
            if k // 2 % 2:
                s = s.translate(COMP)[::-1]
            for copy in range(2 if k % 4 == 0 else 1):
                f.write(f"@h{k}_{copy}\n{s.decode()}\n+\n{'I' * 150}\n")
    return [*PAIR_ARGS, "-q", "hap.fastq"], []


def phase_by_the_rule(bam_path, args, pile_th=None, phase_pr=None, **params):
    """(the calls, the words of the sites, the four sums, the Phase line on stderr) for the records of a BAM file."""
    fasta = os.path.join(os.path.dirname(bam_path), args[args.index("--genome") + 1])
    cut = int(args[args.index("--bucket-len") + 1]), int(args[args.index("-r") + 1])
    raw = gzip.decompress(open(bam_path, "rb").read())
    refs = header_refs(raw)
    recs = [r for _, r in records_of(raw)[0]]
    lens = [l for _, l in refs]
    pile_th = {**P.DEFAULTS, **(pile_th or {})}
    res = P.pile(recs, lens, fasta_bases(fasta, refs, *cut), **pile_th)
    th = dict(min_mapq=pile_th["min_mapq"], min_bq=pile_th["min_bq"])
    called = G.genotype(recs, lens, res.sites, **th, **params)[2]
    _, _, words, sums = K.run(recs, lens, called, **th, **(phase_pr or {}))
    return called, words, sums, K.summary_line(words, sums, called)


def phase_line(err):
    found = [l.split("\t")[-1] for l in err.split("\n") if "Phase:" in l]
    assert len(found) == 1 and PHASE.fullmatch(found[0]), err
    return found[0]


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("phase_tools")
    args, extra = planted_haplotypes(d)
    return d, args, extra


@pytest.mark.parametrize("which", ["bucketmap_align", "bucketmap"])
def test_oracle_tool_writes_what_the_rule_says(planted, which):
    d, args, extra = planted
    exe = TOOLS[(which, "oracle")]
    err0 = run_tool(exe, d, args, f"{which}.p0.bam", [*extra, "--vcf", f"{which}.p0.vcf"])
    plain = (d / f"{which}.p0.vcf").read_text()
    assert "Phase:" not in err0 and "|" not in plain and "PS" not in plain
    err = run_tool(exe, d, args, f"{which}.p.bam", [*extra, "--vcf", f"{which}.p.vcf", "--vcf-phase"])
    assert pair_of(d, f"{which}.p") == pair_of(d, f"{which}.p0") and genotypes_line(err) == genotypes_line(err0)
    called, words, sums, told = phase_by_the_rule(d / f"{which}.p.bam", args)
    text = (d / f"{which}.p.vcf").read_text()
    K.same_as_phased(text, K.phased_vcf(plain, called, words))
    assert K.unphased_vcf(text) == plain and phase_line(err) == told
    if which == "bucketmap":                             # no CIGAR, no calls: nothing is phased
        assert told == "Phase: 0 of 0 het SNVs phased in 0 blocks (longest 0 bases, 0 observations)" and text.replace(K.PS_HEAD, "").count("PS") == 0
        return
    assert told.startswith("Phase: 5 of 5 het SNVs phased in 2 blocks (longest 46 bases, ")
    by_pos = {int(l.split("\t")[1]): l.split("\t") for l in variant_lines(text)}
    assert [by_pos[p + 1][9].split(":")[-1] for p in HETS] == ["15001"] * 3 + ["15301"] * 2 and all(by_pos[p + 1][8] == "GT:DP:AD:GQ:PL:PS" for p in HETS)
    g = [by_pos[p + 1][9][:3] for p in HETS]             # the alternative letters lie on alternating haplotypes
    assert set(g) == {"0|1", "1|0"} and g[0] == g[2] != g[1] and g[3] != g[4]
    # other parameters: no link of three observations at --phase-min-links above the depth, the first block at reach 1
    err = run_tool(exe, d, args, "pl.bam", [*extra, "--vcf", "pl.vcf", "--vcf-phase", "--phase-min-links", "40", "--phase-reach=1", "--phase-min-frac", "0.999999"])
    _, w2, s2, told2 = phase_by_the_rule(d / "pl.bam", args, phase_pr=dict(min_links=40, reach=1, min_frac_ppm=999999))
    assert phase_line(err) == told2 and told2.startswith("Phase: 0 of 5 ") and K.unphased_vcf((d / "pl.vcf").read_text()) == plain
    assert (d / "pl.vcf").read_text().count("|") == 0 and K.PS_HEAD in (d / "pl.vcf").read_text()
    # the option mixes: every file without --vcf-phase is the phased one with the phase taken out
    for tag, opts in (("gi", ["--gvcf", "x.g.vcf", "--vcf-indels"]), ("b", ["--vcf-bias"]), ("gb", ["--gvcf", "x.g.vcf", "--vcf-bias", "--vcf-indels"])):
        opts = [o.replace("x.g.vcf", f"{tag}.g.vcf") for o in opts]
        run_tool(exe, d, args, f"{tag}0.bam", [*extra, "--vcf", f"{tag}0.vcf", *[o.replace(f"{tag}.g", f"{tag}0.g") for o in opts]])
        err = run_tool(exe, d, args, f"{tag}.bam", [*extra, "--vcf", f"{tag}.vcf", *opts, "--vcf-phase"])
        assert phase_line(err) == told
        with_phase = (d / f"{tag}.vcf").read_text()
        assert K.unphased_vcf(with_phase) == (d / f"{tag}0.vcf").read_text() and with_phase.count("|") == 5
        assert ("GT:DP:AD:ADF:ADR:GQ:PL:PS\t" in with_phase) == ("--vcf-bias" in opts)
        if "--gvcf" in opts:
            g_text = (d / f"{tag}.g.vcf").read_text()
            assert K.unphased_vcf(g_text) == (d / f"{tag}0.g.vcf").read_text() and variant_lines(g_text) == variant_lines(with_phase)
            assert g_text.split("\n").index(next(l for l in g_text.split("\n") if l.startswith(K.PS_HEAD))) == \
                   1 + g_text.split("\n").index(next(l for l in g_text.split("\n") if l.startswith("##FORMAT=<ID=PL,")))
            err = run_tool(exe, d, args, f"{tag}o.bam", [*extra, "--gvcf", f"{tag}o.g.vcf", *opts[2:], "--vcf-phase"])
            assert (d / f"{tag}o.g.vcf").read_text() == g_text and phase_line(err) == told      # --gvcf alone


def test_sorter_one_run_and_several_with_and_without_markdup(planted):
    d, args, extra = planted
    exe = TOOLS[("bucketmap_align", "oracle")]
    seen = {}
    for mark in ([], ["--markdup"]):
        tag = "m" if mark else "u"
        err1 = run_tool(exe, d, args, f"s{tag}1.bam", [*extra, *mark, "--vcf", f"s{tag}1.vcf", "--vcf-phase"])
        errn = run_tool(exe, d, args, f"s{tag}n.bam", [*extra, *mark, "--vcf", f"s{tag}n.vcf", "--vcf-phase"], env=dict(BM_SORT_RUN_BYTES="2000"))
        assert "in 1 run" in err1 and int(re.search(r"in (\d+) run", errn).group(1)) > 3
        assert pair_of(d, f"s{tag}1") == pair_of(d, f"s{tag}n") and (d / f"s{tag}1.vcf").read_text() == (d / f"s{tag}n.vcf").read_text()
        called, words, sums, told = phase_by_the_rule(d / f"s{tag}1.bam", args)
        assert phase_line(err1) == phase_line(errn) == told
        seen[tag] = sums[3]
    # a duplicate record gives no observation and no link: the records of the marked file carry 0x400
    raw = gzip.decompress((d / "sm1.bam").read_bytes())
    dups = sum(1 for _, r in records_of(raw)[0] if r[19] & 4)
    assert dups >= 15 and seen["u"] - seen["m"] > dups and seen["m"] > 100


@pytest.mark.parametrize("k", range(3))
def test_oracle_tool_on_the_pileup_jobs(tmp_path_factory, k):
    from test_pileup import pileup_jobs
    name, which, d, args, extra = pileup_jobs(tmp_path_factory)[k]
    exe = TOOLS[(which, "oracle")]
    loose = ["--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--pileup-min-bq", "0", "--vcf-prior", "0"]
    run_tool(exe, d, args, f"{name}.k0.bam", [*extra, *loose, "--vcf", f"{name}.k0.vcf"])
    err = run_tool(exe, d, args, f"{name}.k.bam", [*extra, *loose, "--vcf", f"{name}.k.vcf", "--vcf-phase", "--phase-min-links", "1"])
    errn = run_tool(exe, d, args, f"{name}.kn.bam", [*extra, *loose, "--vcf", f"{name}.kn.vcf", "--vcf-phase", "--phase-min-links", "1"], env=dict(BM_SORT_RUN_BYTES="2000"))
    called, words, sums, told = phase_by_the_rule(d / f"{name}.k.bam", args, pile_th=dict(min_bq=0, min_alt=1, min_frac_ppm=1), phase_pr=dict(min_links=1), prior=0)
    text = (d / f"{name}.k.vcf").read_text()
    K.same_as_phased(text, K.phased_vcf((d / f"{name}.k0.vcf").read_text(), called, words))
    assert phase_line(err) == phase_line(errn) == told and (d / f"{name}.kn.vcf").read_text() == text


# ---- the command line ----
def test_cli_refusals(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        run = lambda *opts: subprocess.run([exe, "-i", "idx", *opts], cwd=str(tmp_path), capture_output=True, text=True)
        fine = lambda r: "Validation failed" not in r.stderr and "Unknown option" not in r.stderr and "Value parse failed" not in r.stderr
        r = run("-o", "x.bam", "--vcf-phase")
        assert r.returncode != 0 and "Validation failed for option --vcf-phase" in r.stderr and "--vcf FILE" in r.stderr and "--gvcf FILE" in r.stderr, r.stderr
        r = run("-o", "x.bam", "--pileup", "p.tsv", "--vcf-phase")
        assert r.returncode != 0 and "Validation failed for option --vcf-phase" in r.stderr
        assert fine(run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-phase")) and fine(run("-o", "x.bam", "--gvcf", "g.vcf", "--vcf-phase"))
        assert fine(run("-o", "x.bam", "--vcf", "v.vcf", "--gvcf", "g.vcf", "--vcf-indels", "--vcf-bias", "--markdup", "--pileup", "p.tsv", "--depth", "d.txt", "--vcf-phase"))
        for opt, value in (("--phase-min-links", "3"), ("--phase-min-frac", "0.9"), ("--phase-reach", "8")):
            r = run("-o", "x.bam", "--vcf", "v.vcf", opt, value)                  # an option of --vcf-phase without it
            assert r.returncode != 0 and "Validation failed for option " + opt in r.stderr and "--vcf-phase" in r.stderr, r.stderr
            assert fine(run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-phase", opt, value)) and fine(run("-o", "x.bam", opt + "=" + value, "--gvcf", "g.vcf", "--vcf-phase"))
            r = run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-phase", opt)
            assert r.returncode != 0 and "Missing value" in r.stderr
        bads = (("--phase-min-links", ("x", "-1", "", "0", "1.5", "4294967296")), ("--phase-reach", ("x", "-1", "", "0", "9", "2e0")),
                ("--phase-min-frac", ("x", "-1", "", "0.5", "0", "1.1", "0.5000001", "2", "8e-1")))
        for opt, values in bads:
            for bad in values:
                r = run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-phase", opt, bad)
                assert r.returncode != 0 and "Value parse failed for " + opt in r.stderr, (opt, bad, r.stderr)
        for opt, goods in (("--phase-min-links", ("1", "4294967295")), ("--phase-reach", ("1", "8")), ("--phase-min-frac", ("0.500001", "1", "1.000000", "0.8"))):
            assert all(fine(run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-phase", opt, good)) for good in goods)
        assert not os.listdir(tmp_path)


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import phase
    header = open(os.path.join(ROOT, "include", "bmk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = sorted(set(re.findall(r"\b(bmk_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(phase.SYMBOLS) and len(names) == 9
    assert not re.search(r"\bbmf_", text)
    L = phase.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    assert (phase.CALL_WORDS, phase.OUT_WORDS, phase.N_STATS, phase.MAX_REACH) == (24, K.OUT_WORDS, K.N_STATS, K.MAX_REACH) and phase.DEFAULTS == K.DEFAULTS
    assert (phase.PHASED, phase.ROOT) == (K.PHASED, K.ROOT) and tuple(phase.PARAMS) == tuple(K.DEFAULTS)
    assert (phase.W_CALL, phase.W_ROOT, phase.W_ROOT_POS, phase.W_HAP, phase.W_FLAGS, phase.W_D, phase.W_CIS, phase.W_TRANS) == tuple(range(8))
    for word in ("BMK_OUT_WORDS = 8", "BMK_N_PARAMS = 5", "BMK_N_STATS = 4", "LEFT OUT, on purpose", "across the two mates", "indel calls as phase sites", "hom\n * sites",
                 "HP/PS tags", "MEC", "phase quality", "trios"):
        assert word in header, word


def test_argument_errors_need_no_device():
    from bucket_map_amd import phase
    L = phase.lib()
    u8p, u32p, u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64))
    err = lambda: L.bmk_last_error().decode()
    recs = [full_record(ops=[4 << 4]), full_record(3, 2, 7, 5, ops=[3 << 4 | 4, 4 << 4 | 7])]
    good, good_off = b"".join(recs), offsets_of(recs)
    lying = bytearray(good)
    lying[0] += 1
    cases = {                                            # bmp_add's checks, in its order
        "first offset": (good, [1, good_off[1], good_off[2]], 2, "rec_offset[0]"),
        "descending": (good, [0, good_off[2], good_off[1]], 2, "ascending"),
        "last offset": (good, [0, good_off[1]], 1, "the stream has"),
        "block_size": (bytes(lying), good_off, 2, "block_size"),
        "too many": (good, good_off, 2 ** 31, "2^31"),
        "op code": (recs[0] + full_record(ops=[4 << 4 | 9]), offsets_of([recs[0]] * 2), 2, "a CIGAR op is 0 .. 8"),
        "query short": (full_record(ops=[3 << 4]), offsets_of([recs[0]]), 1, "query bases"),
    }

    def add(stream, off, n, null=()):
        a, o = np.frombuffer(stream, np.uint8), np.asarray(off, np.uint64)
        p = dict(a=a.ctypes.data_as(u8p), o=o.ctypes.data_as(u64p))
        for k in null:
            p[k] = None
        return L.bmk_add(None, p["a"], len(stream), p["o"], n, None)

    for name, (stream, off, n, word) in cases.items():
        assert add(stream, off, n) == phase.BMK_ERR_ARG, name
        assert word in err() and "bmk_add" in err(), (name, err())
    for null in ("a", "o"):
        assert add(good, good_off, 2, null=(null,)) == phase.BMK_ERR_ARG and "null argument" in err()
    assert add(good, good_off, 2) == phase.BMK_ERR_ARG and "null context" in err()
    assert add(b"", [0], 0) == phase.BMK_ERR_ARG and "null context" in err()

    def begin(lens, calls, n=None, null=(), **params):
        a, t = np.asarray(lens, np.uint32), np.array([{**K.DEFAULTS, **params}[k] for k in phase.PARAMS], np.uint32)
        c = np.asarray(calls, np.uint32).reshape(-1, 24)
        p = dict(lens=a.ctypes.data_as(u32p), pr=t.ctypes.data_as(u32p), calls=c.ctypes.data_as(u32p))
        for k in null:
            p[k] = None
        return L.bmk_begin(None, p["lens"], len(lens) if n is None else n, p["pr"], p["calls"], c.shape[0], None)

    ok = [het(0, 1), het(0, 3)]
    assert begin([5], ok, n=0) == phase.BMK_ERR_ARG and "n_ref is 0" in err()
    assert begin([5, 0, 7], ok) == phase.BMK_ERR_ARG and "reference 1 has the length 0" in err()
    assert begin([2 ** 32 - 2 ** 20, 1], ok) == phase.BMK_ERR_ARG and "2^32 - 2^20" in err()
    for null in ("lens", "pr", "calls"):
        assert begin([5], ok, null=(null,)) == phase.BMK_ERR_ARG and "null argument" in err()
    for bad, word in ((dict(reach=0), "reach"), (dict(reach=9), "reach"), (dict(min_links=0), "min_links"), (dict(min_frac_ppm=500000), "min_frac_ppm"),
                      (dict(min_frac_ppm=1000001), "min_frac_ppm")):
        assert begin([5], ok, **bad) == phase.BMK_ERR_ARG and word in err()
    for bad, word in (([het(1, 0)], "names reference 1"), ([het(0, 5)], "lies at base 5"), ([het(0, 1, 4, 0)], "letters"), ([het(0, 1, 0, 4)], "letters"),
                      ([het(0, 3), het(0, 1)], "ascend"), ([het(0, 3), het(0, 3)], "ascend")):
        assert begin([5], bad) == phase.BMK_ERR_ARG and word in err(), (bad, err())
    assert begin([5, 9], [het(1, 0), het(0, 4)]) == phase.BMK_ERR_ARG and "ascend" in err()
    assert begin([5], ok) == phase.BMK_ERR_ARG and "null context" in err()               # good data: only the context is missing
    assert begin([5], [hom(7, 7, 9), no_variant(9, 9)]) == phase.BMK_ERR_ARG and "null context" in err()
    assert begin([5], []) == phase.BMK_ERR_ARG and "null context" in err()
    out = np.zeros(64, np.uint32)
    assert L.bmk_phase(None, 0, 1, None) == phase.BMK_ERR_ARG and "null argument" in err()
    assert L.bmk_links(None, 0, 1, None) == phase.BMK_ERR_ARG and "null argument" in err()
    assert L.bmk_phase(None, 0, 1, out.ctypes.data_as(u32p)) == phase.BMK_ERR_ARG and "null context" in err()
    assert L.bmk_links(None, 0, 0, None) == phase.BMK_ERR_ARG and "null context" in err()
    assert L.bmk_finish(None, None) == phase.BMK_ERR_ARG and "null context" in err()
    assert L.bmk_create(0, None) == phase.BMK_ERR_ARG and L.bmk_last_stats(None, None, None) == phase.BMK_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import phase
    with pytest.raises(phase.BmkError) as e:
        phase.Phase(0)
    assert e.value.code == phase.BMK_ERR_HIP
