"""Indel calls (-o x.bam --vcf FILE --vcf-indels) without a GPU: the rule on cases worked out by hand, host/indel.h as a program
of its own under ASan + UBSan, the oracle-backed tools (whose calling is the host default of block_compressor), the command line
and the bmn_* ABI surface.

The yardstick is the rule of include/bmn.h in plain Python (tests/indel_rule.py), applied to the records decoded from the x.bam
the tool wrote and to the FASTA file: the indel lines of the VCF are a function of those alone.  Every tool run has its own time
limit; nothing is retried."""
import ctypes as C
import glob
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import genotype_rule as G
import indel_rule as N
from indel_cases import L, edge_placements, ins_record, many_indel_ops, min_frac_records, same_anchor_records, threshold_records
from pileup_cases import EDGE_REFS, REF_LENS, edge_records, many_ops_record, random_records, references
from test_bamsort import offsets_of, pair_of, records_of
from test_depth import full_record, header_refs
from test_genotype import genotypes_by_the_rule, genotypes_line
from test_pileup import fasta_bases
from test_sam_golden import ROOT, TOOLS

INDELS = re.compile(r"Indels: (\d+) variants \((\d+) het, (\d+) hom, (\d+) below QUAL\) at (\d+) sites from (\d+) events \((\d+) other\)")
LOOSE = dict(min_alt=1, min_frac_ppm=0)
PARAM_SETS = ({}, LOOSE, dict(min_mapq=20, min_alt=1, min_frac_ppm=1, q_indel=1, prior=0), dict(min_alt=3, min_frac_ppm=1000000, q_indel=93, prior=2 ** 32 - 1))
INFO_LINE = '##INFO=<ID=INDEL,Number=0,Type=Flag,Description="An insertion or deletion behind POS, from the CIGARs of the records">'


# ---- the rule by hand ----
def test_python_restatement_of_the_rule():
    refs, recs, expect = edge_placements()
    assert [len(N.indels([r], refs, **LOOSE).events) for r in recs] == expect
    one = N.indels([ins_record(0, 10, 4, "CG")], [100], **LOOSE)
    assert one.events == [(13, 2 | N.INS, 1 | 2 << 2, 0)] and one.alleles == [(0, 13, 2 | N.INS, 9, 0, 1, 0, 0)]
    assert one.cover[0][9:18].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0]      # pos 10, end 18: the steps 10 .. 16
    # one read with, none without: L = 3000, 301 + 4000, 4000 -> RR with GQ 10
    assert one.calls == [(0, 13, 2 | N.INS, 9, 0, 1, 0, 10, 0, 0, 1, 0, 1, 0, 1301, 1000)]
    hom = N.indels([ins_record(0, 10, 4, "CG", b"r%d" % k) for k in range(3)], [100])
    assert hom.calls[0][5:16] == (3, 2, 9, 5000, 0, 3, 0, 3, 5000, 903, 0)       # 9000, 903 + 4000, 4000
    het = N.indels(min_frac_records() + [ins_record(0, 10, 4, "C", b"again")], [100])      # 2 with, 3 without: 6000, 1505 + 4000, 9000 + 4000
    assert het.calls[0][5:16] == (3, 1, 4, 495, 3, 2, 0, 5, 495, 0, 7495)
    assert len(N.indels(min_frac_records(), [100], min_alt=1, min_frac_ppm=250000).calls) == 1
    assert len(N.indels(min_frac_records(), [100], min_alt=1, min_frac_ppm=250001).calls) == 0
    assert [c[1] for c in N.indels(threshold_records(), [100], min_alt=3, min_frac_ppm=0).calls] == [32]
    long_ins = N.indels([ins_record(0, 10, 4, "A" * 33)] * 2 + [ins_record(0, 10, 4, "ANA")], [100], **LOOSE)
    assert [a[2:6] for a in long_ins.alleles] == [(3 | N.INS | N.OTHER, 0, 0, 1), (33 | N.INS | N.OTHER, 0, 0, 2)] and long_ins.calls == []
    skipped = N.indels([ins_record(0, 10, 4, "C", mapq=5), L(0, 10, "4M1I4M", "ACGTCACGT", flag=0x400)], [100], min_mapq=6, **LOOSE)
    assert skipped.events == [] and skipped.stats == [[0, 1, 0]] and not skipped.cover[0].any()
    assert N.vcf_fields((0, 3, 2 | N.INS, 9, 0), b"acgNacgt") == (4, "A", "ACG") and N.vcf_fields((0, 2, 3, 0, 0), b"acgNacgt") == (3, "GAAC", "G")


# ---- host/indel.h as a program of its own ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("indel_check")
    exe = str(d / "indel_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "indel_check.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def clean(r, expect=0):
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode == expect, r.stderr[-3000:]
    return r.stdout


def run_check(checker, recs, ref_len, n_calls=1, seed=0, skip=None, expect=0, **params):
    d, exe = checker
    pr = {**N.DEFAULTS, **params}
    (d / "records.bin").write_bytes(b"".join(recs))
    if skip is not None:
        (d / "skip.bin").write_bytes(bytes(skip))
    r = subprocess.run([exe, "records.bin", "skip.bin" if skip is not None else "-", str(n_calls), str(seed),
                        *[str(pr[k]) for k in N.DEFAULTS], *[str(x) for x in ref_len]], cwd=str(d), capture_output=True, text=True, timeout=120)
    return clean(r, expect)


def same_as_rule(out, want):
    lines = out.split("\n")
    numbers = lambda l: tuple(int(x) for x in l.split())
    assert lines[0] == f"events {len(want.events)}" and lines[1] == f"alleles {len(want.alleles)}"
    at = 2
    assert [numbers(l) for l in lines[at: at + len(want.alleles)]] == want.alleles
    at += len(want.alleles)
    assert lines[at] == f"calls {len(want.calls)}"
    assert [numbers(l) for l in lines[at + 1: at + 1 + len(want.calls)]] == want.calls
    at += 1 + len(want.calls)
    n_ref = len(want.stats)
    assert [[int(x) for x in l.split()[1:]] for l in lines[at: at + n_ref]] == want.stats and all(l.startswith("stats") for l in lines[at: at + n_ref])
    for r in range(n_ref):
        assert np.array_equal(np.array(lines[at + n_ref + r].split()[1:], np.int64), want.cover[r]), r
    assert lines[at + 2 * n_ref] == N.indel_line(want, 20) and lines[at + 2 * n_ref + 1:] == [""]


@pytest.mark.parametrize("size", [0, 1, 65, 1025, 5001])
def test_host_rule_is_the_python_rule(checker, size):
    recs = random_records(size, 500 + size)
    for k, pr in enumerate(PARAM_SETS if size == 1025 else PARAM_SETS[1:2]):
        want = N.indels(recs, REF_LENS, **pr)
        same_as_rule(run_check(checker, recs, REF_LENS, **pr), want)
        same_as_rule(run_check(checker, recs, REF_LENS, n_calls=3 + k, seed=7 + k, **pr), want)    # order and cutting do not matter
    if size >= 1025:
        loose = N.indels(recs, REF_LENS, **LOOSE)
        assert len(loose.calls) > 20 and {0, 2} <= {c[6] for c in loose.calls}
        skip = [int(k % 3 == 1) for k in range(size)]
        same_as_rule(run_check(checker, recs, REF_LENS, skip=skip, n_calls=2, seed=3, **LOOSE), N.indels(recs, REF_LENS, skip, **LOOSE))


def test_host_rule_on_the_edges_and_a_record_of_many_ops(checker):
    refs, recs, _ = edge_placements()
    for pr in PARAM_SETS:
        same_as_rule(run_check(checker, recs, refs, **pr), N.indels(recs, refs, **pr))
        same_as_rule(run_check(checker, edge_records(), EDGE_REFS, **pr), N.indels(edge_records(), EDGE_REFS, **pr))
    recs = [many_indel_ops(0, 17, 60001, 3), many_ops_record(0, 40000), many_indel_ops(1, 3, 129, 5)] + same_anchor_records(300, 500)
    want = N.indels(recs, [90000, 300], **LOOSE)
    assert len(want.events) > 30000 and max(c[11] for c in want.calls) >= 299
    same_as_rule(run_check(checker, recs, [90000, 300], n_calls=2, seed=5, **LOOSE), want)
    for size in (1, 16, 31, 32, 33):
        recs = [ins_record(0, 10 + lead, lead, ("ACGGTCA" * 5)[:size], name) for lead in (3, 4) for name in (b"", b"x", b"xy", b"xyz")]
        same_as_rule(run_check(checker, recs, [100], **LOOSE), N.indels(recs, [100], **LOOSE))


def test_host_rule_refuses_what_the_abi_refuses(checker):
    good = random_records(20, 3)
    for lens, pr in (([4, 0], {}), ([2 ** 32 - 2 ** 20, 1], {}), ([4], dict(min_alt=0)), ([4], dict(min_frac_ppm=1000001)), ([4], dict(q_indel=0)),
                     ([4], dict(q_indel=94))):
        assert run_check(checker, [], lens, expect=3, **pr).startswith("refused ")
    for r in (full_record(ops=[4 << 4 | 9]), full_record(ops=[3 << 4])):
        assert run_check(checker, good + [r], REF_LENS, expect=3).startswith("refused ")
    on_ref_9 = bytearray(full_record(ops=[4 << 4]))
    struct.pack_into("<i", on_ref_9, 4, 9)
    assert run_check(checker, good + [bytes(on_ref_9)], REF_LENS, expect=3).startswith("refused ")


def test_vcf_lines_are_the_python_text(checker):
    d, exe = checker
    bases = [b"ACGTNacgtRACGTACGTACGTACGTACGTACGTACGTACGT", b"ttttttttttttgggggggggg"]
    ins32 = sum(((k * 7 + 1) % 4) << (2 * k) for k in range(32))
    calls = [
        (0, 0, 1 | N.INS, 2, 0, 3, 1, 35, 1234, 4, 3, 1, 8, 1234, 0, 4321),          # anchor 0, one inserted G, het
        (0, 3, 3, 0, 0, 3, 2, 99, 2 ** 32 - 1, 0, 7, 0, 7, 2 ** 32 - 1, 900, 0),     # a deletion over N a c, hom, saturated
        (0, 4, 2, 0, 0, 1, 0, 5, 0, 9, 1, 0, 10, 0, 500, 9000),                      # not a variant: no line
        (0, 8, 32 | N.INS, ins32 & 0xFFFFFFFF, ins32 >> 32, 3, 1, 0, 1999, 5, 5, 0, 10, 1999, 0, 5),   # 32 bases; QUAL below 20
        (1, 11, 10, 0, 0, 3, 1, 12, 2000, 3, 3, 2, 8, 2000, 0, 100),                 # a deletion to the last base of the reference
        (1, 20, 1 | N.INS, 0, 0, 3, 2, 9, 2001, 0, 2, 0, 2, 2001, 30, 0),            # the last possible anchor
    ]
    (d / "calls.bin").write_bytes(np.array(calls, np.uint32).tobytes())
    names = ["chr1", "two words"]
    r = subprocess.run([exe, "vcf", "calls.bin", "20", *[f"{n}:{b.decode()}" for n, b in zip(names, bases)]], cwd=str(d), capture_output=True,
                       text=True, timeout=120)
    want = [N.vcf_line(c, names[c[0]], bases[c[0]], 20) for c in calls]
    assert want[2] is None and clean(r) == "\n".join([INFO_LINE] + [l for l in want if l]) + "\n"
    assert want[0] == "chr1\t1\t.\tA\tAG\t12.34\tLowQual\tINDEL;DP=8\tGT:DP:AD:GQ:PL\t0/1:8:4,3:35:12,0,43"
    assert want[1].split("\t")[:7] == ["chr1", "4", ".", "TAAC", "T", "42949672.95", "PASS"] and want[3].split("\t")[5:7] == ["19.99", "LowQual"]
    assert want[4].split("\t")[:5] == ["two words", "12", ".", "TGGGGGGGGGG", "T"] and len(want[3].split("\t")[4]) == 33
    beyond = (1, 12, 10, 0, 0, 3, 1, 12, 2000, 3, 3, 2, 8, 2000, 0, 100)           # one base too far: refused, not read
    (d / "calls.bin").write_bytes(np.array([beyond], np.uint32).tobytes())
    r = subprocess.run([exe, "vcf", "calls.bin", "20", *[f"{n}:{b.decode()}" for n, b in zip(names, bases)]], cwd=str(d), capture_output=True,
                       text=True, timeout=120)
    assert clean(r, 3).startswith("refused ")


# ---- the command line ----
def test_cli_refusals(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        run = lambda *opts: subprocess.run([exe, "-i", "idx", *opts], cwd=str(tmp_path), capture_output=True, text=True, timeout=60)
        fine = lambda r: "Validation failed" not in r.stderr and "Unknown option" not in r.stderr and "Value parse failed" not in r.stderr
        for opts in (("--vcf-indels",), ("--vcf-indel-qual", "20"), ("--vcf-indel-prior", "20")):
            r = run("-o", "x.bam", *opts)                # an option of --vcf without it: the wording of the other --vcf-* options
            assert r.returncode != 0 and f"Validation failed for option {opts[0]}: it is an option of --vcf FILE, which is not given." in r.stderr, r.stderr
            r = run("-o", "x.bam", "--pileup", "p.tsv", *opts)
            assert r.returncode != 0 and "--vcf FILE" in r.stderr
            assert fine(run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-indels", *opts))
        for opt in ("--vcf-indel-qual", "--vcf-indel-prior"):
            r = run("-o", "x.bam", "--vcf", "v.vcf", opt, "20")                  # an option of --vcf-indels without it
            assert r.returncode != 0 and f"Validation failed for option {opt}" in r.stderr and "--vcf-indels, which is not given" in r.stderr, r.stderr
            r = run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-indels", opt)
            assert r.returncode != 0 and "Missing value" in r.stderr
        for opt, bads, goods in (("--vcf-indel-qual", ("x", "-1", "", "0", "94", "1.5"), ("1", "93")), ("--vcf-indel-prior", ("x", "-1", "", "256", "2e1"), ("0", "255"))):
            for bad in bads:
                r = run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-indels", opt, bad)
                assert r.returncode != 0 and "Value parse failed for " + opt in r.stderr, (opt, bad, r.stderr)
            for good in goods:
                assert fine(run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-indels", opt, good))
        assert fine(run("-o", "x.bam", "--vcf", "v.vcf", "--vcf-indels", "--pileup-min-alt", "3", "--pileup-min-frac", "0.5", "--pileup-min-mapq", "20"))
        assert not os.listdir(tmp_path)


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import indel
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmn.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bmn_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(indel.SYMBOLS) and len(names) == 11
    lib = indel.lib()
    for n in names:
        assert hasattr(lib, n), f"libbmf.so does not export {n}"
    for n in ("bmn_create", "bmn_destroy", "bmn_last_error", "bmn_begin", "bmn_add", "bmn_finish", "bmn_alleles", "bmn_calls", "bmn_events_of",
              "bmn_cover_at", "bmn_last_stats"):
        assert n in names
    assert (indel.EVENT_WORDS, indel.ALLELE_WORDS, indel.CALL_WORDS, indel.N_STATS) == (4, 8, 16, 3) and indel.DEFAULTS == N.DEFAULTS
    assert list(indel.PARAMS) == list(N.DEFAULTS) and (indel.INS, indel.OTHER, indel.MAX_INS) == (N.INS, N.OTHER, N.MAX_INS)
    for word in ("BMN_CALL_WORDS = 16", "BMN_N_PARAMS = 5", "4 bytes per base", "16 bytes per event", "LEFT OUT, on purpose"):
        assert word in open(os.path.join(ROOT, "include", "bmn.h")).read()


def test_argument_errors_need_no_device():
    from bucket_map_amd import indel
    lib = indel.lib()
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
    }

    def add(stream, off, n, null=(), skip=True):
        a = np.frombuffer(stream, np.uint8)
        o = np.asarray(off, np.uint64)
        s = np.zeros(8, np.uint8)
        p = dict(a=a.ctypes.data_as(u8p), o=o.ctypes.data_as(u64p))
        for k in null:
            p[k] = None
        return lib.bmn_add(None, p["a"], len(stream), p["o"], n, s.ctypes.data_as(u8p) if skip else None)

    err = lambda: lib.bmn_last_error().decode()
    for name, (stream, off, n, word) in cases.items():
        assert add(stream, off, n) == indel.BMN_ERR_ARG, name
        assert word in err() and "bmn_add" in err(), (name, err())
    for null in ("a", "o"):
        assert add(good, good_off, 2, null=(null,)) == indel.BMN_ERR_ARG and "null argument" in err()
    for skip in (True, False):                           # good data: only the context is missing
        assert add(good, good_off, 2, skip=skip) == indel.BMN_ERR_ARG and "null context" in err()
    assert add(b"", [0], 0) == indel.BMN_ERR_ARG and "null context" in err()

    def begin(lens, n=None, null=(), pr=(0, 2, 200000, 30, 4000)):
        a, t = np.asarray(lens, np.uint32), np.asarray(pr, np.uint32)
        p = dict(lens=a.ctypes.data_as(u32p), pr=t.ctypes.data_as(u32p))
        for k in null:
            p[k] = None
        return lib.bmn_begin(None, p["lens"], len(lens) if n is None else n, p["pr"])

    assert begin([5], n=0) == indel.BMN_ERR_ARG and "n_ref is 0" in err()
    assert begin([5, 0, 7]) == indel.BMN_ERR_ARG and "reference 1 has the length 0" in err()
    assert begin([2 ** 32 - 2 ** 20, 1]) == indel.BMN_ERR_ARG and "2^32 - 2^20" in err()
    for null in ("lens", "pr"):
        assert begin([5], null=(null,)) == indel.BMN_ERR_ARG and "null argument" in err()
    assert begin([5], pr=(0, 0, 200000, 30, 4000)) == indel.BMN_ERR_ARG and "min_alt" in err()
    assert begin([5], pr=(0, 2, 1000001, 30, 4000)) == indel.BMN_ERR_ARG and "min_frac_ppm" in err()
    assert begin([5], pr=(0, 2, 200000, 0, 4000)) == indel.BMN_ERR_ARG and "q_indel" in err()
    assert begin([5], pr=(0, 2, 200000, 94, 4000)) == indel.BMN_ERR_ARG and "q_indel" in err()
    assert begin([2 ** 32 - 2 ** 20]) == indel.BMN_ERR_ARG and "null context" in err()
    assert begin([1], pr=(255, 2 ** 32 - 1, 1000000, 93, 2 ** 32 - 1)) == indel.BMN_ERR_ARG and "null context" in err()
    n, out = (C.c_uint64 * 3)(), np.zeros(16, np.uint32)
    p64, p32 = C.cast(n, u64p), out.ctypes.data_as(u32p)
    assert lib.bmn_finish(None, p64, p64, p64, None) == indel.BMN_ERR_ARG and "null argument" in err()
    assert lib.bmn_finish(None, p64, p64, p64, p64) == indel.BMN_ERR_ARG and "null context" in err()
    for fn in (lib.bmn_alleles, lib.bmn_calls):
        assert fn(None, 0, 1, None) == indel.BMN_ERR_ARG and "null argument" in err()
        assert fn(None, 0, 1, p32) == indel.BMN_ERR_ARG and "null context" in err()
    assert lib.bmn_cover_at(None, 0, 0, 1, None) == indel.BMN_ERR_ARG and "null argument" in err()
    assert lib.bmn_cover_at(None, 0, 0, 1, p32) == indel.BMN_ERR_ARG and "null context" in err()
    assert lib.bmn_events_of(None, 0, None, None, None) == indel.BMN_ERR_ARG and "null argument" in err()
    assert lib.bmn_events_of(None, 0, p64, None, p32) == indel.BMN_ERR_ARG and "null argument" in err()
    assert lib.bmn_events_of(None, 0, p64, p64, None) == indel.BMN_ERR_ARG and "null context" in err()
    assert lib.bmn_create(0, None) == indel.BMN_ERR_ARG and lib.bmn_last_stats(None, None, None) == indel.BMN_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import indel
    with pytest.raises(indel.BmnError) as e:
        indel.Indel(0)
    assert e.value.code == indel.BMN_ERR_HIP


# ---- the oracle-backed tools ----
def run_tool(exe, d, args, out, extra=(), env=None, limit=120):
    r = subprocess.run([exe, *args, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, timeout=limit, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert not glob.glob(str(d / "*.tmp")), "a run file was left behind"
    return r.stderr


def indels_line(err):
    found = [l.split("\t")[-1] for l in err.split("\n") if "Indels:" in l]
    assert len(found) == 1 and INDELS.fullmatch(found[0]), err
    return found[0]


def indels_by_the_rule(bam_path, args, min_qual=20, **params):
    """(the indel lines as (reference index, POS, text), the stderr line, the rule's result) for the records of a BAM file and the
    FASTA file of the tool's arguments."""
    fasta = os.path.join(os.path.dirname(bam_path), args[args.index("--genome") + 1])
    cut = int(args[args.index("--bucket-len") + 1]), int(args[args.index("-r") + 1])
    raw = gzip.decompress(open(bam_path, "rb").read())
    refs = header_refs(raw)
    recs = [r for _, r in records_of(raw)[0]]
    bases = fasta_bases(fasta, refs, *cut)
    res = N.indels(recs, [l for _, l in refs], **params)
    lines = [(c[0], c[1] + 1, N.vcf_line(c, refs[c[0]][0], bases[c[0]], min_qual)) for c in res.calls if c[5] & N.VARIANT]
    return lines, N.indel_line(res, min_qual), res


def merged(snv_lines, indel_lines, refs):
    """The lines of both kinds by (reference, POS); the SNV first at an equal POS."""
    index = {name: k for k, (name, _) in enumerate(refs)}
    keyed = [((index[l.split("\t")[0]], int(l.split("\t")[1]), 0), l) for l in snv_lines] + [((r, p, 1), l) for r, p, l in indel_lines]
    return [l for _, l in sorted(keyed, key=lambda x: x[0])]


def split_header(text):
    """The text without the INFO line of --vcf-indels, which stands once, behind the INFO line of DP."""
    lines = text.split("\n")
    at = lines.index(INFO_LINE)
    assert lines.count(INFO_LINE) == 1 and lines[at - 1].startswith("##INFO=<ID=DP,") and lines[at + 1].startswith("##FILTER=")
    return "\n".join(lines[:at] + lines[at + 1:])


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_pileup import pileup_jobs
    return pileup_jobs(tmp_path_factory)


LOOSE_OPTS = ["--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--pileup-min-bq", "0"]


@pytest.mark.parametrize("k", range(3))
def test_oracle_tool_writes_what_the_rule_says(jobs, k):
    name, which, d, args, extra = jobs[k]
    exe = TOOLS[(which, "oracle")]
    aligned = name != "plain"                            # the plain tool writes no CIGAR: no event and no line
    # without the option: the file of --vcf alone, byte for byte, and no line on stderr
    err = run_tool(exe, d, args, f"{name}.n0.bam", [*extra, "--vcf", f"{name}.n0.vcf"])
    assert "Indels:" not in err
    plain_text = (d / f"{name}.n0.vcf").read_text()
    assert "INDEL" not in plain_text
    # with it, the defaults
    err = run_tool(exe, d, args, f"{name}.n.bam", [*extra, "--vcf", f"{name}.n.vcf", "--vcf-indels"])
    assert pair_of(d, f"{name}.n") == pair_of(d, f"{name}.n0") and genotypes_line(err)
    snv, _, refs, _ = genotypes_by_the_rule(d / f"{name}.n.bam", args)
    lines, told, res = indels_by_the_rule(d / f"{name}.n.bam", args)
    text = (d / f"{name}.n.vcf").read_text()
    assert G.check_vcf_header(split_header(text), refs) == merged(snv, lines, refs) and indels_line(err) == told
    assert [l for l in text.split("\n") if "\tINDEL;" not in l and l != INFO_LINE] == plain_text.split("\n")
    if aligned:
        assert len(res.events) > 10 and len(lines) >= 2 and any(l[2].split("\t")[3] > l[2].split("\t")[4] for l in lines), told
    else:
        assert lines == [] and told == "Indels: 0 variants (0 het, 0 hom, 0 below QUAL) at 0 sites from 0 events (0 other)"
        assert split_header(text) == plain_text
    # looser thresholds, the two options, in one run and in several, with --markdup
    opts = [*LOOSE_OPTS, "--vcf-indels", "--vcf-indel-qual", "7", "--vcf-indel-prior=3", "--vcf-min-qual", "10"]
    pr = dict(min_alt=1, min_frac_ppm=1, q_indel=7, prior=300)
    err = run_tool(exe, d, args, f"{name}.nl.bam", [*extra, "--vcf", f"{name}.nl.vcf", *opts])
    l_snv, _, _, _ = genotypes_by_the_rule(d / f"{name}.nl.bam", args, pile_th=dict(min_bq=0, min_alt=1, min_frac_ppm=1), min_qual=10)
    l_lines, l_told, l_res = indels_by_the_rule(d / f"{name}.nl.bam", args, min_qual=10, **pr)
    l_text = (d / f"{name}.nl.vcf").read_text()
    assert G.check_vcf_header(split_header(l_text), refs) == merged(l_snv, l_lines, refs) and indels_line(err) == l_told
    assert not aligned or (len(l_res.calls) > len(res.calls) and l_lines != lines and {l[2].split("\t")[9][:3] for l in lines + l_lines} == {"0/1", "1/1"})
    err = run_tool(exe, d, args, f"{name}.nr.bam", [*extra, "--vcf", f"{name}.nr.vcf", *opts], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1 and (d / f"{name}.nr.vcf").read_text() == l_text and indels_line(err) == l_told
    err = run_tool(exe, d, args, f"{name}.nm.bam", [*extra, "--markdup", "--vcf", f"{name}.nm.vcf", *opts])
    m_lines, m_told, m_res = indels_by_the_rule(d / f"{name}.nm.bam", args, min_qual=10, **pr)
    assert indels_line(err) == m_told and not aligned or sum(s[0] for s in m_res.stats) < sum(s[0] for s in l_res.stats)
    assert [l for l in (d / f"{name}.nm.vcf").read_text().split("\n") if "\tINDEL;" in l] == [l for _, _, l in m_lines]
