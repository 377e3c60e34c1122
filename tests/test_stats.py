"""Mapping statistics (--stats FILE) without a GPU: the rule on cases worked out by hand, host/stats.h as a program of its own
under ASan + UBSan against the Python rule, the writer, the sorter in one run and in several, with and without --markdup,
through the oracle-backed tools (whose counter is the host default of block_compressor), the command line and the bmq_* ABI
surface.

The yardstick is the rule of include/bmq.h in plain Python (tests/stats_rule.py)."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import stats_rule as Q
from stats_cases import DESIGNED, border_reads, long_read, ops_record, qrec, random_set, short_reads
from test_bamsort import offsets_of, pair_of, records_of, run_tool
from test_depth import full_record
from test_sam_golden import ROOT, TOOLS

STATS = re.compile(r"Stats: (\d+) records \((\d+) mapped, (\d+) properly paired, (\d+) duplicates\), (\d+) bases, (\d+) of (\d+) =/X bases mismatch")
MARKED = re.compile(r"Marked (\d+) of (\d+) records as duplicates")


def python_rule(records, skip=None, **params):
    return Q.run(records, skip, **params)


@pytest.mark.parametrize("case", DESIGNED, ids=lambda f: f.__name__[5:])
def test_python_rule_on_the_designed_cases(case):
    case(python_rule)


# ---- host/stats.h as a program of its own ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("stats_check")
    exe = str(d / "stats_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "stats_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def clean(r, expect=0):
    """expect None: the program may refuse (3) or not (0)."""
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode in ((0, 3) if expect is None else (expect,)), r.stderr[-3000:]
    return r.stdout


def run_check(checker, recs, n_adds=1, seed=0, skip=None, expect=0, as_text=False, **params):
    d, exe = checker
    pr = {**Q.DEFAULTS, **params}
    (d / "records.bin").write_bytes(b"".join(recs))
    if skip is not None:
        (d / "skip.bin").write_bytes(bytes(skip))
    r = subprocess.run([exe, "records.bin", "skip.bin" if skip is not None else "-", str(n_adds), str(seed), str(pr["max_cycle"]), str(pr["max_insert"]),
                        *(["text"] if as_text else [])], cwd=str(d), capture_output=True, text=True)
    return (clean(r, expect), r.stderr) if as_text else clean(r, expect)


def parsed(out):
    """(tallies, tables) of the checker's output, as stats_rule.run returns them."""
    lines = out.split("\n")
    assert lines[0].startswith("tallies ")
    t = [int(x) for x in lines[0].split()[1:]]
    tab, name = {}, None
    for line in lines[1:]:
        if line.startswith("table "):
            _, k, n_rows, width = line.split()
            name = Q.TABLES[int(k)]
            tab[name] = np.zeros((int(n_rows), int(width)), np.int64)
        elif line:
            r, c, v = (int(x) for x in line.split())
            tab[name][r, c] = v
    return t, tab


def same(got, want):
    (t, tab), (want_t, want_tab) = got, want
    assert [int(x) for x in t] == [int(x) for x in want_t], [(Q.NAMES[k], int(a), int(b)) for k, (a, b) in enumerate(zip(t, want_t)) if int(a) != int(b)]
    assert list(tab) == list(want_tab) == list(Q.TABLES)
    for name in Q.TABLES:
        a, b = np.asarray(tab[name]).astype(np.int64), want_tab[name]
        assert a.shape == b.shape, name
        assert (a == b).all(), (name, np.argwhere(a != b)[:5].tolist())


def host_rule(checker):
    """host/stats.h as the engine of the designed cases: what it prints, after it has been compared with the Python rule too."""
    def rule(records, skip=None, **params):
        got = parsed(run_check(checker, records, skip=skip, **params))
        same(got, Q.run(records, skip, **params))
        return got
    return rule


@pytest.mark.parametrize("case", DESIGNED, ids=lambda f: f.__name__[5:])
def test_host_rule_on_the_designed_cases(checker, case):
    case(host_rule(checker))


@pytest.mark.parametrize("size", [1, 63, 65, 2000])
def test_host_rule_is_the_python_rule(checker, size):
    recs = random_set(size, 40 + size)
    want = Q.run(recs)
    one = run_check(checker, recs)
    same(parsed(one), want)
    if size == 2000:                                     # the set reaches every tally but the placeholder's and every table
        t, tab = want
        assert all(t[k] > 0 for k in range(Q.N_TALLIES) if k not in (Q.T["left_out"], Q.T["reads_no_acgt"])) and all(tab[name].any() for name in Q.TABLES)
        assert min((tab["IS"] > 0).sum(axis=0).tolist()) > 3 and tab["IS"][8000].sum() > 0 and tab["MC"][:, 5].sum() > 50
    if size >= 65:                                       # order and cutting do not matter; other parameters; skip bytes
        assert run_check(checker, recs, n_adds=3, seed=1 + size) == one
        assert run_check(checker, recs, n_adds=7, seed=size) == one
        for pr in (dict(max_cycle=1, max_insert=1), dict(max_cycle=20, max_insert=50), dict(max_cycle=65535, max_insert=65535)):
            same(parsed(run_check(checker, recs, **pr)), Q.run(recs, **pr))
        skip = [int(k % 3 == 1) for k in range(size)]
        same(parsed(run_check(checker, recs, skip=skip)), Q.run(recs, skip))


def test_host_rule_on_records_of_many_ops_and_many_bases(checker):
    recs = [ops_record(300, 5), ops_record(5000, 6), ops_record(60000, 7), long_read(), long_read(9000, 12, 0)] + border_reads()
    for pr in ({}, dict(max_cycle=100), dict(max_cycle=65535)):
        want = Q.run(recs, **pr)
        same(parsed(run_check(checker, recs, n_adds=2, **pr)), want)
    assert want[0][Q.T["bases_beyond_cycle"]] >= 70000 - 65535 and want[1]["ID"].sum() > 1000   # the long read's, and the 60 000-op record's
    assert Q.run([long_read()], max_cycle=65535)[0][Q.T["bases_beyond_cycle"]] == 70000 - 65535


def test_host_rule_refuses_what_the_abi_refuses(checker):
    from test_markdup_gpu import rec, rec_ops
    ok = [qrec(0, "3M", "ACG")]
    assert run_check(checker, ok).startswith("tallies 1 ")
    for pr in (dict(max_cycle=0), dict(max_cycle=65536), dict(max_insert=0), dict(max_insert=65536)):
        assert run_check(checker, ok, expect=3, **pr).startswith("refused")
        with pytest.raises(Q.Refused):
            Q.run(ok, **pr)
    for stream in ([rec_ops(0, 0, 0, [3 << 4 | 9], b"")], [rec(0, 5, 0, "3M", b"ab")], [rec(0, 5, 0, "1M2I", b"ab")]):
        assert run_check(checker, ok + stream, expect=3).startswith("refused")
        with pytest.raises(Q.Refused):
            Q.run(ok + stream)
    assert run_check(checker, [rec(7, 5, 0, "2M", b"ab")]).startswith("tallies 1 ")      # any refID: there are no references


# ---- the writer ----
def test_writer_is_the_python_text(checker):
    sets = [([], {}), ([qrec(4, "", "")], {}), (random_set(2000, 2040), {}), (random_set(300, 9), dict(max_cycle=20, max_insert=50)),
            (short_reads(300), dict(max_insert=500)), (border_reads(), dict(max_cycle=30)), ([qrec(0, "2M", "AC", [0xFF, 0xFF])], {})]
    for recs, pr in sets:
        t, tab = Q.run(recs, **pr)
        text, err = run_check(checker, recs, as_text=True, **pr)
        assert text == Q.text(t, tab, {**Q.DEFAULTS, **pr}["max_insert"])
        assert err.strip() == Q.summary_line(t) and STATS.fullmatch(err.strip())
    # the shape of the file, on the last but one set: 40-base reads with max_cycle 30
    t, tab = Q.run(border_reads(), max_cycle=30)
    lines = Q.text(t, tab, 8000).split("\n")
    assert lines[0] == "# bucketmap --stats 1" and lines[1] == "SN\trecords\t2" and lines[35] == "SN\treads_no_acgt\t0"
    assert lines[36:40] == ["SN\terror_rate_ppm\t.", "SN\tmean_quality_centi\t1950", "SN\tmean_length_centi\t4000", "SN\tinsert_size_median\t."]
    assert [l for l in lines if l.startswith("#")][1:] == ["# MAPQ\tmapq\trecords", "# RL\tlength\trecords", "# GCF\tgc_percent\trecords",
                                                            "# ID\tlength\tinsertions\tdeletions", "# IS\tinsert_size\tinward\toutward\tother",
                                                            "# BCC\tcycle\tA\tC\tG\tT\tother", "# QCC\tcycle\t" + "\t".join(f"q{q}" for q in range(30)),
                                                            "# MCC\tcycle\t=\tX\tM\tI\tS\tD"]
    assert "RL\t30\t2" in lines and "MAPQ\t30\t2" in lines and sum(l.startswith("BCC\t") for l in lines) == 30 and "BCC\t30\t0\t1\t0\t1\t0" in lines
    assert "MCC\t10\t0\t0\t1\t0\t1\t0" in lines and "MCC\t11\t0\t0\t2\t0\t0\t0" in lines
    # the median: the smallest insert size at which the doubled cumulative count of the inward pairs reaches their total
    pairs = [qrec(0x61, "2M", "AC", tlen=v) for v in (5, 5, 7, 9, 60)] + [qrec(0x51, "2M", "AC", tlen=1)]
    t, tab = Q.run(pairs, max_insert=50)
    assert dict(Q.derived(t, tab, 50))["insert_size_median"] == 5                         # the 60 lies in row I and does not count
    assert "SN\tinsert_size_median\t5\n" in run_check(checker, pairs, as_text=True, max_insert=50)[0]
    t, tab = Q.run(pairs[2:], max_insert=50)
    assert dict(Q.derived(t, tab, 50))["insert_size_median"] == 7 and "SN\tinsert_size_median\t7\n" in run_check(checker, pairs[2:], as_text=True, max_insert=50)[0]


# ---- the oracle-backed tools ----
def stats_by_the_rule(bam_path, **params):
    """(the --stats text, the Stats line, the tallies) for the records of a BAM file."""
    raw = gzip.decompress(open(bam_path, "rb").read())
    recs = [r for _, r in records_of(raw)[0]]
    t, tab = Q.run(recs, **params)
    return Q.text(t, tab, {**Q.DEFAULTS, **params}["max_insert"]), Q.summary_line(t), t


def stats_line(err):
    found = [l.split("\t")[-1] for l in err.split("\n") if "Stats:" in l]
    assert len(found) == 1 and STATS.fullmatch(found[0]), err
    after = err[err.index(found[0]):]                    # the last thing the run says of its output files
    assert not any(word in after for word in ("Sorted ", "Marked ", "Coverage:", "Pileup:", "Genotypes:", "Indels:", "Blocks:", "Bias:", "Phase:"))
    return found[0]


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_markdup import markdup_jobs
    return markdup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", range(3))
def test_oracle_tool_writes_what_the_rule_says(jobs, k):
    name, which, d, args, extra = jobs[k]
    exe = TOOLS[(which, "oracle")]
    run_tool(exe, d, args, f"{name}.qi.bam", [*extra, "--sort"])                 # the first run of a job builds its index and says so
    err0 = run_tool(exe, d, args, f"{name}.q0.bam", [*extra, "--sort"])
    assert "Stats:" not in err0
    err = run_tool(exe, d, args, f"{name}.q.bam", [*extra, "--stats", f"{name}.q.txt"])
    assert re.search(r"Sorted \d+ records by coordinate in 1 run", err)
    assert pair_of(d, f"{name}.q") == pair_of(d, f"{name}.q0")                   # the BAM and its index are what they were
    said = lambda e: [l for l in e.split("\n") if not l.startswith("[BENCHMARK]")]      # the timings differ from run to run
    assert [l for l in said(err) if "Stats:" not in l] == said(err0)             # ... and stderr but for the one line
    text, told, t = stats_by_the_rule(d / f"{name}.q.bam")
    assert (d / f"{name}.q.txt").read_text() == text and stats_line(err) == told
    assert t[Q.T["records"]] > 20 and t[Q.T["bases"]] > 1000 and t[Q.T["duplicates"]] == 0
    if name == "plain":                                  # no CIGAR: the read-level sections are filled, the CIGAR-derived ones empty
        assert t[Q.T["aligned_records"]] == 0 and sum(t[22:30]) == 0 and "\nMCC\t" not in text and "\nID\t" not in text and "\nBCC\t1\t" in text and "\nQCC\t1\t" in text
    else:
        assert t[Q.T["aligned_records"]] > 20 and "\nMCC\t1\t" in text
    if name == "pairs":
        assert t[Q.T["properly_paired"]] > 20 and t[Q.T["pairs_in_is"]] > 10 and "\nIS\t" in text and "SN\tinsert_size_median\t." not in text
    # several runs: the same file
    errn = run_tool(exe, d, args, f"{name}.qn.bam", [*extra, "--stats", f"{name}.qn.txt"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", errn).group(1)) > 1
    assert (d / f"{name}.qn.txt").read_text() == text and stats_line(errn) == told and pair_of(d, f"{name}.qn") == pair_of(d, f"{name}.q0")
    # with --markdup the duplicate tally is the marker's count, in one run and in several
    run_tool(exe, d, args, f"{name}.qm0.bam", [*extra, "--markdup"])
    for tag, env in (("qm", None), ("qmn", dict(BM_SORT_RUN_BYTES="2000"))):
        errm = run_tool(exe, d, args, f"{name}.{tag}.bam", [*extra, "--markdup", "--stats", f"{name}.{tag}.txt"], env=env)
        m_text, m_told, m_t = stats_by_the_rule(d / f"{name}.{tag}.bam")
        assert (d / f"{name}.{tag}.txt").read_text() == m_text and stats_line(errm) == m_told and pair_of(d, f"{name}.{tag}") == pair_of(d, f"{name}.qm0")
        marked = MARKED.search(errm)
        assert m_t[Q.T["duplicates"]] == int(marked.group(1)) > 0 and m_t[Q.T["records"]] == int(marked.group(2)) == t[Q.T["records"]]
    # other sizes of the tables, and beside every other file of the sorter
    run_tool(exe, d, args, f"{name}.qs.bam", [*extra, "--stats", f"{name}.qs.txt", "--stats-max-cycle", "100", "--stats-max-insert=500"])
    assert (d / f"{name}.qs.txt").read_text() == stats_by_the_rule(d / f"{name}.qs.bam", max_cycle=100, max_insert=500)[0] != text
    others = ["--depth", f"{name}.qa.bedgraph", "--pileup", f"{name}.qa.tsv", "--vcf", f"{name}.qa.vcf", "--vcf-indels", "--vcf-phase"]
    run_tool(exe, d, args, f"{name}.qa0.bam", [*extra, *[o.replace(".qa.", ".qa0.") for o in others]])
    erra = run_tool(exe, d, args, f"{name}.qa.bam", [*extra, *others, "--stats", f"{name}.qa.txt"])
    assert (d / f"{name}.qa.txt").read_text() == text and stats_line(erra) == told
    for ext in ("bam", "bam.bai", "bedgraph", "tsv", "vcf"):
        assert (d / f"{name}.qa.{ext}").read_bytes() == (d / f"{name}.qa0.{ext}").read_bytes(), ext


# ---- the command line ----
def test_cli_refusals(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        run = lambda *opts: subprocess.run([exe, "-i", "idx", *opts], cwd=str(tmp_path), capture_output=True, text=True)
        fine = lambda r: "Validation failed" not in r.stderr and "Unknown option" not in r.stderr and "Value parse failed" not in r.stderr
        r = run("--stats", "s.txt", "-o", "x.sam")
        assert r.returncode != 0 and "Validation failed for option --stats: only BAM output is sorted and indexed; write -o x.bam instead of -o x.sam." in r.stderr, r.stderr
        r = run("--stats", "s.txt", "--markdup", "-o", "x.sam")                 # an earlier name of the chain keeps its message
        assert r.returncode != 0 and "Validation failed for option --markdup: only BAM output" in r.stderr
        r = run("--sort", "-o", "x.sam")
        assert r.returncode != 0 and "Validation failed for option --sort: only BAM output" in r.stderr
        r = run("--stats", "s.txt")
        assert r.returncode != 0 and "Validation failed for option --stats" in r.stderr and "-o x.bam" in r.stderr, r.stderr
        r = run("--stats")
        assert r.returncode != 0 and "Missing value" in r.stderr
        assert fine(run("-o", "x.bam", "--stats", "s.txt")) and fine(run("-o", "x.bam", "--stats=s.txt", "--stats-max-cycle", "300", "--stats-max-insert", "1000"))
        assert fine(run("-o", "x.bam", "--stats", "s.txt", "--vcf", "v.vcf", "--gvcf", "g.vcf", "--vcf-indels", "--vcf-bias", "--vcf-phase", "--markdup", "--pileup", "p.tsv",
                        "--depth", "d.txt", "--coverage", "c.txt"))
        for other in ("--depth", "--coverage", "--pileup", "--vcf", "--gvcf"):
            r = run("-o", "x.bam", other, "same.txt", "--stats", "same.txt")
            assert r.returncode != 0 and f"Validation failed for option --stats: same.txt is the file of {other} too." in r.stderr, r.stderr
        for opt in ("--stats-max-cycle", "--stats-max-insert"):
            r = run("-o", "x.bam", opt, "100")
            assert r.returncode != 0 and f"Validation failed for option {opt}" in r.stderr and "--stats FILE" in r.stderr, r.stderr
            r = run("-o", "x.bam", "--stats", "s.txt", opt)
            assert r.returncode != 0 and "Missing value" in r.stderr
            for bad in ("x", "-1", "", "0", "65536", "1.5", "2e2"):
                r = run("-o", "x.bam", "--stats", "s.txt", opt, bad)
                assert r.returncode != 0 and "Value parse failed for " + opt in r.stderr, (opt, bad, r.stderr)
                assert "1..65535" in r.stderr or bad in ("x", "", "1.5", "2e2"), (opt, bad, r.stderr)
            assert all(fine(run("-o", "x.bam", "--stats", "s.txt", opt, good)) for good in ("1", "65535"))
        assert not os.listdir(tmp_path)


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import stats
    header = open(os.path.join(ROOT, "include", "bmq.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = sorted(set(re.findall(r"\b(bmq_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(stats.SYMBOLS) and len(names) == 8
    assert not re.search(r"\bbmf_", text)
    L = stats.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    assert (stats.N_TALLIES, stats.N_TABLES) == (Q.N_TALLIES, len(Q.TABLES)) and stats.DEFAULTS == Q.DEFAULTS and tuple(stats.PARAMS) == tuple(Q.DEFAULTS)
    assert stats.TABLES == Q.TABLES and stats.WIDTH == tuple(Q.WIDTH[n] for n in Q.TABLES)
    assert re.search(r"BMQ_N_TALLIES = 35, BMQ_N_TABLES = 8, BMQ_MAX_LDS_CYCLES = (\d+)", text).group(1) == str(stats.MAX_LDS_CYCLES)
    enum = re.search(r"BMQ_RECORDS = 0.*?\}", text, flags=re.S).group(0)
    assert [n.lower() for n in re.findall(r"BMQ_([A-Z0-9_]+) = \d+", enum)] == list(Q.NAMES)          # the tallies' names, in order
    assert [int(v) for v in re.findall(r"BMQ_[A-Z0-9_]+ = (\d+)", enum)] == list(range(35))
    assert [f"BMQ_T_{n} = {k}" in text for k, n in enumerate(Q.TABLES)] == [True] * 8
    for word in ("LEFT OUT, on purpose", "NM/MD", "read groups", "counts per reference", "per tile or\n * lane", "GC against depth", "threshold on mapq or quality",
                 "secondary and supplementary records in the read-level tables", "another tool's parser", "Hard clips do not shift cycles", "BMQ_LDS_CYCLES"):
        assert word in header, word


def test_argument_errors_need_no_device():
    from bucket_map_amd import stats
    L = stats.lib()
    u8p, u32p, u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64))
    err = lambda: L.bmq_last_error().decode()
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
        return L.bmq_add(None, p["a"], len(stream), p["o"], n, None)

    for name, (stream, off, n, word) in cases.items():
        assert add(stream, off, n) == stats.BMQ_ERR_ARG, name
        assert word in err() and "bmq_add" in err(), (name, err())
    for null in ("a", "o"):
        assert add(good, good_off, 2, null=(null,)) == stats.BMQ_ERR_ARG and "null argument" in err()
    assert add(good, good_off, 2) == stats.BMQ_ERR_ARG and "null context" in err()
    far = bytearray(good)                                # a refID beyond any reference is no error here: the context is what is missing
    far[4:8] = (12345).to_bytes(4, "little")
    assert add(bytes(far), good_off, 2) == stats.BMQ_ERR_ARG and "null context" in err()
    assert add(b"", [0], 0) == stats.BMQ_ERR_ARG and "null context" in err()

    def begin(max_cycle=1024, max_insert=8000):
        pr = np.array([max_cycle, max_insert], np.uint32)
        return L.bmq_begin(None, pr.ctypes.data_as(u32p))

    assert L.bmq_begin(None, None) == stats.BMQ_ERR_ARG and "null argument" in err()
    for bad, word in ((dict(max_cycle=0), "max_cycle"), (dict(max_cycle=65536), "max_cycle"), (dict(max_insert=0), "max_insert"), (dict(max_insert=65536), "max_insert")):
        assert begin(**bad) == stats.BMQ_ERR_ARG and word in err() and "1 .. 65535" in err()
    for good_pr in (dict(), dict(max_cycle=1, max_insert=1), dict(max_cycle=65535, max_insert=65535)):
        assert begin(**good_pr) == stats.BMQ_ERR_ARG and "null context" in err()          # good data: only the context is missing
    out = np.zeros(64, np.uint64)
    assert L.bmq_table(None, 0, 0, 1, None) == stats.BMQ_ERR_ARG and "null argument" in err()
    assert L.bmq_table(None, 0, 0, 1, out.ctypes.data_as(u64p)) == stats.BMQ_ERR_ARG and "null context" in err()
    assert L.bmq_table(None, 0, 0, 0, None) == stats.BMQ_ERR_ARG and "null context" in err()
    assert L.bmq_finish(None, None) == stats.BMQ_ERR_ARG and "null context" in err()
    assert L.bmq_create(0, None) == stats.BMQ_ERR_ARG and L.bmq_last_stats(None, None, None) == stats.BMQ_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import stats
    with pytest.raises(stats.BmqError) as e:
        stats.Stats(0)
    assert e.value.code == stats.BMQ_ERR_HIP
