"""Coverage (-o x.bam --depth FILE --coverage FILE) without a GPU: host/depth.h as a program of its own under ASan + UBSan, the
oracle-backed tools (whose counting is the host default of block_compressor), the command line and the bmc_* ABI surface.

The yardstick is the rule of include/bmc.h in plain Python (tests/depth_rule.py), applied to the records decoded from the
x.bam the tool wrote: the two files are a function of those records alone.
"""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import depth_rule as D
from depth_cases import EDGE_REFS, REF_LENS, edge_records, many_ops_record, op, parse_check_output, random_records
from test_bamsort import offsets_of, pair_of, records_of, run_tool
from test_markdup_gpu import rec, rec_ops
from test_sam_golden import ROOT, TOOLS

COVERAGE = re.compile(r"Coverage: (\d+) of (\d+) bases covered by (\d+) records \((\d+) long-CIGAR records left out\)")


# ---- the rule itself, on cases worked out by hand ----
def test_python_restatement_of_the_rule():
    recs = edge_records()
    res = D.count(recs, EDGE_REFS)
    by_name = {r[36: 36 + r[12] - 1]: i for i, r in enumerate(recs)}
    only = lambda *names: D.count([recs[by_name[n]] for n in names], EDGE_REFS)
    assert only(b"to_the_end").runs == [(0, 990, 1000, 1)]
    one = only(b"one_past")
    assert one.runs == [(0, 991, 1000, 1)] and one.stats[0] == [1, 9, 9, 30, sum(range(30, 39)), 9, 0]
    far = only(b"hundred_past")
    assert far.runs == [(0, 950, 1000, 1)] and far.stats[0][4:6] == [sum((50 + k) % 200 for k in range(50)), 50]
    assert only(b"last_base").runs == [(0, 999, 1000, 1)] and only(b"on_one_base").runs == [(2, 0, 1, 1)]
    assert only(b"block_beyond").runs == [(0, 995, 998, 1)] and only(b"block_beyond").stats[0][4:6] == [11 + 12 + 13, 3]
    assert only(b"insert_then_clip").stats[0][4:6] == [60 + 61 + 64 + 65, 4]
    for name in (b"pos_is_len", b"pos_negative", b"no_reference", b"no_cigar", b"flag4", b"flag100", b"flag200", b"flag400", b"placeholder_dup"):
        got = only(name)
        assert got.runs == [] and got.stats == [[0] * 7] * 3, name
    for name in (b"clips_only", b"hard_and_soft", b"pads_only", b"insert_only"):
        got = only(name)
        assert got.runs == [] and got.stats[0] == [1, 0, 0, 30, 0, 0, 0], name
    assert only(b"flag800").runs == [(1, 10, 15, 1)]
    assert only(b"eq_x_eq").runs == [(0, 20, 30, 1)] and only(b"empty_blocks").runs == [(0, 40, 45, 1)]
    assert only(b"abut_a", b"abut_b").runs == [(0, 100, 120, 1)]
    assert only(b"abut_c", b"abut_d", b"abut_e").runs == [(0, 200, 210, 1), (0, 210, 220, 2)]
    assert only(b"gaps").runs == [(0, 300, 304, 1), (0, 307, 311, 1), (0, 313, 317, 1)]
    assert only(b"no_qualities").stats[0] == [1, 8, 8, 30, 0, 0, 0] and only(b"some_qualities").stats[0][4:6] == [264, 4]
    assert only(b"no_sequence").stats[0] == [1, 8, 8, 30, 0, 0, 0]
    assert only(b"placeholder").stats[1] == [0, 0, 0, 0, 0, 0, 1] and only(b"placeholder").runs == []
    assert only(b"no_placeholder").stats[1] == [1, 0, 0, 30, 0, 0, 0]
    assert {len(r) % 16 for r in recs} == set(range(16))
    assert res.stats[0][6] == 0 and res.stats[1][6] == 1 and len(res.runs) > 20
    assert sum(int(d.sum()) for d in res.depth) == sum(s[2] for s in res.stats)
    assert D.depth_text(only(b"abut_a"), ["a", "b", "c"]) == "a\t100\t110\t1\n"
    assert D.coverage_text(only(b"abut_a"), ["a", "b", "c"], EDGE_REFS).split("\n")[1:3] == [
        "a\t1\t1000\t1\t10\t1.0000\t0.0100\t24.5000\t30.0000", "b\t1\t50\t0\t0\t0.0000\t0.0000\t0.0000\t0.0000"]
    assert D.refused([rec_ops(0, 1, 0, [op(3, "M") | 9], b"")], 3) and D.refused([rec(0, 1, 0, "3M", b"ab")], 3)
    assert D.refused([rec(3, 1, 0, "3M", b"")], 3) and D.refused([rec(3, 1, 4, "3M", b"")], 3) is None


# ---- host/depth.h as a program of its own ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_check")
    exe = str(d / "depth_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "depth_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_check(checker, recs, ref_len, n_calls=1, seed=0, skip=None, expect=0):
    d, exe = checker
    (d / "records.bin").write_bytes(b"".join(recs))
    if skip is not None:
        (d / "skip.bin").write_bytes(bytes(skip))
    r = subprocess.run([exe, "records.bin", "skip.bin" if skip is not None else "-", str(n_calls), str(seed), *[str(x) for x in ref_len]],
                       cwd=str(d), capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode == expect, r.stderr[-3000:]
    return r.stdout


def same_as_rule(out, want):
    runs, stats, depth = parse_check_output(out)
    assert stats == want.stats
    assert runs == want.runs
    assert depth == [d.tolist() for d in want.depth]


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1025, 20001])
def test_host_rule_is_the_python_rule(checker, n):
    recs = random_records(n, 300 + n)
    want = D.count(recs, REF_LENS)
    if n >= 257:
        assert all(s[0] for s in want.stats[1:]) and sum(s[6] for s in want.stats) == 0 and len(want.runs) > 50
    one = run_check(checker, recs, REF_LENS)
    same_as_rule(one, want)
    if n in (2, 65, 1025):                               # order and cutting do not matter
        assert run_check(checker, recs, REF_LENS, n_calls=3) == one
        assert run_check(checker, recs, REF_LENS, n_calls=7, seed=n) == one


def test_host_rule_on_the_edges_and_a_record_of_many_ops(checker):
    recs = edge_records()
    one = run_check(checker, recs, EDGE_REFS)
    same_as_rule(one, D.count(recs, EDGE_REFS))
    assert run_check(checker, recs, EDGE_REFS, n_calls=5, seed=3) == one
    refs = [90000, 300]
    recs = random_records(40, 5, refs) + [many_ops_record(0, 17)] + random_records(40, 6, refs) + [many_ops_record(0, 60000, with_sequence=False)]
    want = D.count(recs, refs)
    assert want.stats[0][2] > 50000 and want.stats[0][5] > 50000
    same_as_rule(run_check(checker, recs, refs), want)


def test_host_skip_bytes_equal_removing_the_records(checker):
    recs = random_records(500, 77)
    skip = [int(k % 3 == 1) for k in range(500)]
    want = D.count(recs, REF_LENS, skip)
    assert want.stats != D.count(recs, REF_LENS).stats
    kept = [r for r, s in zip(recs, skip) if not s]
    assert D.count(kept, REF_LENS).runs == want.runs and D.count(kept, REF_LENS).stats == want.stats
    same_as_rule(run_check(checker, recs, REF_LENS, skip=skip), want)
    assert run_check(checker, recs, REF_LENS, n_calls=4, seed=9, skip=skip) == run_check(checker, kept, REF_LENS)


def test_host_rule_refuses_what_the_abi_refuses(checker):
    good = random_records(10, 1)
    for bad in (rec_ops(0, 0, 0, [3 << 4 | 9], b""), rec(1, 5, 0, "3M", b"ab"), rec(6, 5, 0, "3M", b""), rec(1, 5, 0, "3M2I", b"abcd")):
        assert D.refused([bad], len(REF_LENS))
        assert run_check(checker, good + [bad], REF_LENS, expect=3).startswith("refused ")
    assert "runs" in run_check(checker, good + [rec(6, 5, 4, "3M", b"")], REF_LENS)      # unmapped: its reference is not looked at
    assert run_check(checker, good, [5, 0, 5], expect=3).startswith("refused ")                  # a reference without bases


# ---- the oracle-backed tools ----
def header_refs(raw):
    """[(name, length)] of an inflated BAM file."""
    l_text = struct.unpack_from("<I", raw, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<I", raw, at)[0]
    at += 4
    out = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<I", raw, at)[0]
        out.append((raw[at + 4: at + 4 + l_name - 1].decode(), struct.unpack_from("<I", raw, at + 4 + l_name)[0]))
        at += 8 + l_name
    return out


def files_by_the_rule(bam_path):
    """(the --depth text, the --coverage text, the rule's result) for the records of a BAM file."""
    raw = gzip.decompress(open(bam_path, "rb").read())
    refs = header_refs(raw)
    recs = [r for _, r in records_of(raw)[0]]
    names, lens = [n for n, _ in refs], [l for _, l in refs]
    res = D.count(recs, lens)
    return D.depth_text(res, names), D.coverage_text(res, names, lens), res


def parse_coverage_line(err):
    found = COVERAGE.findall(err)
    assert len(found) == 1, err
    return tuple(int(x) for x in found[0])


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_markdup import markdup_jobs
    return markdup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", range(3))
def test_oracle_tool_writes_what_the_rule_says(jobs, k):
    name, which, d, args, extra = jobs[k]
    exe = TOOLS[(which, "oracle")]
    err = run_tool(exe, d, args, f"{name}.ds.bam", [*extra, "--sort"])
    assert "Coverage:" not in err
    err = run_tool(exe, d, args, f"{name}.d.bam", [*extra, "--depth", f"{name}.d.bedgraph", "--coverage", f"{name}.d.cov"])
    assert re.search(r"Sorted \d+ records by coordinate in 1 run", err)
    assert pair_of(d, f"{name}.d") == pair_of(d, f"{name}.ds")                   # the BAM and its index are what they were
    depth, cov, res = files_by_the_rule(d / f"{name}.d.bam")
    assert (d / f"{name}.d.bedgraph").read_text() == depth and (d / f"{name}.d.cov").read_text() == cov
    aligned = name != "plain"                            # the plain tool writes no CIGAR: records without depth, an empty file
    if aligned:
        assert len(res.runs) > 10 and max(r[3] for r in res.runs) > 1 and sum(s[5] for s in res.stats) > 0
    else:
        assert depth == "" and cov.count("\n") == 1 + len(res.stats) and not any(any(s) for s in res.stats)
    total = [sum(s[j] for s in res.stats) for j in range(7)]
    assert parse_coverage_line(err) == (total[1], sum(l for l in [len(x) for x in res.depth]), total[0], total[6])
    # either option alone
    run_tool(exe, d, args, f"{name}.d1.bam", [*extra, "--depth", f"{name}.d1.bedgraph"])
    run_tool(exe, d, args, f"{name}.d2.bam", [*extra, "--coverage", f"{name}.d2.cov", "--sort"])
    assert (d / f"{name}.d1.bedgraph").read_text() == depth and (d / f"{name}.d2.cov").read_text() == cov
    assert not os.path.exists(d / f"{name}.d1.cov") and pair_of(d, f"{name}.d1") == pair_of(d, f"{name}.ds") == pair_of(d, f"{name}.d2")
    # several runs: the same two files
    err = run_tool(exe, d, args, f"{name}.dr.bam", [*extra, "--depth", f"{name}.dr.bedgraph", "--coverage", f"{name}.dr.cov"],
                   env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1
    assert (d / f"{name}.dr.bedgraph").read_text() == depth and (d / f"{name}.dr.cov").read_text() == cov
    assert pair_of(d, f"{name}.dr") == pair_of(d, f"{name}.ds")
    # with --markdup the duplicates are left out: the rule on the marked records, and other files than before
    run_tool(exe, d, args, f"{name}.dm0.bam", [*extra, "--markdup"])
    err = run_tool(exe, d, args, f"{name}.dm.bam", [*extra, "--markdup", "--depth", f"{name}.dm.bedgraph", "--coverage", f"{name}.dm.cov"])
    assert pair_of(d, f"{name}.dm") == pair_of(d, f"{name}.dm0")
    m_depth, m_cov, m_res = files_by_the_rule(d / f"{name}.dm.bam")
    assert (d / f"{name}.dm.bedgraph").read_text() == m_depth and (d / f"{name}.dm.cov").read_text() == m_cov
    assert not aligned or (m_depth != depth and m_cov != cov and sum(s[0] for s in m_res.stats) < total[0])
    err = run_tool(exe, d, args, f"{name}.dmr.bam", [*extra, "--markdup", "--depth", f"{name}.dmr.bedgraph", "--coverage", f"{name}.dmr.cov"],
                   env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1
    assert (d / f"{name}.dmr.bedgraph").read_text() == m_depth and (d / f"{name}.dmr.cov").read_text() == m_cov
    assert pair_of(d, f"{name}.dmr") == pair_of(d, f"{name}.dm0")


# ---- the command line ----
def test_cli_refuses_sam_and_no_output(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        for opt in ("--depth", "--coverage"):
            r = subprocess.run([exe, "-i", "idx", opt, "d.txt", "-o", "x.sam"], cwd=str(tmp_path), capture_output=True, text=True)
            assert r.returncode != 0 and "x.bam" in r.stderr and opt in r.stderr and not os.listdir(tmp_path), r.stderr
            assert "only BAM output is sorted and indexed" in r.stderr
            r = subprocess.run([exe, "-i", "idx", opt, "d.txt"], cwd=str(tmp_path), capture_output=True, text=True)
            assert r.returncode != 0 and "-o x.bam" in r.stderr and opt in r.stderr and not os.listdir(tmp_path), r.stderr
            r = subprocess.run([exe, "-i", "idx", opt], cwd=str(tmp_path), capture_output=True, text=True)
            assert r.returncode != 0 and "Missing value" in r.stderr
            r = subprocess.run([exe, "-i", "idx", "-o", "x.bam", opt, "d.txt"], cwd=str(tmp_path), capture_output=True, text=True)
            assert "Validation failed" not in r.stderr and "Unknown option" not in r.stderr
        r = subprocess.run([exe, "-i", "idx", "-o", "x.bam", "--depth", "d.txt", "--coverage", "d.txt"], cwd=str(tmp_path), capture_output=True, text=True)
        assert r.returncode != 0 and "--coverage" in r.stderr and "Validation failed" in r.stderr


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import depth
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmc.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bmc_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(depth.SYMBOLS) and len(names) == 9
    L = depth.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    for n in ("bmc_create", "bmc_destroy", "bmc_last_error", "bmc_begin", "bmc_add", "bmc_finish", "bmc_runs", "bmc_depth_at", "bmc_last_stats"):
        assert n in names


def full_record(l_name=2, n_cigar=1, l_seq=4, room=0, ops=None):
    body = struct.pack("<iiBBHHHIiii", 0, 5, l_name, 0, 4680, n_cigar, 0, l_seq, -1, -1, 0) + bytes(l_name)
    body += struct.pack(f"<{n_cigar}I", *(ops if ops is not None else [0] * n_cigar)) + bytes((l_seq + 1) // 2 + l_seq + room)
    return struct.pack("<I", len(body)) + body


def test_argument_errors_need_no_device():
    from bucket_map_amd import depth
    L = depth.lib()
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
        return L.bmc_add(None, p["a"], len(stream), p["o"], n, s.ctypes.data_as(u8p) if skip else None)

    for name, (stream, off, n, word) in cases.items():
        assert add(stream, off, n) == depth.BMC_ERR_ARG, name
        assert word in L.bmc_last_error().decode(), (name, L.bmc_last_error())
    for null in ("a", "o"):
        assert add(good, good_off, 2, null=(null,)) == depth.BMC_ERR_ARG and "null argument" in L.bmc_last_error().decode()
    for skip in (True, False):                           # good data: only the context is missing
        assert add(good, good_off, 2, skip=skip) == depth.BMC_ERR_ARG and "null context" in L.bmc_last_error().decode()
    assert add(b"", [0], 0) == depth.BMC_ERR_ARG and "null context" in L.bmc_last_error().decode()
    # a D or N of any length, H and P take no query bases; no CIGAR or no sequence: nothing to compare
    fine = [full_record(2, 3, 4, ops=[4 << 4, 900 << 4 | 2, 7 << 4 | 5]), full_record(2, 0, 4), full_record(2, 1, 0, ops=[9 << 4])]
    assert add(b"".join(fine), offsets_of(fine), 3) == depth.BMC_ERR_ARG and "null context" in L.bmc_last_error().decode()

    def begin(lens, n=None, null=False):
        a = np.asarray(lens, np.uint32)
        return L.bmc_begin(None, None if null else a.ctypes.data_as(u32p), len(lens) if n is None else n)

    assert begin([5], n=0) == depth.BMC_ERR_ARG and "n_ref is 0" in L.bmc_last_error().decode()
    assert begin([5, 0, 7]) == depth.BMC_ERR_ARG and "reference 1 has the length 0" in L.bmc_last_error().decode()
    assert begin([2 ** 32 - 2 ** 20, 1]) == depth.BMC_ERR_ARG and "2^32 - 2^20" in L.bmc_last_error().decode()
    assert begin([2 ** 31, 2 ** 31]) == depth.BMC_ERR_ARG and "2^32 - 2^20" in L.bmc_last_error().decode()
    assert begin([5], null=True) == depth.BMC_ERR_ARG and "null argument" in L.bmc_last_error().decode()
    assert begin([2 ** 32 - 2 ** 20]) == depth.BMC_ERR_ARG and "null context" in L.bmc_last_error().decode()
    assert begin([1]) == depth.BMC_ERR_ARG and "null context" in L.bmc_last_error().decode()
    n_runs, stats, out = C.c_uint64(0), np.zeros(7, np.uint64), np.zeros(4, np.uint32)
    assert L.bmc_finish(None, None, stats.ctypes.data_as(u64p)) == depth.BMC_ERR_ARG and "null argument" in L.bmc_last_error().decode()
    assert L.bmc_finish(None, C.byref(n_runs), None) == depth.BMC_ERR_ARG and "null argument" in L.bmc_last_error().decode()
    assert L.bmc_finish(None, C.byref(n_runs), stats.ctypes.data_as(u64p)) == depth.BMC_ERR_ARG and "null context" in L.bmc_last_error().decode()
    assert L.bmc_runs(None, 0, 1, None) == depth.BMC_ERR_ARG and "null argument" in L.bmc_last_error().decode()
    assert L.bmc_runs(None, 0, 1, out.ctypes.data_as(u32p)) == depth.BMC_ERR_ARG and "null context" in L.bmc_last_error().decode()
    assert L.bmc_depth_at(None, 0, 0, 1, None) == depth.BMC_ERR_ARG and "null argument" in L.bmc_last_error().decode()
    assert L.bmc_depth_at(None, 0, 0, 1, out.ctypes.data_as(u32p)) == depth.BMC_ERR_ARG and "null context" in L.bmc_last_error().decode()
    assert L.bmc_create(0, None) == depth.BMC_ERR_ARG and L.bmc_last_stats(None, None, None) == depth.BMC_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import depth
    with pytest.raises(depth.BmcError) as e:
        depth.Depth(0)
    assert e.value.code == depth.BMC_ERR_HIP
