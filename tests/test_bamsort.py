"""Coordinate-sorted BAM with a .bai index (-o x.bam --sort) without a GPU: host/bam_sort.h as a program of its own under
ASan + UBSan, the oracle-backed tools (whose sort is the host default of block_compressor: std::stable_sort on the key of
include/bms.h), the sanitized tools, and the bms_* ABI surface.

The yardsticks are the SAM specification and plain Python: the expected order is sorted() on (refID as u32, POS) with the
input order breaking ties, the index is read by tests/bai_reader.py, and every region query through the index is compared
with a brute-force scan of all records.
"""
import ctypes as C
import glob
import json
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import bai_reader as B
from test_bgzf import RUNS, bam_to_sam, fold_seq, golden_args, split_blocks
from test_pair import ARGS as PAIR_ARGS, make_paired_fixture
from test_sam_golden import ROOT, TOOLS, write_inputs

REFS = [("chr1", 2 ** 29 + 1000), ("chr2", 200000), ("chr3", 5000)]
HEADER = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in REFS)
SORTED_HD = "@HD\tVN:1.6\tSO:coordinate\n"


# ---- synthetic minimal records, shared with tests/test_bamsort_gpu.py ----
def make_record(rid, pos, name=b"r", filler=b"", flag=0):
    """A BAM record with no CIGAR and no bases: block_size, the 32 fixed bytes, the name, then filler (as if tags)."""
    body = struct.pack("<iiBBHHHIiii", rid, pos, len(name) + 1, 0, 4680, 0, flag, 0, -1, -1, 0) + name + b"\0" + filler
    return struct.pack("<I", len(body)) + body


def offsets_of(records):
    out = [0]
    for r in records:
        out.append(out[-1] + len(r))
    return out


def key_of(rec):
    rid, pos = struct.unpack_from("<II", rec, 4)
    return rid << 32 | (pos + 1) & 0xFFFFFFFF


def sort_reference(records):
    """(perm, the sorted stream, sorted_offset) as include/bms.h defines them."""
    keys = [key_of(r) for r in records]
    perm = sorted(range(len(records)), key=lambda i: (keys[i], i))
    return perm, b"".join(records[i] for i in perm), offsets_of([records[i] for i in perm])


# ---- the hand-written SAM ----
def hand_sam():
    rng = random.Random(20241020)
    recs = []

    def add(name, flag, ref, pos0, cigar, qlen, tags=""):
        seq = "".join(rng.choice("ACGT") for _ in range(qlen)) or "*"
        qual = "I" * qlen if qlen else "*"
        recs.append(f"{name}\t{flag}\t{ref}\t{pos0 + 1}\t30\t{cigar}\t*\t0\t0\t{seq}\t{qual}{tags}\n")

    for p in (2 ** 14, 2 ** 17, 2 ** 20, 2 ** 23, 2 ** 26):        # the bin borders: a record across each and one at it
        for pos0 in (p - 4, p):
            add(f"border{pos0}", 16, "chr1", pos0, "4M1D2I2S", 8, "\tNM:i:3")
    ops = "".join(f"1{'=X'[i % 2]}" for i in range(70000))           # a long CIGAR: the CG:B,I convention, 5 windows
    recs.append(f"long\t0\tchr1\t7\t60\t{ops}\t*\t0\t0\t{'ACGT' * 17500}\t*\tNM:i:35000\n")
    for k in (1, 2, 5, 9):                                           # two 16 kbp windows each
        add(f"span{k}", 0, "chr2", 16384 * k - 50, "100M", 100)
    add("ends_on_border", 0, "chr2", 16384 * 3 - 100, "100M", 100)   # its last base is 16383 of its window
    for g, (ref, pos0) in enumerate((("chr1", 1000), ("chr2", 16383), ("chr2", 16384), ("chr3", 0), ("chr1", 2 ** 26))):
        for k in range(5):                                           # equal keys: the input order must survive
            add(f"tie{g}.{k}", 16 * (k % 2), ref, pos0, "10M", 10)
    for k in range(6):                                               # unmapped mates placed beside their partners
        add(f"placed_unmapped{k}", 4, "chr2", 40000 + 7000 * k, "*", 12)
    for k in range(7):
        recs.append(f"nowhere{k}\t4\t*\t0\t0\t*\t*\t0\t0\tACGTN\tIIIII\n")
    while len(recs) < 400:
        ref, top = rng.choice((("chr1", 2 ** 27), ("chr2", 199000), ("chr2", 199000), ("chr3", 4900)))
        m = rng.choice((1, 36, 100, 151))
        cigar, qlen = rng.choice(((f"{m}M", m), (f"5S{m}M", m + 5), (f"{m}M2D{m}M", 2 * m), (f"{m}=1X3I", m + 4)))
        add(f"read{len(recs)}", rng.choice((0, 16)), ref, rng.randrange(top), cigar, qlen, rng.choice(("", "\tNM:i:1\tMD:Z:5A5")))
    rng.shuffle(recs)
    return recs


def sam_key(line):
    f = line.split("\t")
    rid = [n for n, _ in REFS].index(f[2]) if f[2] != "*" else 0xFFFFFFFF
    return rid << 32 | int(f[3])


def expected_text(lines):
    order = sorted(range(len(lines)), key=lambda i: (sam_key(lines[i]), i))
    return fold_seq(SORTED_HD + HEADER.split("\n", 1)[1] + "".join(lines[i] for i in order))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_sort_check")
    exe = str(d / "bam_sort_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "bam_sort_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_check(checker, lines, stem, run_bytes=None):
    d, exe = checker
    (d / f"{stem}.sam").write_text(HEADER + "".join(lines))
    r = subprocess.run([exe, f"{stem}.sam", f"{stem}.bam", *([str(run_bytes)] if run_bytes else [])], cwd=str(d), capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode == 0, r.stderr[-3000:]
    assert not glob.glob(str(d / "*.tmp")), "a run file was left behind"
    n_records, n_runs = (int(x) for x in r.stdout.split())
    return (d / f"{stem}.bam").read_bytes(), (d / f"{stem}.bam.bai").read_bytes(), n_records, n_runs


# ---- what a sorted file and its index must satisfy ----
def records_of(raw):
    """[(stream offset, record bytes)] and the length of the BAM header in raw."""
    l_text = struct.unpack_from("<I", raw, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<I", raw, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<I", raw, at)[0]
    head, out = at, []
    while at < len(raw):
        size = 4 + struct.unpack_from("<I", raw, at)[0]
        out.append((at - head, raw[at: at + size]))
        at += size
    assert at == len(raw)
    return out, head, n_ref


def check_sorted_file(bam, bai, regions_per_ref, seed=1):
    """Everything the issue asks of one x.bam / x.bam.bai pair; returns the records in file order."""
    import gzip
    raw = gzip.decompress(bam)
    recs, head, n_ref = records_of(raw)
    keys = [key_of(r) for _, r in recs]
    assert keys == sorted(keys)
    assert raw[8:].startswith(SORTED_HD.encode())
    # virtual offsets by the stated formula, from the file's own BSIZE fields
    blocks = split_blocks(bam)
    file_at, sizes, at = [], [], 0
    for b in blocks:
        file_at.append(at)
        sizes.append(struct.unpack_from("<I", b, len(b) - 4)[0])
        at += len(b)
    n_head, got = 0, 0
    while got < head:
        got += sizes[n_head]
        n_head += 1
    assert got == head, "the header shares a block with records"
    assert all(s == B.BLOCK_MAX for s in sizes[n_head: -2]) and sizes[-1] == 0

    def vo(so):
        return file_at[n_head + so // B.BLOCK_MAX] << 16 | so % B.BLOCK_MAX
    total = len(raw) - head
    starts = {vo(so) for so, _ in recs}
    ends = starts | {vo(total)}
    index = B.parse_bai(bai)
    assert len(index["refs"]) == n_ref
    spans = [B.record_span(r) for _, r in recs]
    for ref, r in enumerate(index["refs"]):
        mine = [k for k, s in enumerate(spans) if s[0] == ref]
        assert r["bin_order"] == sorted(r["bin_order"])
        for chunks in r["bins"].values():
            for beg, end in chunks:
                assert beg in starts and end in ends and beg < end
        assert r["linear"] == sorted(r["linear"])
        if not mine:
            assert r["bin_order"] == [] and r["linear"] == [] and r["pseudo"] is None
            continue
        first, last = recs[mine[0]], recs[mine[-1]]
        assert r["pseudo"] == (vo(first[0]), vo(last[0] + len(last[1])), sum(1 for k in mine if not spans[k][3] & 4),
                               sum(1 for k in mine if spans[k][3] & 4))
        assert len(r["linear"]) == max((spans[k][2] - 1) >> 14 for k in mine) + 1
        for w, io in enumerate(r["linear"]):                      # the first record overlapping w, or the next touched window's
            over = [k for k in mine if spans[k][1] < (w + 1) << 14 and spans[k][2] > w << 14]
            if over:
                assert io == vo(recs[over[0]][0]), (ref, w)
            else:
                assert io == r["linear"][w + 1], (ref, w)
        # one chunk per maximal run of consecutive records with the same bin
        want = {}
        prev = None
        for k in mine:
            b = struct.unpack_from("<H", recs[k][1], 14)[0]
            so, size = recs[k][0], len(recs[k][1])
            if prev == (b, k - 1):
                want[b][-1][1] = vo(so + size)
            else:
                want.setdefault(b, []).append([vo(so), vo(so + size)])
            prev = (b, k)
        assert {b: [tuple(c) for c in cs] for b, cs in want.items()} == r["bins"]
    assert index["n_no_coor"] == sum(1 for s in spans if s[0] < 0)
    # region queries through the index against a scan of everything
    rng = random.Random(seed)
    file = B.Bgzf(bam)
    lengths = read_ref_lengths(raw)
    for ref in range(n_ref):
        mine = [k for k, s in enumerate(spans) if s[0] == ref]
        top = min(lengths[ref], 2 ** 29)
        regions = [(0, top), (16383, 16384), (16384, 16385), (16383, 16385)]
        if regions_per_ref is None:                                # every record's first base, last base and the one after
            for k in mine:
                regions += [(p, p + 1) for p in (spans[k][1], spans[k][2] - 1, spans[k][2]) if p < top]
            n_random = 200
        else:
            n_random = regions_per_ref
        for _ in range(n_random):
            a = rng.randrange(top)
            regions.append((a, min(top, a + rng.choice((1, 50, 1000, 20000, 2 ** 21)))))
        for beg, end in regions:
            want = [recs[k][1] for k in mine if spans[k][1] < end and spans[k][2] > beg]
            assert B.fetch(file, index, ref, beg, end) == want, (ref, beg, end)
    return [r for _, r in recs]


def read_ref_lengths(raw):
    l_text = struct.unpack_from("<I", raw, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<I", raw, at)[0]
    at += 4
    out = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<I", raw, at)[0]
        out.append(struct.unpack_from("<I", raw, at + 4 + l_name)[0])
        at += 8 + l_name
    return out


# ---- host/bam_sort.h under ASan + UBSan ----
def test_hand_written_sam_sorted_and_indexed(checker):
    lines = hand_sam()
    assert len(lines) == 400
    bam, bai, n_records, n_runs = run_check(checker, lines, "hand")
    assert (n_records, n_runs) == (400, 1)
    d = checker[0]
    text, _ = bam_to_sam(d / "hand.bam")
    assert text == expected_text(lines)
    recs = check_sorted_file(bam, bai, None)
    assert len(recs) == 400
    index = B.parse_bai(bai)
    assert index["n_no_coor"] == 7 and index["refs"][1]["pseudo"][3] == 6
    assert len({b for r in index["refs"] for b in r["bins"]} & {0, 1, 9, 73, 585}) >= 4      # the borders reach the upper levels


def test_runs_give_the_same_files(checker):
    lines = hand_sam()
    one = run_check(checker, lines, "one")
    small = run_check(checker, lines, "r300", 300)
    mid = run_check(checker, lines, "r5000", 5000)
    assert one[3] == 1 and small[3] > 100 and 2 < mid[3] < small[3]
    assert small[:2] == one[:2] and mid[:2] == one[:2]


@pytest.mark.parametrize("n", [0, 1])
def test_no_record_and_one_record(checker, n):
    lines = ["only\t0\tchr2\t101\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n"][:n]
    for run_bytes in (None, 300):
        bam, bai, n_records, n_runs = run_check(checker, lines, f"few{n}", run_bytes)
        assert (n_records, n_runs) == (n, n)
        assert bam_to_sam(checker[0] / f"few{n}.bam")[0] == expected_text(lines)
        assert len(check_sorted_file(bam, bai, 5)) == n


# ---- the oracle-backed tools ----
def raw_records(path):
    import gzip
    return [r for _, r in records_of(gzip.decompress(open(path, "rb").read()))[0]]


def run_tool(exe, d, args, out, extra=(), env=None):
    r = subprocess.run([exe, *args, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    assert not glob.glob(str(d / "*.tmp")), "a run file was left behind"
    return r.stderr


def tool_jobs(tmp_path_factory):
    """[(name, tool, directory, arguments, options)]: RUNS of test_bgzf on the SAM fixture's inputs, and the paired fixture."""
    d = tmp_path_factory.mktemp("bamsort_tools")
    with open(os.path.join(ROOT, "tests", "golden", "sam_small.json")) as f:
        golden = json.load(f)
    write_inputs(golden, d)
    jobs = [(f"run{k}", which, d, golden_args(golden), list(extra)) for k, (which, extra) in enumerate(RUNS)]
    dp = tmp_path_factory.mktemp("bamsort_pairs")
    make_paired_fixture(dp)
    jobs.append(("pairs", "bucketmap_align", dp, [*PAIR_ARGS, "-q", "pairs.fastq"], ["--paired", "--rescue"]))
    return jobs


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    return tool_jobs(tmp_path_factory)


def pair_of(d, stem):
    return (d / f"{stem}.bam").read_bytes(), (d / f"{stem}.bam.bai").read_bytes()


@pytest.mark.parametrize("k", range(len(RUNS) + 1))
def test_oracle_tool_sorts_and_indexes(jobs, k):
    name, which, d, args, extra = jobs[k]
    exe = TOOLS[(which, "oracle")]
    run_tool(exe, d, args, f"{name}.u.bam", extra)
    err = run_tool(exe, d, args, f"{name}.s.bam", [*extra, "--sort"])
    assert re.search(r"Sorted \d+ records by coordinate in 1 run", err)
    assert not os.path.exists(d / f"{name}.u.bam.bai")
    unsorted = raw_records(d / f"{name}.u.bam")
    bam, bai = pair_of(d, f"{name}.s")
    got = check_sorted_file(bam, bai, 50, seed=k)
    assert len(got) > 10 and got == [unsorted[i] for i in sort_reference(unsorted)[0]]
    err = run_tool(exe, d, args, f"{name}.r.bam", [*extra, "--sort"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1
    assert pair_of(d, f"{name}.r") == (bam, bai)
    run_tool(exe, d, args, f"{name}.v.bam", [*extra, "--sort-mem", "1"], env=dict(BM_VERIFY_BLOCK_READS="3", BM_BATCH_READS="5"))
    assert pair_of(d, f"{name}.v") == (bam, bai)


def test_cli_refuses_what_it_cannot_sort(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        r = subprocess.run([exe, "-i", "idx", "--sort", "-o", "x.sam"], cwd=str(tmp_path), capture_output=True, text=True)
        assert r.returncode != 0 and "x.bam" in r.stderr and "--sort" in r.stderr and not os.listdir(tmp_path), r.stderr
        r = subprocess.run([exe, "-i", "idx", "-o", "x.sam", "--sort-mem", "5"], cwd=str(tmp_path), capture_output=True, text=True)
        assert r.returncode != 0 and "x.bam" in r.stderr
        for bad in ("0", "x"):
            r = subprocess.run([exe, "-i", "idx", "-o", "x.bam", "--sort-mem", bad], cwd=str(tmp_path), capture_output=True, text=True)
            assert r.returncode != 0 and "--sort-mem" in r.stderr and "[ERROR]" in r.stderr, r.stderr
        r = subprocess.run([exe, "-i", "idx", "-o", "x.bam", "--sort"], cwd=str(tmp_path), capture_output=True, text=True)
        assert "Validation failed" not in r.stderr and "Unknown option" not in r.stderr


# ---- the sanitized tools ----
@pytest.fixture(scope="module")
def asan_tools():
    exe = {w: os.path.join(ROOT, "tests", "cpp", f"{w}_oracle_asan") for w in ("bucketmap", "bucketmap_align")}
    r = subprocess.run(["make", "-C", ROOT, "-j2", *[os.path.relpath(p, ROOT) for p in exe.values()]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("k", [0, 1])
def test_sanitized_tool_sorts_clean(jobs, asan_tools, k):
    name, which, d, args, extra = jobs[k]
    run_tool(TOOLS[(which, "oracle")], d, args, f"{name}.p.bam", [*extra, "--sort"])
    want = pair_of(d, f"{name}.p")
    run_tool(asan_tools[which], d, args, f"{name}.a.bam", [*extra, "--sort"])
    assert pair_of(d, f"{name}.a") == want
    run_tool(asan_tools[which], d, args, f"{name}.b.bam", [*extra, "--sort"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert pair_of(d, f"{name}.b") == want


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import bamsort, bgzf
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bms.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bms_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(bamsort.SYMBOLS) and len(names) == 6
    L = bamsort.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    assert f"BMS_MIN_RECORD = {bamsort.MIN_RECORD}" in text
    z = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmz.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(bmz_[a-z0-9_]+)\s*\(", z))) == sorted(bgzf.SYMBOLS) and len(bgzf.SYMBOLS) == 7


def test_argument_errors_need_no_device():
    from bucket_map_amd import bamsort
    L = bamsort.lib()
    u8p, u32p, u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64))
    recs = [make_record(0, 5, b"a"), make_record(0, 3, b"bb", b"xyz")]
    good, good_off = b"".join(recs), offsets_of(recs)
    short = struct.pack("<I", 31) + bytes(31)                         # 35 bytes: no room for the fixed fields
    lying = bytearray(good)
    lying[0] += 1                                                      # block_size says one byte more than the extent
    cases = {
        "first offset": (good, [1, good_off[1], good_off[2]], 2, "rec_offset[0]"),
        "descending": (good, [0, good_off[2], good_off[1]], 2, "ascending"),
        "equal": (good, [0, good_off[1], good_off[1]], 2, "ascending"),
        "last offset": (good, [0, good_off[1]], 1, "the stream has"),
        "beyond": (good, [0, good_off[1], good_off[2] + 4], 2, "beyond"),
        "short record": (short, [0, 35], 1, "35 bytes"),
        "block_size": (bytes(lying), good_off, 2, "block_size"),
        "too many": (good, good_off, 2 ** 31, "2^31"),
    }

    def call(which, stream, off, n, block_bytes=65280, out_cap=None, null=()):
        a = np.frombuffer(stream, np.uint8)
        o = np.asarray(off, np.uint64)
        out = np.zeros(len(stream) + 1000, np.uint8)
        perm, so, got = np.zeros(8, np.uint32), np.full(9, 77, np.uint64), C.c_uint64(0)
        p = dict(a=a.ctypes.data_as(u8p), o=o.ctypes.data_as(u64p), out=out.ctypes.data_as(u8p), perm=perm.ctypes.data_as(u32p),
                 so=so.ctypes.data_as(u64p), got=C.byref(got))
        for k in null:
            p[k] = None
        if which == "sort":
            return L.bms_sort(None, p["a"], len(stream), p["o"], n, p["out"], p["perm"], p["so"])
        cap = out.size if out_cap is None else out_cap
        return L.bms_sort_deflate(None, p["a"], len(stream), p["o"], n, block_bytes, p["out"], cap, p["got"], p["perm"], p["so"])

    for which in ("sort", "deflate"):
        for name, (stream, off, n, word) in cases.items():
            assert call(which, stream, off, n) == bamsort.BMS_ERR_ARG, (which, name)
            assert word in L.bms_last_error().decode(), (which, name, L.bms_last_error())
        for null in ("a", "o", "out", "perm", "so"):
            assert call(which, good, good_off, 2, null=(null,)) == bamsort.BMS_ERR_ARG
            assert "null argument" in L.bms_last_error().decode(), (which, null)
        # a stream that passes every check reaches the context, which is looked at last
        assert call(which, good, good_off, 2) == bamsort.BMS_ERR_ARG and "null context" in L.bms_last_error().decode()
        assert call(which, b"", [0], 0) == bamsort.BMS_ERR_ARG and "null context" in L.bms_last_error().decode()
    for block in (0, 65281, 2 ** 32 - 1):
        assert call("deflate", good, good_off, 2, block_bytes=block) == bamsort.BMS_ERR_ARG and "block_bytes" in L.bms_last_error().decode()
    assert call("deflate", good, good_off, 2, out_cap=len(good) + 30) == bamsort.BMS_ERR_ARG and "may be needed" in L.bms_last_error().decode()
    assert call("deflate", good, good_off, 2, null=("got",)) == bamsort.BMS_ERR_ARG
    assert L.bms_create(0, None) == bamsort.BMS_ERR_ARG and L.bms_last_stats(None, None, None, None, None) == bamsort.BMS_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import bamsort
    with pytest.raises(bamsort.BmsError) as e:
        bamsort.Sorter(0)
    assert e.value.code == bamsort.BMS_ERR_HIP


def test_python_restatement_of_the_key():
    """refID = -1 sorts last, pos = -1 before pos = 0, ties keep their order."""
    recs = [make_record(-1, -1, b"u0"), make_record(1, 0, b"b"), make_record(0, 2 ** 31 - 2, b"c"), make_record(1, -1, b"d"),
            make_record(0, 0, b"e"), make_record(1, 0, b"f"), make_record(-1, -1, b"u1")]
    perm, stream, so = sort_reference(recs)
    assert perm == [4, 2, 3, 1, 5, 0, 6] and so[-1] == len(stream) == sum(len(r) for r in recs)
