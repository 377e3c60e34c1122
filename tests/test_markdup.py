"""Duplicate marking (-o x.bam --markdup) without a GPU: host/markdup.h and host/bam_sort.h in mark mode as a program of its
own under ASan + UBSan, the oracle-backed tools (whose marking is the host default of block_compressor), the command line and
the bmd_* ABI surface.

The yardstick is the rule of include/bmd.h in plain Python (tests/markdup_rule.py), applied to the records in the order they
were written; the sorted file is then the --sort file with 0x400 ORed where the rule says so, and nothing else changed.
"""
import ctypes as C
import glob
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import markdup_rule as M
from test_bamsort import HEADER, check_sorted_file, offsets_of, pair_of, raw_records, run_tool, sort_reference
from test_bgzf import golden_args
from test_pair import ARGS as PAIR_ARGS, make_paired_fixture
from test_sam_golden import ROOT, TOOLS, write_inputs

COUNTS = re.compile(r"Marked (\d+) of (\d+) records as duplicates \((\d+) pair units, (\d+) fragment units\)")


def parse_counts(err):
    """(duplicates, records, pair units, fragment units) from the tools' stderr line."""
    found = COUNTS.findall(err)
    assert len(found) == 1, err
    return tuple(int(x) for x in found[0])


# ---- the hand-written SAM ----
def hand_sam():
    """(lines, what the rule must say about some of them by name)"""
    lines, expect = [], {}

    def add(name, flag, ref, pos1, cigar, qual, dup=None, tags=""):
        qlen = len(qual)
        seq = ("ACGT" * qlen)[:qlen] or "*"
        lines.append(f"{name}\t{flag}\t{ref}\t{pos1}\t30\t{cigar}\t*\t0\t0\t{seq}\t{qual or '*'}{tags}\n")
        if dup is not None:
            expect[(name, flag & 0xC0)] = dup

    # forward reads whose unclipped 5' end is base 1000 while their POS differ; the best score is kept
    add("f_plain", 0, "chr2", 1000, "20M", "I" * 20, 1)
    add("f_5S", 0, "chr2", 1005, "5S20M", "I" * 25, 0)
    add("f_3H2S", 0, "chr2", 1005, "3H2S20M", "I" * 22, 1)
    add("f_other", 0, "chr2", 1001, "20M", "I" * 20, 0)
    # reverse reads whose unclipped 5' end is base 2049
    add("r_plain", 16, "chr2", 2000, "50M", "5" * 50, 1)
    add("r_4S", 16, "chr2", 2010, "36M4S", "J" * 40, 0)
    add("r_2S3H", 16, "chr2", 2005, "10M5D25M2I2S3H", "J" * 38 + "K", 1)
    add("r_forward_there", 0, "chr2", 2049, "5M", "IIIII", 0)         # the same base on the other strand: another key
    # pairs at equal keys: different scores, then tied scores (the first stays)
    for k, q in enumerate("HJI"):
        add("pair_a%d" % k, 0x63, "chr2", 5000, "30M", q * 30, int(q != "J"))
        add("pair_a%d" % k, 0x93, "chr2", 5300, "30M", q * 30, int(q != "J"))
    for k in range(3):
        add("pair_t%d" % k, 0x53, "chr3", 400, "10M", "I" * 10, int(k > 0))        # the first mate is the reverse one
        add("pair_t%d" % k, 0xA3, "chr3", 100, "2S10M", "I" * 12, int(k > 0))
    add("pair_other", 0x63, "chr2", 5271, "30M1S", "I" * 31, 0)         # other ends: another pair key
    add("pair_other", 0x93, "chr2", 5000, "30M", "I" * 30, 0)
    # fragments on a pair's ends, whatever their score
    add("frag_on_first_end", 0, "chr2", 5000, "40M", "K" * 40, 1)
    add("frag_on_second_end", 16, "chr2", 5310, "20M", "K" * 20, 1)
    add("frag_beside", 0, "chr2", 5001, "40M", "K" * 40, 0)
    # an unmapped mate placed beside its partner: the partner is a fragment, the mate is nothing
    add("half0", 0x49, "chr2", 7000, "20M", "I" * 20, 0)
    add("half0", 0x85, "chr2", 7000, "*", "I" * 20, 0)
    add("half1", 0x49, "chr2", 7000, "20M", "H" * 20, 1)
    add("half1", 0x85, "chr2", 7000, "*", "K" * 20, 0)
    # supplementary, secondary: never marked, never a key
    add("sup", 0x800, "chr2", 1000, "20M", "K" * 20, 0)
    add("sec", 0x100, "chr2", 1000, "20M", "K" * 20, 0)
    # a long CIGAR (the CG:B,I placeholder in BAM) on a used key: never marked
    ops = "".join(f"1{'=X'[i % 2]}" for i in range(70000))
    lines.append(f"long\t0\tchr1\t7\t60\t{ops}\t*\t0\t0\t{'ACGT' * 17500}\t*\n")
    expect[("long", 0)] = 0
    add("on_long", 0, "chr1", 7, "5M", "IIIII", 0)
    add("on_long_again", 0, "chr1", 7, "5M", "IIIIH", 1)
    # names that differ in their last byte only: no pair, two fragments
    add("lastbyte_a", 0x43, "chr3", 900, "10M", "I" * 10, 0)
    add("lastbyte_b", 0x83, "chr3", 950, "10M", "I" * 10, 0)
    add("lastbyte_c", 0x43, "chr3", 900, "10M", "H" * 10, 1)
    add("lastbyte_d", 0x83, "chr3", 950, "10M", "H" * 10, 1)
    for k in range(7):
        lines.append(f"nowhere{k}\t4\t*\t0\t0\t*\t*\t0\t0\tACGTN\tIIIII\n")
    # filler in pairs and singles, some on equal places
    for k in range(60):
        pos = 20000 + 37 * (k % 23)
        add("fill%d" % k, 0x63, "chr1", pos, "25M", "I" * 25)
        add("fill%d" % k, 0x93, "chr1", pos + 200, "25M", "I" * 25)
        add("single%d" % k, 16 * (k % 2), "chr2", 30000 + 11 * (k % 17), "15M", "IJ"[k % 2] * 15)
    return lines, expect


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("markdup_check")
    exe = str(d / "markdup_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "markdup_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_check(checker, lines, stem, run_bytes=None):
    d, exe = checker
    (d / f"{stem}.sam").write_text(HEADER + "".join(lines))
    r = subprocess.run([exe, f"{stem}.sam", f"{stem}.bam", *([str(run_bytes)] if run_bytes else [])], cwd=str(d), capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and r.returncode == 0, r.stderr[-3000:]
    assert not glob.glob(str(d / "*.tmp")), "a run file was left behind"
    numbers = [int(x) for x in r.stdout.split()]
    return (d / f"{stem}.bam").read_bytes(), (d / f"{stem}.bam.bai").read_bytes(), numbers


def unsorted_records(checker, lines):
    """(the records of the lines in the order written, the records of their unmarked --sort file): the encoding is the
    sorter's own -- tests/cpp/bam_sort_check.cpp's file, put back into input order by name and flag."""
    d, _ = checker
    sort_exe = str(d / "bam_sort_check")
    if not os.path.exists(sort_exe):
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", sort_exe, os.path.join(ROOT, "tests", "cpp", "bam_sort_check.cpp")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
    (d / "plain.sam").write_text(HEADER + "".join(lines))
    r = subprocess.run([sort_exe, "plain.sam", "plain.bam"], cwd=str(d), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    recs = raw_records(d / "plain.bam")
    by_id = {}
    for rec in recs:
        by_id.setdefault((rec[36: 36 + rec[12] - 1].decode(), struct.unpack_from("<H", rec, 18)[0]), []).append(rec)
    out = []
    for line in lines:
        f = line.split("\t")
        out.append(by_id[(f[0], int(f[1]))].pop(0))
    return out, recs


def test_hand_written_sam_marked_sorted_and_indexed(checker):
    lines, expect = hand_sam()
    records, plain_sorted = unsorted_records(checker, lines)
    marked, dup, counts = M.marked(records)
    for (name, mate), want in expect.items():
        at = [i for i, l in enumerate(lines) if l.split("\t")[0] == name and int(l.split("\t")[1]) & 0xC0 == mate]
        assert len(at) == 1 and dup[at[0]] == want, (name, mate)
    kind = M.ends(records)[2]
    assert kind[lines.index(next(l for l in lines if l.startswith("long\t")))] == 0
    assert kind[[l.split("\t")[0] for l in lines].index("lastbyte_a")] == 1
    bam, bai, numbers = run_check(checker, lines, "hand")
    assert numbers == [len(lines), 1, *counts] and counts[2] >= 8 and counts[3] >= 8
    got = check_sorted_file(bam, bai, None)
    assert got == [marked[i] for i in sort_reference(marked)[0]]
    assert [bytes(r[:19]) + bytes([r[19] & ~4]) + bytes(r[20:]) for r in got] == plain_sorted
    assert sum(1 for r in got if r[19] & 4) == counts[2] + counts[3]


def test_runs_give_the_same_files_and_do_not_part_mates(checker):
    lines, _ = hand_sam()
    one = run_check(checker, lines, "one")
    small = run_check(checker, lines, "r300", 300)
    mid = run_check(checker, lines, "r5000", 5000)
    assert one[2][1] == 1 and small[2][1] > 50 and 2 < mid[2][1] < small[2][1]
    assert small[:2] == one[:2] and mid[:2] == one[:2]
    assert small[2][2:] == one[2][2:] and mid[2][2:] == one[2][2:]      # the same units: no pair was cut in two


@pytest.mark.parametrize("n", [0, 1])
def test_no_record_and_one_record(checker, n):
    lines = ["only\t0\tchr2\t101\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII\n"][:n]
    for run_bytes in (None, 300):
        bam, bai, numbers = run_check(checker, lines, f"few{n}", run_bytes)
        assert numbers == [n, n, 0, n, 0, 0]
        assert len(check_sorted_file(bam, bai, 5)) == n


def test_host_rule_refuses_what_the_abi_refuses(tmp_path):
    """markdup_ends and markdup_mark throw where bmd_ends and bmd_mark return BMD_ERR_ARG (a stand-alone program)."""
    src = tmp_path / "refuse.cpp"
    src.write_text('#include "%s"\n#include <cstdio>\nint main() {\n'
                   '    std::vector<uint64_t> e, s; std::vector<uint8_t> k, d; uint64_t c[4];\n'
                   '    uint8_t rec[40] = {36, 0, 0, 0}; rec[12] = 9; const uint64_t off[2] = {0, 40};\n'
                   '    int caught = 0;\n'
                   '    try { bm::markdup_ends(rec, off, 1, e, s, k); } catch (const std::runtime_error &) { caught++; }\n'
                   '    const uint64_t z[2] = {0, 0}; const uint8_t bad[2] = {3, 2};\n'
                   '    try { bm::markdup_mark(z, z, bad, 2, d, c); } catch (const std::runtime_error &) { caught++; }\n'
                   '    rec[12] = 4; bm::markdup_ends(rec, off, 1, e, s, k);\n'
                   '    std::printf("%%d %%d\\n", caught, (int)k[0]);\n    return 0;\n}\n'
                   % os.path.join(ROOT, "bucket-map_amd", "host", "markdup.h"))
    exe = str(tmp_path / "refuse")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["2", "1"], r.stderr[-2000:]


# ---- the oracle-backed tools ----
def markdup_jobs(tmp_path_factory):
    """[(name, tool, directory, arguments, options)]: the paired fixture with copies of some pairs appended (new names, qualities
    H / I / J so that scores differ and some tie), and the single-end job of sam_small.json with some reads repeated."""
    dp = tmp_path_factory.mktemp("markdup_pairs")
    make_paired_fixture(dp)
    fq = (dp / "pairs.fastq").read_text().split("\n")
    reads = [fq[i: i + 4] for i in range(0, len(fq) - 1, 4)]                  # [name, seq, +, qual]
    extra = []
    for c, q in enumerate("HJIIJ"):
        for p in (0, 1, 4, 5, 8, 11):
            for mate in (0, 1):
                name, seq, plus, qual = reads[2 * p + mate]
                extra.append([f"@copy{c}_{name[1:]}", seq, plus, q * len(qual)])
    with open(dp / "dups.fastq", "w") as f:
        f.write("".join("\n".join(r) + "\n" for r in reads + extra))
    jobs = [("pairs", "bucketmap_align", dp, [*PAIR_ARGS, "-q", "dups.fastq"], ["--paired", "--rescue"])]
    d = tmp_path_factory.mktemp("markdup_single")
    with open(os.path.join(ROOT, "tests", "golden", "sam_small.json")) as f:
        golden = json.load(f)
    write_inputs(golden, d)
    with open(d / "dups.fastq", "w") as f:
        for name, seq, qual in golden["reads"]:
            f.write(f"@{name}\n{seq}\n+\n{qual}\n")
        for c, q in enumerate("HJI"):
            for name, seq, qual in golden["reads"][c::4]:
                f.write(f"@copy{c}_{name}\n{seq}\n+\n{q * len(qual)}\n")
    args = golden_args(golden)
    args[args.index("reads.fastq")] = "dups.fastq"
    jobs.append(("single", "bucketmap_align", d, args, ["--annotate"]))
    jobs.append(("plain", "bucketmap", d, args, []))
    return jobs


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    return markdup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", range(3))
def test_oracle_tool_marks_what_the_rule_marks(jobs, k):
    name, which, d, args, extra = jobs[k]
    exe = TOOLS[(which, "oracle")]
    run_tool(exe, d, args, f"{name}.u.bam", extra)
    err = run_tool(exe, d, args, f"{name}.s.bam", [*extra, "--sort"])
    assert "Marked" not in err
    err = run_tool(exe, d, args, f"{name}.m.bam", [*extra, "--markdup"])
    assert re.search(r"Sorted \d+ records by coordinate in 1 run", err)
    told = parse_counts(err)
    unsorted = raw_records(d / f"{name}.u.bam")
    assert not any(r[19] & 4 for r in unsorted)
    marked, dup, counts = M.marked(unsorted)
    assert told == (counts[2] + counts[3], len(unsorted), counts[0], counts[1])
    if name == "pairs":
        assert counts[0] >= 2 and counts[2] >= 2, counts
    else:
        assert counts[1] >= 2 and counts[3] >= 1, counts
    bam, bai = pair_of(d, f"{name}.m")
    got = check_sorted_file(bam, bai, 50, seed=k)
    perm = sort_reference(unsorted)[0]
    assert got == [marked[i] for i in perm]
    assert raw_records(d / f"{name}.s.bam") == [unsorted[i] for i in perm]     # and --sort alone is what it was
    err = run_tool(exe, d, args, f"{name}.r.bam", [*extra, "--markdup"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert int(re.search(r"in (\d+) run", err).group(1)) > 1 and parse_counts(err) == told
    assert pair_of(d, f"{name}.r") == (bam, bai)
    err = run_tool(exe, d, args, f"{name}.v.bam", [*extra, "--markdup", "--sort-mem", "1"], env=dict(BM_VERIFY_BLOCK_READS="3", BM_BATCH_READS="5"))
    assert parse_counts(err) == told
    assert pair_of(d, f"{name}.v") == (bam, bai)


# ---- the command line ----
def test_cli_refuses_sam_and_turns_sort_on(tmp_path):
    for which in ("bucketmap", "bucketmap_align"):
        exe = TOOLS[(which, "oracle")]
        r = subprocess.run([exe, "-i", "idx", "--markdup", "-o", "x.sam"], cwd=str(tmp_path), capture_output=True, text=True)
        assert r.returncode != 0 and "x.bam" in r.stderr and "--markdup" in r.stderr and not os.listdir(tmp_path), r.stderr
        assert "only BAM output is sorted and indexed" in r.stderr
        r = subprocess.run([exe, "-i", "idx", "-o", "x.bam", "--markdup"], cwd=str(tmp_path), capture_output=True, text=True)
        assert "Validation failed" not in r.stderr and "Unknown option" not in r.stderr


def test_markdup_alone_sorts(jobs):
    name, which, d, args, extra = jobs[2]
    err = run_tool(TOOLS[(which, "oracle")], d, args, "alone.bam", ["--markdup"])
    assert "Sorted" in err and os.path.exists(d / "alone.bam.bai")
    import gzip
    assert b"SO:coordinate" in gzip.decompress((d / "alone.bam").read_bytes())[:200]


# ---- the ABI ----
def test_abi_symbols():
    from bucket_map_amd import markdup
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmd.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(bmd_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(markdup.SYMBOLS) and len(names) == 8
    L = markdup.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    for n in ("bmd_ends", "bmd_mark", "bmd_mark_sort_deflate", "bmd_last_stats", "bmd_create", "bmd_destroy", "bmd_last_error"):
        assert n in names


def full_record(l_name=2, n_cigar=1, l_seq=4, room=0):
    body = struct.pack("<iiBBHHHIiii", 0, 5, l_name, 0, 4680, n_cigar, 0, l_seq, -1, -1, 0)
    body += bytes(l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq + room)
    return struct.pack("<I", len(body)) + body


def test_argument_errors_need_no_device():
    from bucket_map_amd import markdup
    L = markdup.lib()
    u8p, u32p, u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64))
    recs = [full_record(), full_record(3, 2, 7, 5)]
    good, good_off = b"".join(recs), offsets_of(recs)
    short = struct.pack("<I", 31) + bytes(31)
    lying = bytearray(good)
    lying[0] += 1
    unfit = {}
    for what, at, fmt, v in (("name", 12, "<B", 200), ("cigar", 16, "<H", 9), ("seq", 20, "<I", 40)):
        b = bytearray(good)
        struct.pack_into(fmt, b, good_off[1] + at, v)
        unfit[what] = bytes(b)
    b = bytearray(recs[0])
    struct.pack_into("<I", b, 20, 5)                                    # one quality byte too many, in the last record
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
        "one byte": (recs[1] + bytes(b), offsets_of([recs[1], bytes(b)]), 2, "record 1"),
    }

    def call(which, stream, off, n, block_bytes=65280, out_cap=None, null=()):
        a = np.frombuffer(stream, np.uint8)
        o = np.asarray(off, np.uint64)
        out = np.zeros(len(stream) + 1000, np.uint8)
        perm, so, got = np.zeros(8, np.uint32), np.full(9, 77, np.uint64), C.c_uint64(0)
        end, score, kind, dup, counts = np.zeros(8, np.uint64), np.zeros(8, np.uint64), np.zeros(8, np.uint8), np.zeros(8, np.uint8), np.zeros(4, np.uint64)
        p = dict(a=a.ctypes.data_as(u8p), o=o.ctypes.data_as(u64p), out=out.ctypes.data_as(u8p), perm=perm.ctypes.data_as(u32p),
                 so=so.ctypes.data_as(u64p), got=C.byref(got), end=end.ctypes.data_as(u64p), score=score.ctypes.data_as(u64p),
                 kind=kind.ctypes.data_as(u8p), dup=dup.ctypes.data_as(u8p), counts=counts.ctypes.data_as(u64p))
        for k in null:
            p[k] = None
        if which == "ends":
            return L.bmd_ends(None, p["a"], len(stream), p["o"], n, p["end"], p["score"], p["kind"])
        cap = out.size if out_cap is None else out_cap
        return L.bmd_mark_sort_deflate(None, p["a"], len(stream), p["o"], n, block_bytes, p["out"], cap, p["got"], p["perm"], p["so"],
                                       p["dup"], p["counts"])

    for which, nulls in (("ends", ("a", "o", "end", "score", "kind")), ("fused", ("a", "o", "out", "perm", "so", "got", "dup", "counts"))):
        for name, (stream, off, n, word) in cases.items():
            assert call(which, stream, off, n) == markdup.BMD_ERR_ARG, (which, name)
            assert word in L.bmd_last_error().decode(), (which, name, L.bmd_last_error())
        for null in nulls:
            assert call(which, good, good_off, 2, null=(null,)) == markdup.BMD_ERR_ARG
            assert "null argument" in L.bmd_last_error().decode(), (which, null)
        assert call(which, good, good_off, 2) == markdup.BMD_ERR_ARG and "null context" in L.bmd_last_error().decode()
        assert call(which, b"", [0], 0) == markdup.BMD_ERR_ARG and "null context" in L.bmd_last_error().decode()
    for block in (0, 65281, 2 ** 32 - 1):
        assert call("fused", good, good_off, 2, block_bytes=block) == markdup.BMD_ERR_ARG and "block_bytes" in L.bmd_last_error().decode()
    assert call("fused", good, good_off, 2, out_cap=len(good) + 30) == markdup.BMD_ERR_ARG and "may be needed" in L.bmd_last_error().decode()

    def mark(kind, n=None, null=()):
        k = np.asarray(kind, np.uint8)
        end, score, dup, counts = np.zeros(k.size + 1, np.uint64), np.zeros(k.size + 1, np.uint64), np.zeros(k.size + 1, np.uint8), np.zeros(4, np.uint64)
        p = dict(end=end.ctypes.data_as(u64p), score=score.ctypes.data_as(u64p), kind=k.ctypes.data_as(u8p), dup=dup.ctypes.data_as(u8p),
                 counts=counts.ctypes.data_as(u64p))
        for x in null:
            p[x] = None
        return L.bmd_mark(None, p["end"], p["score"], p["kind"], k.size if n is None else n, p["dup"], p["counts"])

    for kind, word in (([0, 4], "0 .. 3"), ([1, 2], "not followed"), ([2, 1, 3], "not followed"), ([3, 1], "not preceded"),
                       ([2, 3, 3], "not preceded"), ([1, 3], "not preceded"), ([2, 2, 3], "not followed")):
        assert mark(kind) == markdup.BMD_ERR_ARG and word in L.bmd_last_error().decode(), (kind, L.bmd_last_error())
    assert mark([1], n=2 ** 31) == markdup.BMD_ERR_ARG and "2^31" in L.bmd_last_error().decode()
    for null in ("end", "score", "kind", "dup", "counts"):
        assert mark([1, 2, 3], null=(null,)) == markdup.BMD_ERR_ARG and "null argument" in L.bmd_last_error().decode()
    assert mark([0, 1, 2, 3, 1]) == markdup.BMD_ERR_ARG and "null context" in L.bmd_last_error().decode()
    assert mark([]) == markdup.BMD_ERR_ARG and "null context" in L.bmd_last_error().decode()
    assert L.bmd_create(0, None) == markdup.BMD_ERR_ARG and L.bmd_last_stats(None, None, None, None) == markdup.BMD_ERR_ARG
    assert L.bmd_last_sort_stats(None, None, None, None, None) == markdup.BMD_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import markdup
    with pytest.raises(markdup.BmdError) as e:
        markdup.Marker(0)
    assert e.value.code == markdup.BMD_ERR_HIP


def test_python_restatement_of_the_rule():
    """The corners of the rule on descriptors: ties to the lowest i, a pair end beats any fragment, equal ends, kind 0 ignored."""
    E = lambda ref, end5, rev=0: ref << 33 | (end5 + 2 ** 31) << 1 | rev
    a, b = E(0, 10), E(0, 90, 1)
    end = [a, b, a, b, b, a, a, a, b, 0, E(0, 10, 1)]
    score = [5, 5, 6, 4, 5, 5, 99, 98, 1, 1000, 0]
    kind = [2, 3, 2, 3, 2, 3, 1, 1, 1, 0, 1]
    dup, counts = M.mark(end, score, kind)
    assert dup == [0, 0, 1, 1, 1, 1, 1, 1, 1, 0, 0] and counts == [3, 4, 4, 3]
    assert M.mark([a, a, a], [1, 2, 2], [1, 1, 1])[0] == [1, 0, 1]
    assert M.mark([a, a, a, a], [0, 0, 0, 0], [2, 3, 2, 3])[0] == [0, 0, 1, 1]
    assert M.passes([a, a, a], [1, 2, 2], [1, 1, 1]) == 1 and M.passes([], [], []) == 0
