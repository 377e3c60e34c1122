"""Edit-bounded verification without a GPU: the ABI of bmv_align_bounded, the tools' --max-edit-rate option, and the
default alignment_verifier::align_bounded (align, then mark) through the oracle-backed tool."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOLS = {
    "bucketmap": os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle"),
    "bucketmap_align": os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle"),
}


def test_header_and_binding_agree_on_the_new_symbols():
    from bucket_map_amd import verify
    text = open(os.path.join(ROOT, "include", "bmv.h")).read()
    assert re.search(r"#define\s+BMV_REJECTED\s+INT32_MIN", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = verify.lib()
    for name in ("bmv_align_bounded", "bmv_last_bounded_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
    # max_edits sits between query_len and n, as the header has it
    decl = re.search(r"bmv_align_bounded\s*\((.*?)\)", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")][-4:] == ["query_len", "max_edits", "n", "total_cigar"]
    assert len(verify.SYMBOLS["bmv_align_bounded"][1]) == len(verify.SYMBOLS["bmv_align_long"][1]) + 1
    assert verify.REJECTED == -2 ** 31
    assert callable(verify.Verifier.align_bounded) and callable(verify.Verifier.bounded_stats)


def test_entry_points_fail_cleanly_without_a_context():
    from bucket_map_amd import verify
    L = verify.lib()
    total = C.c_uint64()
    assert L.bmv_align_bounded(None, None, 0, None, None, None, None, None, None, 0, C.byref(total)) == 1     # BMV_ERR_ARG
    assert b"bmv_align_bounded" in L.bmv_last_error()
    assert L.bmv_last_bounded_stats(None, None, None, None) == 1
    assert b"bmv_last_bounded_stats" in L.bmv_last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_cpu_fallback_for_the_bounded_call():
    from bucket_map_amd import verify
    with pytest.raises(verify.BmvError) as e:
        verify.Verifier().align_bounded([], [], [], [], [], [], [])
    assert e.value.code == 2                                         # BMV_ERR_HIP: no device, no context, no result


@pytest.mark.parametrize("tool", ["bucketmap", "bucketmap_align"])
def test_option_is_parsed_by_both_tools(tool, tmp_path):
    def run(*extra):
        return subprocess.run([TOOLS[tool], "-i", "idx", *extra], cwd=str(tmp_path), capture_output=True, text=True)
    for bad in (["--max-edit-rate", "-1"], ["--max-edit-rate", "x"], ["--max-edit-rate=-0.5"], ["--max-edit-rate=nan"]):
        r = run(*bad)
        assert r.returncode != 0 and "Value parse failed for --max-edit-rate" in r.stderr, (bad, r.stderr)
    r = run("--max-edit-rate")
    assert r.returncode != 0 and "Missing value for option --max-edit-rate" in r.stderr
    for good in (["--max-edit-rate=0.1"], ["--max-edit-rate", "0.1"], ["--max-edit-rate", "0"]):
        r = run(*good)                                               # parsed; what fails next is something else
        assert "--max-edit-rate" not in r.stderr and "Unknown option" not in r.stderr, (good, r.stderr)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "sam_small.json")) as f:
        return json.load(f)


def _run(golden, tool, d, out, extra=(), env=None):
    fl = golden["flags"]
    args = ["-i", "idx", "--genome", "g.fa", "--bucket-len", str(fl["bucket_len"]), "-r", str(fl["read_len"]),
            "-k", str(fl["q"]), "-l", str(fl["k"]), "-s", str(fl["S"]), "-e", str(fl["e"]), "-d", str(fl["d"]),
            "-b", str(fl["b"]), "-n", str(fl["n"]), "-p", str(fl["p"]), "-u", str(fl["u"]), "-f", "1",
            "-q", "reads.fastq", "-o", out, *extra]
    r = subprocess.run([TOOLS[tool], *args], cwd=str(d), capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return open(d / out).read().split("\n")


def _inputs(golden, d):
    with open(d / "g.fa", "w") as f:
        for name, seq in golden["records"]:
            f.write(f">{name}\n{seq}\n")
    with open(d / "reads.fastq", "w") as f:
        for name, seq, qual in golden["reads"]:
            f.write(f"@{name}\n{seq}\n+\n{qual}\n")


def bounded_sam_is_unbounded_minus_rejections(lines_all, dump_all, lines_bounded, dump_bounded, rate, u):
    """The check both backends share: the dump lists every alignment in record order (read, text start, text length,
    strand, query length, score, begin, CIGAR); a record exists for those that pass the MAPQ rule."""
    rows = [l.split() for l in dump_all if l]
    rows_b = [l.split() for l in dump_bounded if l]
    assert len(rows) == len(rows_b) > 0
    head = [l for l in lines_all if l.startswith("@")]
    recs = [l for l in lines_all if l and not l.startswith("@")]
    written = [r for r in rows if not ((60 + int(r[5])) % 2 ** 32 < u)]
    assert len(written) == len(recs)
    keep, n_over = [], 0
    for r, rb in zip(rows, rows_b):
        over = -int(r[5]) > int(rate * int(r[4]))        # the tool's bound: (uint32_t)(R * read length), R and the product in float32
        n_over += over
        assert rb[:5] == r[:5]
        assert rb[5:] == ([str(-2 ** 31), "0", "*"] if over else r[5:])
    for r, line in zip(written, recs):
        if not -int(r[5]) > int(rate * int(r[4])):
            keep.append(line)
    assert [l for l in lines_bounded if l.startswith("@")] == head
    assert [l for l in lines_bounded if l and not l.startswith("@")] == keep
    return n_over, len(recs) - len(keep)


def test_default_align_bounded_of_the_oracle_backed_tool(golden, tmp_path):
    _inputs(golden, tmp_path)
    u, rate = golden["flags"]["u"], 0.125                            # (exact in float32)
    plain = _run(golden, "bucketmap_align", tmp_path, "a.sam", env={"BM_DUMP_ALIGNMENTS": str(tmp_path / "a.txt")})
    assert [l.split("\t")[0] for l in plain if l and not l.startswith("@")] == [r[0] for r in golden["bucketmap_align"]["sam"]]
    bounded = _run(golden, "bucketmap_align", tmp_path, "b.sam", extra=["--max-edit-rate", str(rate)],
                   env={"BM_DUMP_ALIGNMENTS": str(tmp_path / "b.txt"), "BM_VERIFY_BLOCK_READS": "3"})
    n_over, n_gone = bounded_sam_is_unbounded_minus_rejections(plain, open(tmp_path / "a.txt").read().split("\n"), bounded,
                                                               open(tmp_path / "b.txt").read().split("\n"), rate, u)
    assert n_over > 0 and n_gone > 0, "the fixture has no alignment beyond the bound: the test shows nothing"
    loose = _run(golden, "bucketmap_align", tmp_path, "c.sam", extra=["--max-edit-rate=1"])
    assert loose == plain
    # plain bucketmap accepts the option and ignores it
    assert _run(golden, "bucketmap", tmp_path, "d.sam", extra=["--max-edit-rate=0.01"]) == _run(golden, "bucketmap", tmp_path, "e.sam")
