"""The host plumbing and the C oracles under AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY.md section 5's race /
memory-error detection, CPU build: GPU sanitizers are not available on the pool).

`make tests/cpp/bucketmap[_align]_oracle_asan` compiles main.cpp, the locator, the SAM writer, the FASTA/FASTQ readers
and the three C oracles with -fsanitize=address,undefined; the tools then index and map the inputs of
tests/golden/sam_small.json -- short reads, a 5-window read, N / IUPAC / lower case, low qualities, both strands -- and must
(i) exit 0 with no sanitizer report and (ii) still write the fixture's records.
"""
import json
import os
import subprocess

import pytest

from test_sam_golden import ROOT, check, write_inputs

ASAN = {"bucketmap": os.path.join(ROOT, "tests", "cpp", "bucketmap_oracle_asan"),
        "bucketmap_align": os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle_asan")}


@pytest.fixture(scope="module")
def asan_tools():
    r = subprocess.run(["make", "-C", ROOT, "-j2", *[os.path.relpath(p, ROOT) for p in ASAN.values()]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return ASAN


@pytest.mark.parametrize("which", ["bucketmap", "bucketmap_align"])
@pytest.mark.parametrize("blocks", [None, {"BM_VERIFY_BLOCK_READS": "3", "BM_BATCH_READS": "5", "BM_IO_BLOCK": "64"}])
def test_sanitized_tool_is_clean_and_writes_the_fixture(asan_tools, tmp_path, which, blocks):
    with open(os.path.join(ROOT, "tests", "golden", "sam_small.json")) as f:
        golden = json.load(f)
    write_inputs(golden, tmp_path)
    fl = golden["flags"]
    args = ["-i", "idx", "--genome", "g.fa", "--bucket-len", str(fl["bucket_len"]), "-r", str(fl["read_len"]),
            "-k", str(fl["q"]), "-l", str(fl["k"]), "-s", str(fl["S"]), "-e", str(fl["e"]), "-d", str(fl["d"]),
            "-b", str(fl["b"]), "-n", str(fl["n"]), "-p", str(fl["p"]), "-u", str(fl["u"]), "-f", "1",
            "-q", "reads.fastq", "-o", "out.sam"]
    env = dict(os.environ, ASAN_OPTIONS="protect_shadow_gap=0:detect_leaks=1:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", **(blocks or {}))
    r = subprocess.run([asan_tools[which], *args], cwd=str(tmp_path), capture_output=True, text=True, env=env)
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, \
        r.stderr[-4000:]
    assert r.returncode == 0, r.stderr[-4000:]
    sq, recs = [], []
    for line in open(tmp_path / "out.sam"):
        f = line.rstrip("\n").split("\t")
        if f[0] == "@SQ":
            sq.append([f[1][3:], int(f[2][3:])])
        elif not line.startswith("@"):
            recs.append([f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[9], f[10]])
    check(golden, which, sq, recs, r.stderr)


# ------------------------------------------------------------------------------------------------ every option family

# What the oracle-backed tools run on the CPU under each option family -- host/best_mapq.h, pair_mapq.h, pair_rescue.h,
# frag_range.h, affine_realign.h, bgzf.h, bam.h, the annotation and the left-align code of the host layer --, which the GPU tools
# are held to byte for byte.  Per family: the tool, the inputs (the SAM fixture's; the paired fixture of tests/test_pair.py, its
# pairs in the duplicate and its pairs in unique sequence in one file; the pairs with a mate without a candidate of
# tests/test_rescue.py; the chimeric reads of tests/test_split_gpu.py), the options, the output's name, and what the run has to
# show for itself on stderr.
# Two families end in a refusal, and that is the path the sanitizers see: the oracle-backed verifier has no clipping pass
# (host/bucket_locator.h; tests/test_bgzf.py: GPU_ONLY_RUNS), so --clip and --split index, map and align the first block and
# then leave through the exception that says so -- the same exit status and the same message as the unsanitized tool, and
# nothing leaked on the way out.
FAMILIES = [
    ("--best", "bucketmap_align", "golden", ["--best"], "out.sam", None),
    ("--annotate", "bucketmap_align", "golden", ["--annotate"], "out.sam", None),
    ("--clip", "bucketmap_align", "golden", ["--clip"], "out.sam", "no clipping pass"),
    ("--max-edit-rate 0.1", "bucketmap_align", "golden", ["--max-edit-rate", "0.1"], "out.sam", None),
    ("--affine --left-align", "bucketmap_align", "golden", ["--affine", "--left-align"], "out.sam", None),
    ("--split", "bucketmap_align", "chimeric", ["--split"], "out.sam", "no clipping pass"),
    ("--paired --rescue", "bucketmap_align", "lost mates", ["--paired", "--rescue"], "out.sam", None),
    ("--frag-auto --frag-min-pairs 1", "bucketmap_align", "pairs", ["--frag-auto", "--frag-min-pairs", "1"], "out.sam", "learned from"),
    ("-o out.bam, bucketmap", "bucketmap", "golden", [], "out.bam", None),
    ("-o out.bam, bucketmap_align", "bucketmap_align", "golden", [], "out.bam", None),
]
REFUSED = ("--clip", "--split")
SMALL_BLOCKS = {"BM_VERIFY_BLOCK_READS": "3", "BM_BATCH_READS": "5", "BM_IO_BLOCK": "64"}


def _family_inputs(inputs, d):
    """the input files of a family in d; returns the tool's arguments but for the options and -o"""
    if inputs == "golden":
        from test_bgzf import golden_args
        with open(os.path.join(ROOT, "tests", "golden", "sam_small.json")) as f:
            golden = json.load(f)
        write_inputs(golden, d)
        return golden_args(golden)
    if inputs == "pairs":
        from test_pair import ARGS, make_paired_fixture
        make_paired_fixture(d)
        with open(d / "all.fastq", "w") as f:
            f.write(open(d / "pairs.fastq").read() + open(d / "unique.fastq").read())
        return [*ARGS, "-q", "all.fastq"]
    if inputs == "lost mates":
        from test_pair import ARGS
        from test_rescue import make_rescue_fixture
        make_rescue_fixture(d)
        return [*ARGS, "-q", "lost.fastq"]
    from test_split_gpu import TOOL_FLAGS, make_split_job
    make_split_job(d, n_chimeric=10, n_plain=6)
    return list(TOOL_FLAGS)


@pytest.mark.parametrize("blocks", [None, SMALL_BLOCKS], ids=["default blocks", "small blocks"])
@pytest.mark.parametrize("family", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_sanitized_tool_under_every_option_family(asan_tools, tmp_path, family, blocks):
    """Each option family through the sanitized tool, in one block and in blocks of a few reads: exit 0, no ASan, UBSan or
    LeakSanitizer report, and the file the unsanitized tool writes for the same inputs, byte for byte.  (--clip and --split:
    the unsanitized tool's refusal, see FAMILIES.)"""
    from test_sam_golden import TOOLS
    name, which, inputs, options, out, says = family
    runs = {}
    for build, exe in (("sanitized", asan_tools[which]), ("plain", TOOLS[(which, "oracle")])):
        d = tmp_path / build
        d.mkdir()
        args = _family_inputs(inputs, d)
        env = dict(os.environ, ASAN_OPTIONS="protect_shadow_gap=0:detect_leaks=1:abort_on_error=0:exitcode=23",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", **(blocks or {}))
        runs[build] = subprocess.run([exe, *args, *options, "-o", out], cwd=str(d), capture_output=True, text=True, env=env)
    r, plain = runs["sanitized"], runs["plain"]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr and "LeakSanitizer" not in r.stderr, \
        r.stderr[-4000:]
    if name in REFUSED:
        assert plain.returncode != 0 and r.returncode == plain.returncode and r.returncode != 23, (r.returncode, plain.returncode, r.stderr[-4000:])
        assert says in r.stderr and says in plain.stderr and name in r.stderr, r.stderr[-4000:]
        assert "number of buckets" in r.stderr, "the refusal came before the tool did any work"
        return
    assert r.returncode == 0, r.stderr[-4000:]
    assert plain.returncode == 0, plain.stderr[-4000:]
    if says is not None:
        assert says in r.stderr and says in plain.stderr, r.stderr[-4000:]
    got, want = (tmp_path / "sanitized" / out).read_bytes(), (tmp_path / "plain" / out).read_bytes()
    assert len(want) > 200 and got == want, f"{name}: the sanitized tool's {out} differs from the unsanitized tool's"
    if inputs == "lost mates":
        assert got.count(b"XR:i:1") >= 10, "hardly a mate was rescued: the rescue path did not run"
