"""Compressed input on the device: bmu_inflate (include/bmu.h) against the text, gzip.decompress and the block-type counts
of tests/inflate_rule.py; independence from the batch; corrupt streams refused cleanly; `bucketmap` and `bucketmap_align`
on BGZF -q / --genome, whose output must be the plain-input run's byte for byte."""
import gzip
import json
import os
import random
import subprocess

import pytest

import inflate_rule as Z
from test_bgzf import golden_args
from test_bgzf_gpu import bam_like
from test_inflate import compressed_args
from test_pair import ARGS as PAIR_ARGS, make_paired_fixture
from test_sam_golden import ROOT, TOOLS, write_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def u():
    from bucket_map_amd import inflate
    c = inflate.Inflater(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def type_counts():
    """name -> [n_stored, n_fixed, n_dynamic] by the pure-Python decoder, computed once."""
    out = {}
    for name, (blob, _) in Z.CASES.items():
        raw = Z.payload(blob) if name != "fname_extra" else Z.raw_deflate(Z.CASES[name][1])
        types = Z.inflate(raw)[1]["types"]
        out[name] = [types.count(k) for k in range(3)]
    return out


@pytest.mark.parametrize("name", sorted(Z.CASES))
def test_device_inflates_every_case(u, type_counts, name):
    blob, data = Z.CASES[name]
    got = u.inflate(blob)
    assert got == data
    assert got == gzip.decompress(blob)
    assert [u.n_stored, u.n_fixed, u.n_dynamic] == type_counts[name]


def test_all_cases_in_one_file_and_cut_in_two(u, type_counts):
    parts, want, counts = [], [], [0, 0, 0]
    for k, name in enumerate(sorted(Z.CASES)):
        parts.append(Z.CASES[name][0])
        want.append(Z.CASES[name][1])
        counts = [a + b for a, b in zip(counts, type_counts[name])]
        if k % 3 == 0:
            parts.append(Z.EOF)                          # an empty block: one fixed DEFLATE block
            want.append(b"")
            counts[1] += 1
    parts.append(Z.EOF)
    counts[1] += 1
    blob, text = b"".join(parts), b"".join(want)
    assert u.inflate(blob) == text
    assert [u.n_stored, u.n_fixed, u.n_dynamic] == counts
    # a block's output does not depend on its neighbours: the same bytes from two calls cut at a block border
    cut = sum(map(len, parts[: len(parts) // 2]))
    assert u.inflate(blob[:cut]) + u.inflate(blob[cut:]) == text


def test_more_blocks_than_the_device_holds_at_once(u):
    rng = random.Random(31)
    sizes = [rng.randrange(300, 2001) for _ in range(2500)] + [65280] + [rng.randrange(300, 2001) for _ in range(200)]
    data = Z.fastq(sum(sizes), seed=12)
    blob, in_off, out_off = Z.bgzf(data, sizes, level=1)
    assert len(in_off) == 2703 and out_off[-1] == len(data)
    assert u.inflate(blob) == data


def test_round_trip_with_the_compressor(u):
    from bucket_map_amd import bgzf
    z = bgzf.Compressor(0)
    try:
        x = bam_like(300_000, 7)
        for block_bytes in (300, 65280):
            blob, offsets, _ = z.deflate(x, block_bytes)
            assert u.inflate(blob + bgzf.EOF) == x
    finally:
        z.close()


def test_small_after_large_and_large_after_small(u):
    from bucket_map_amd import inflate
    small, large = Z.CASES["zfixed"], (Z.bgzf(Z.fastq(400_000, seed=3), 65280)[0], Z.fastq(400_000, seed=3))
    fresh = inflate.Inflater(0)
    try:
        for blob, data in (small, large, small, large):
            assert fresh.inflate(blob) == data
            assert u.inflate(blob) == data
    finally:
        fresh.close()


CORRUPT = ("cut_short", "block_type_3", "stored_nlen", "oversubscribed", "oversubscribed_ll", "distance_at_0", "isize_less", "isize_more", "crc_bit",
           "third_block")


@pytest.mark.parametrize("name", CORRUPT)
def test_corrupt_streams_are_refused_and_the_context_stays_usable(u, name):
    """The same inputs pass tests/test_inflate.py's stand-alone program under the sanitizers first; here the point is the
    clean refusal."""
    from bucket_map_amd import inflate
    blob, block, reason = Z.CORRUPT[name]
    with pytest.raises(inflate.BmuError) as e:
        u.inflate(blob)
    assert e.value.code == inflate.BMU_ERR_DATA
    assert u.bad_block() == (block, reason)
    good, data = Z.CASES["z6_fastq"]
    assert u.inflate(good) == data and u.bad_block() is None


def test_argument_and_format_refusals(u):
    from bucket_map_amd import inflate
    blob, data = Z.CASES["zfixed"]
    with pytest.raises(inflate.BmuError) as e:
        u.inflate(blob, out_cap=len(data) - 1)
    assert e.value.code == inflate.BMU_ERR_ARG
    with pytest.raises(inflate.BmuError) as e:
        u.inflate(gzip.compress(data))
    assert e.value.code == inflate.BMU_ERR_FORMAT and "bgzip" in str(e.value)
    assert u.inflate(blob) == data


# ---- the tools ----
def run(exe, d, args, out, extra=(), limit=120):
    r = subprocess.run([exe, *args, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0, r.stderr
    return d / out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_gpu")
    with open(os.path.join(ROOT, "tests", "golden", "sam_small.json")) as f:
        golden = json.load(f)
    write_inputs(golden, d)
    for block in (997, 65280):
        os.mkdir(d / f"b{block}")
        for name in ("reads.fastq", "g.fa"):
            (d / f"b{block}" / (name + ".gz")).write_bytes(Z.bgzf((d / name).read_bytes(), block)[0])
    return d, golden_args(golden)


@pytest.mark.parametrize("which", ["bucketmap", "bucketmap_align"])
def test_gpu_tools_read_compressed_inputs(inputs, which):
    d, args = inputs
    exe = TOOLS[(which, "gpu")]
    want = run(exe, d, args, f"{which}_plain.sam").read_bytes()
    assert want.count(b"\n") > 40
    for block in (997, 65280):
        z_args = compressed_args(args, f"b{block}/reads.fastq.gz", f"b{block}/g.fa.gz")
        for k, gpus in enumerate(("0", "0,0")):
            assert run(exe, d, z_args, f"{which}_{block}_{k}.sam", ["--gpus", gpus]).read_bytes() == want, (block, gpus)


def test_gpu_tool_refuses_plain_gzip(inputs):
    d, args = inputs
    (d / "plain.fastq.gz").write_bytes(gzip.compress((d / "reads.fastq").read_bytes()))
    r = subprocess.run([TOOLS[("bucketmap", "gpu")], *compressed_args(args, "plain.fastq.gz", "g.fa"), "-o", "refused.sam"], cwd=str(d),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "bgzip" in r.stderr and not (d / "refused.sam").exists(), r.stderr


def test_gpu_paired_markdup_bam_from_compressed_pairs(tmp_path):
    make_paired_fixture(tmp_path)
    (tmp_path / "z.fastq.gz").write_bytes(Z.bgzf((tmp_path / "pairs.fastq").read_bytes(), 997)[0])
    exe, extra = TOOLS[("bucketmap_align", "gpu")], ["--paired", "--markdup"]
    want = run(exe, tmp_path, [*PAIR_ARGS, "-q", "pairs.fastq"], "plain.bam", extra).read_bytes()
    assert run(exe, tmp_path, [*PAIR_ARGS, "-q", "z.fastq.gz"], "z.bam", extra).read_bytes() == want
