"""Compressed input without a GPU: the cases of tests/inflate_rule.py, the shared decoder lines (host/inflate_rule.h,
host/bgzf_in.h) as a program of their own under ASan + UBSan, the layout walk through the binding, the bmu_* ABI surface,
and the oracle-backed tools on BGZF -q / --genome, whose .sam must be the plain-input run's byte for byte."""
import ctypes as C
import gzip
import json
import os
import random
import re
import subprocess

import pytest

import inflate_rule as Z
from test_bgzf import golden_args
from test_sam_golden import ROOT, TOOLS, write_inputs


def test_cases_do_what_they_were_built_for():
    """Every case inflates to its text (here and with gzip), and has the property it exists for."""
    stats = {}
    for name, (blob, data) in Z.CASES.items():
        assert gzip.decompress(blob) == data, name
    for name in ("rule_deep_code_form2", "rule_dist32768_form1", "rule_match258_form2", "rule_random_form0", "rule_match4_form2",
                 "rule_len0_form0", "rule_len0_form1", "rule_len0_form2", "z6_zeros", "z6_acg", "z6_period2", "z6_period63",
                 "z6_period64", "z6_period65", "zfixed", "z6_fastq", "z1_fastq", "flushes", "z6_random", "deep_literals"):
        blob, data = Z.CASES[name]
        got, stats[name] = Z.inflate(Z.payload(blob))
        assert got == data, name
    s = stats
    # all three forms of every test_bgzf case, but for Huffman forms of 65 280 near-incompressible bytes that exceed a block's
    # 64 KiB (BSIZE has 16 bits): those are no BGZF blocks
    rule = {n for n in Z.CASES if n.startswith("rule_")}
    assert len({n.rsplit("_form", 1)[0] for n in rule}) * 3 == len(rule) + len(Z.OVERSIZE)
    assert Z.OVERSIZE and all(form > 0 and name in ("random", "deep_code") for name, form in Z.OVERSIZE), Z.OVERSIZE
    assert s["rule_deep_code_form2"]["max_code_len"] == 15 and s["rule_deep_code_form2"]["types"] == [2]
    assert s["rule_dist32768_form1"]["max_dist"] == 32768 and s["rule_dist32768_form1"]["types"] == [1]
    assert s["rule_match258_form2"]["max_match"] == 258
    assert s["rule_random_form0"]["types"] == [0] and len(Z.CASES["rule_random_form0"][0]) == 65311
    # the one-symbol distance code: a single distance symbol, one code of length 1
    assert s["rule_match4_form2"]["one_dist_code"] == 1 and s["rule_match4_form2"]["max_match"] == 4
    assert [s[f"rule_len0_form{f}"]["types"] for f in range(3)] == [[0], [1], [2]] and s["rule_len0_form0"]["empty_stored"] == 1
    assert s["z6_zeros"]["min_dist"] == 1 and s["z6_zeros"]["max_match"] == 258 and 18 in s["z6_zeros"]["run_syms"]
    assert s["z6_zeros"]["overlapping"] > 0
    assert s["z6_acg"]["min_dist"] == 3 and s["z6_acg"]["overlapping"] > 0
    for period in (2, 63, 64, 65):
        st = s[f"z6_period{period}"]
        assert st["min_dist"] == period and st["max_match"] == 258 and st["overlapping"] > 0, period
    assert s["zfixed"]["types"] == [1] and s["zfixed"]["max_match"] > 3
    for name in ("z6_fastq", "z1_fastq"):
        assert s[name]["run_syms"] == {16, 17, 18} and s[name]["max_code_len"] >= 13 and s[name]["max_dist"] > 30000, (name, s[name])
    assert s["z6_fastq"]["types"] == [2, 2]
    t = s["flushes"]["types"]
    assert s["flushes"]["empty_stored"] >= 2 and any(a == 0 and b in (1, 2) for a, b in zip(t, t[1:])), t
    assert s["z6_random"]["types"] == [0, 0]
    assert s["deep_literals"]["types"] == [2] and s["deep_literals"]["max_code_len"] == 15 and s["deep_literals"]["max_match"] == 0
    assert Z.CASES["fname_extra"][0][3] == 0x0C and Z.CASES["fname_extra"][0].index(b"BC") > 12


# ---- the decoder's lines as a program of their own, under ASan + UBSan ----
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_check")
    exe = str(d / "inflate_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "inflate_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return d, exe


def run_check(checker, blob, out=None):
    d, exe = checker
    (d / "in.gz").write_bytes(blob)
    r = subprocess.run([exe, "in.gz", *([out] if out else [])], cwd=str(d), capture_output=True, text=True)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and r.returncode == 0, r.stderr[-3000:]
    return r.stdout.split()


def test_host_decoder_on_every_case(checker):
    for name, (blob, data) in Z.CASES.items():
        got = run_check(checker, blob, "out.bin")
        assert got[:2] == ["ok", str(len(data))], (name, got)
        assert (checker[0] / "out.bin").read_bytes() == data, name
    got = run_check(checker, Z.CASES["z6_fastq"][0] + Z.EOF + Z.CASES["z6_random"][0], "out.bin")
    assert got == ["ok", str(63000 + 65280), "2", "1", "2"]             # DEFLATE blocks: two stored, the EOF block's fixed one, two dynamic


def test_host_decoder_refuses_corrupt_streams_cleanly(checker):
    for name, (blob, block, reason) in Z.CORRUPT.items():
        assert run_check(checker, blob) == ["data", str(block), str(reason)], name
    for name, blob in Z.format_errors().items():
        assert run_check(checker, blob)[0] == "format", name


def test_host_decoder_survives_bit_flips_and_truncations(checker):
    """A few hundred damaged copies of three small cases: any status, a clean exit, nothing out of range."""
    rng = random.Random(4242)
    seen = set()
    for name in ("zfixed", "deep_literals", "fname_extra"):
        blob = Z.CASES[name][0]
        for k in range(120):
            b = bytearray(blob)
            if k % 3 == 2:
                cut = rng.randrange(18, len(b) - 8)                     # payload cut short, BSIZE adjusted
                b = bytearray(Z.wrap(bytes(b[18:cut]), Z.CASES[name][1])) if name != "fname_extra" else b[:rng.randrange(1, len(b))]
            else:
                at = rng.randrange(len(b) * 8)
                b[at // 8] ^= 1 << (at % 8)
            seen.add(run_check(checker, bytes(b))[0])
    assert seen == {"ok", "format", "data"} or seen == {"format", "data"}


# ---- the layout through the binding ----
def test_layout_equals_the_writers_offsets():
    from bucket_map_amd import inflate
    data = Z.fastq(20000, seed=9)
    for sizes in (997, 65280, [1, 0 + 3, 5000, 1]):
        blob, in_off, out_off = Z.bgzf(data, sizes)
        assert inflate.layout(blob) == (in_off, out_off), sizes
    # empty blocks anywhere, and a header with FNAME and another subfield ahead of BC
    blob = Z.EOF + Z.CASES["fname_extra"][0] + Z.EOF + Z.EOF + Z.CASES["zfixed"][0]
    a, b = len(Z.CASES["fname_extra"][0]), len(Z.CASES["zfixed"][0])
    n = len(Z.CASES["zfixed"][1])
    assert inflate.layout(blob) == ([0, 28, 28 + a, 56 + a, 84 + a, 84 + a + b], [0, 0, n, n, n, 2 * n])
    assert inflate.layout(b"") == ([0], [0])


def test_layout_refuses_what_is_not_bgzf():
    from bucket_map_amd import inflate
    for name, blob in Z.format_errors().items():
        with pytest.raises(inflate.BmuError) as e:
            inflate.layout(blob)
        assert e.value.code == inflate.BMU_ERR_FORMAT, name
        if name == "plain_gzip":
            assert "bgzip" in str(e.value) and "byte 0" in str(e.value)
    # the offset of a plain member behind good blocks
    good = Z.CASES["zfixed"][0]
    with pytest.raises(inflate.BmuError) as e:
        inflate.layout(good + gzip.compress(b"x"))
    assert f"byte {len(good)}" in str(e.value) and "bgzip" in str(e.value)


# ---- the ABI ----
def test_abi_symbols_and_argument_errors():
    from bucket_map_amd import inflate
    text = open(os.path.join(ROOT, "include", "bmu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(bmu_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(inflate.SYMBOLS) and len(names) == 7
    L = inflate.lib()
    for n in names:
        assert hasattr(L, n), f"libbmf.so does not export {n}"
    for k, name in enumerate(("NONE", "TRUNCATED", "BLOCK_TYPE", "STORED_LEN", "CODE", "DISTANCE", "TOO_LONG", "TOO_SHORT", "CRC")):
        assert re.search(rf"BMU_REASON_{name} = {k}\b", text) and getattr(inflate, f"REASON_{name}") == k
    # argument errors need no device
    got = C.c_uint64(7)
    assert L.bmu_inflate(None, None, 0, None, 0, C.byref(got)) == inflate.BMU_ERR_ARG
    assert L.bmu_layout(None, 5, None, None, C.byref(got), C.byref(got)) == inflate.BMU_ERR_ARG
    assert L.bmu_create(0, None) == inflate.BMU_ERR_ARG and L.bmu_bad_block(None, None, None) == inflate.BMU_ERR_ARG
    assert L.bmu_last_stats(None, None, None, None, None) == inflate.BMU_ERR_ARG


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_is_an_error_not_a_cpu_path():
    from bucket_map_amd import inflate
    with pytest.raises(inflate.BmuError) as e:
        inflate.Inflater(0)
    assert e.value.code == inflate.BMU_ERR_HIP


# ---- the oracle-backed tools on compressed inputs ----
def compressed_args(args, reads, genome):
    out = list(args)
    out[out.index("-q") + 1] = reads
    out[out.index("--genome") + 1] = genome
    return out


@pytest.fixture(scope="module")
def tool_inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("inflate_tools")
    with open(os.path.join(ROOT, "tests", "golden", "sam_small.json")) as f:
        golden = json.load(f)
    write_inputs(golden, d)
    for block in (997, 65280):
        os.mkdir(d / f"b{block}")
        for name in ("reads.fastq", "g.fa"):
            (d / f"b{block}" / (name + ".gz")).write_bytes(Z.bgzf((d / name).read_bytes(), block)[0])
    return d, golden_args(golden)


def run_tool(exe, d, args, out):
    return subprocess.run([exe, *args, "-o", out], cwd=str(d), capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("which", ["bucketmap", "bucketmap_align"])
def test_oracle_tools_read_compressed_inputs(tool_inputs, which):
    d, args = tool_inputs
    exe = TOOLS[(which, "oracle")]
    r = run_tool(exe, d, args, f"{which}_plain.sam")
    assert r.returncode == 0, r.stderr
    want = (d / f"{which}_plain.sam").read_bytes()
    assert want.count(b"\n") > 40
    for block in (997, 65280):
        for k, (reads, genome) in enumerate((("reads.fastq.gz", "g.fa"), ("reads.fastq", "g.fa.gz"), ("reads.fastq.gz", "g.fa.gz"))):
            reads, genome = (f"b{block}/{p}" if p.endswith(".gz") else p for p in (reads, genome))
            out = f"{which}_{block}_{k}.sam"
            r = run_tool(exe, d, compressed_args(args, reads, genome), out)
            assert r.returncode == 0, r.stderr
            assert (d / out).read_bytes() == want, (block, reads, genome)


def test_oracle_tool_refuses_plain_gzip_and_names_a_bad_block(tool_inputs):
    d, args = tool_inputs
    exe = TOOLS[("bucketmap", "oracle")]
    (d / "plain.fastq.gz").write_bytes(gzip.compress((d / "reads.fastq").read_bytes()))
    r = run_tool(exe, d, compressed_args(args, "plain.fastq.gz", "g.fa"), "refused.sam")
    assert r.returncode != 0 and "bgzip" in r.stderr and not (d / "refused.sam").exists(), r.stderr
    blob = bytearray((d / "b997" / "reads.fastq.gz").read_bytes())
    in_off = Z.bgzf((d / "reads.fastq").read_bytes(), 997)[1]
    blob[in_off[3] + 18 + 20] ^= 0x04                                   # a payload byte of block 3
    (d / "flipped.fastq.gz").write_bytes(bytes(blob))
    r = run_tool(exe, d, compressed_args(args, "flipped.fastq.gz", "g.fa"), "flipped.sam")
    assert r.returncode != 0 and "block 3" in r.stderr, r.stderr
