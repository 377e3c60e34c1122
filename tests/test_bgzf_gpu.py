"""bmz_deflate on the MI355X against the plain-Python rule (tests/bgzf_rule.py), byte for byte -- the blocks, their
offsets and the form counts -- and the product tools' -o x.bam against the oracle-backed tools' (whose blocks come from
host/bgzf.h): the compressor is deterministic, so the files are equal.  Every tool run has its own time limit; nothing is
retried."""
import json
import os
import random
import struct
import subprocess

import pytest

import bgzf_rule as R
from test_bgzf import CASES, GPU_ONLY_RUNS, RUNS, bam_to_sam, fold_seq, golden_args
from test_pair import ARGS as PAIR_ARGS, make_paired_fixture
from test_sam_golden import ROOT, TOOLS, write_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    from bucket_map_amd import bgzf
    c = bgzf.Compressor(0)
    yield c
    c.close()


def bam_like(n, seed):
    """n bytes that look like a BAM stream: fixed-width little-endian fields, names, 4-bit bases, qualities, tags."""
    rng = random.Random(seed)
    out = bytearray()
    k = 0
    while len(out) < n:
        l_seq = rng.choice((100, 150, 151))
        name = f"read{seed}.{k}".encode() + b"\0"
        cigar = struct.pack("<I", l_seq << 4 | 7)
        seq = bytes(rng.choice((0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88))
                    for _ in range((l_seq + 1) // 2))
        qual = bytes(min(41, max(2, int(rng.gauss(36, 4)))) for _ in range(l_seq))
        tags = b"NMC" + bytes([rng.randrange(3)]) + b"MDZ" + str(l_seq).encode() + b"\0"
        body = struct.pack("<iiBBHHHIiii", 0, rng.randrange(1 << 27), len(name), 60, 4681, 1, rng.choice((0, 16)), l_seq, -1, -1, 0)
        body += name + cigar + seq + qual + tags
        out += struct.pack("<I", len(body)) + body
        k += 1
    return bytes(out[:n])


def check(z, data, block_bytes=R.BLOCK_MAX):
    got, offsets, forms = z.deflate(data, block_bytes)
    want, want_offsets, want_forms = R.deflate(data, block_bytes)
    assert offsets == want_offsets and forms == want_forms
    assert got == want
    return got, offsets


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_rule(z, name):
    check(z, CASES[name])


def test_three_full_blocks_and_a_tail(z):
    got, offsets = check(z, bam_like(3 * R.BLOCK_MAX + 1234, 1))
    assert len(offsets) == 5


@pytest.fixture(scope="module")
def payloads():
    """(1 200 blocks' worth at 300 bytes a block, four full blocks: two BAM-like, a random and a constant one)"""
    return bam_like(1200 * 300, 2), bam_like(2 * R.BLOCK_MAX, 3) + CASES["random"] + CASES["equal"]


def test_more_blocks_than_workgroups_between_full_blocks(z, payloads):
    """1 200 blocks of 300 bytes are more than the resident workgroups: the persistent loop and the packed placement; a call
    of four full blocks before and after it on the same context changes nothing."""
    SMALL, FULL = payloads
    full, _ = check(z, FULL)
    small, offsets = check(z, SMALL, 300)
    assert len(offsets) == 1201
    assert z.deflate(FULL)[0] == full and z.deflate(SMALL, 300)[0] == small


def test_bytes_do_not_depend_on_the_batch(z, payloads):
    FULL = payloads[1]
    blocks = [FULL[i * R.BLOCK_MAX: (i + 1) * R.BLOCK_MAX] for i in range(4)]
    alone = [z.deflate(b)[0] for b in blocks]
    assert alone == [R.deflate_block(b)[0] for b in blocks]
    other = blocks[3] + blocks[1] + bam_like(R.BLOCK_MAX, 4) + blocks[0] + blocks[2] + blocks[2][:777]
    got, offsets, _ = z.deflate(other)
    for place, b in ((0, 3), (1, 1), (3, 0), (4, 2)):
        assert got[offsets[place]: offsets[place + 1]] == alone[b]


def test_small_after_large_and_large_after_small(z, payloads):
    from bucket_map_amd import bgzf
    small, large = CASES["len515"], payloads[1] + payloads[0]
    want_small, want_large = R.deflate(small)[0], z.deflate(large)[0]
    assert z.deflate(small)[0] == want_small               # on a context that just served the large call
    fresh = bgzf.Compressor(0)
    try:
        assert fresh.deflate(small)[0] == want_small
        assert fresh.deflate(large)[0] == want_large       # ... and the reverse
        assert fresh.deflate(b"") == (b"", [0], [0, 0, 0])
    finally:
        fresh.close()


def test_refusals_leave_the_context_usable(z):
    from bucket_map_amd import bgzf
    data = CASES["len65279"]
    for kwargs in (dict(block_bytes=0), dict(block_bytes=65281), dict(out_cap=bgzf.bound(len(data)) - 1)):
        with pytest.raises(bgzf.BmzError) as e:
            z.deflate(data, **kwargs)
        assert e.value.code == bgzf.BMZ_ERR_ARG
    check(z, data)


# ---- the tools ----
def run(exe, d, args, out, extra=(), limit=120):
    r = subprocess.run([exe, *args, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, timeout=limit)
    assert r.returncode == 0, r.stderr
    return d / out


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_gpu")
    with open(os.path.join(ROOT, "tests", "golden", "sam_small.json")) as f:
        golden = json.load(f)
    write_inputs(golden, d)
    return d, golden_args(golden)


@pytest.mark.parametrize("k", range(len(RUNS)))
def test_gpu_tool_writes_the_oracle_tools_bam(inputs, k):
    d, args = inputs
    which, extra = RUNS[k]
    want = run(TOOLS[(which, "oracle")], d, args, f"o{k}.bam", extra).read_bytes()
    assert run(TOOLS[(which, "gpu")], d, args, f"g{k}.bam", extra).read_bytes() == want
    assert run(TOOLS[(which, "gpu")], d, args, f"gg{k}.bam", [*extra, "--gpus", "0,0"]).read_bytes() == want
    sam = run(TOOLS[(which, "gpu")], d, args, f"g{k}.sam", extra).read_text()
    assert bam_to_sam(d / f"g{k}.bam")[0] == fold_seq(sam)


@pytest.mark.parametrize("k", range(len(GPU_ONLY_RUNS)))
def test_gpu_tool_bam_decodes_to_its_sam(inputs, k):
    d, args = inputs
    which, extra = GPU_ONLY_RUNS[k]
    sam = run(TOOLS[(which, "gpu")], d, args, f"c{k}.sam", extra).read_text()
    run(TOOLS[(which, "gpu")], d, args, f"c{k}.bam", extra)
    assert bam_to_sam(d / f"c{k}.bam")[0] == fold_seq(sam)
    assert "AS:i" in sam


def test_gpu_paired_rescue_bam(tmp_path):
    make_paired_fixture(tmp_path)
    args, extra = [*PAIR_ARGS, "-q", "pairs.fastq"], ["--paired", "--rescue"]
    want = run(TOOLS[("bucketmap_align", "oracle")], tmp_path, args, "o.bam", extra).read_bytes()
    assert run(TOOLS[("bucketmap_align", "gpu")], tmp_path, args, "g.bam", extra).read_bytes() == want
    sam = run(TOOLS[("bucketmap_align", "gpu")], tmp_path, args, "g.sam", extra).read_text()
    assert bam_to_sam(tmp_path / "g.bam")[0] == fold_seq(sam)
