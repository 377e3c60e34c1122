"""bms_sort / bms_sort_deflate on the MI355X against plain Python (perm = sorted(range(n), key=lambda i: (key[i], i)), the
sorted stream by slicing), bms_sort_deflate against the BGZF rule of tests/bgzf_rule.py, and the product tools' --sort files
against the oracle-backed tools' (whose sort is std::stable_sort on the host): the order is exact, so the files are equal.
Every tool run has its own time limit; nothing is retried."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bgzf_rule as R
from test_bamsort import check_sorted_file, make_record, offsets_of, pair_of, raw_records, sort_reference, tool_jobs
from test_bgzf import GPU_ONLY_RUNS, RUNS
from test_sam_golden import TOOLS

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 70001, 300001]


@pytest.fixture(scope="module")
def s():
    from bucket_map_amd import bamsort
    c = bamsort.Sorter(0)
    yield c
    c.close()


# ---- streams of 38-byte records from arrays of (refID, pos), and their reference ----
def stream38(rid, pos):
    n = len(rid)
    a = np.zeros((n, 38), np.uint8)
    a[:, 0:4] = np.frombuffer(struct.pack("<I", 34), np.uint8)
    a[:, 4:8] = np.asarray(rid, np.int64).astype(np.uint32).astype("<u4").view(np.uint8).reshape(n, 4)
    a[:, 8:12] = np.asarray(pos, np.int64).astype(np.uint32).astype("<u4").view(np.uint8).reshape(n, 4)
    a[:, 12] = 2                                                  # l_read_name: one letter and the NUL
    a[:, 14:16] = np.frombuffer(struct.pack("<H", 4680), np.uint8)
    a[:, 36] = 97 + np.arange(n) % 26
    return a


def keys_of(rid, pos):
    r = np.asarray(rid, np.int64).astype(np.uint32).astype(np.uint64)
    p = (np.asarray(pos, np.int64) + 1).astype(np.uint32).astype(np.uint64)
    return [int(x) for x in (r << np.uint64(32)) | p]


def check38(s, rid, pos):
    n = len(rid)
    a = stream38(rid, pos)
    key = keys_of(rid, pos)
    perm = sorted(range(n), key=lambda i: (key[i], i))
    got, got_perm, got_so = s.sort(a.tobytes(), np.arange(n + 1, dtype=np.uint64) * 38)
    assert got_perm.tolist() == perm
    assert got_so.tolist() == [38 * k for k in range(n + 1)]
    assert got == a[np.asarray(perm, np.int64)].tobytes()
    return perm


def pattern(name, n, seed=5):
    rng = np.random.default_rng(seed + n)
    zero = np.zeros(n, np.int64)
    if name == "equal":
        return zero + 3, zero + 1000
    if name == "sorted":
        return zero, np.arange(n) * 3
    if name == "reversed":
        return zero, (n - np.arange(n)) * 3
    if name == "16keys":                                          # every one of the 16 occurs: n >= 65
        combo = rng.permutation(n) % 16
        return combo // 4, combo % 4 * 1000
    if name == "byte3":                                           # pos + 1 differs in its top byte alone
        top = rng.integers(0, 256, n)
        top[:2] = (0, 255)
        return zero + 2, (top << 24 | 0x123456) - 1
    if name == "ref-1or0":
        return rng.integers(-1, 1, n), rng.integers(0, 50, n)
    if name == "ref70000":
        rid = rng.integers(0, 70001, n)
        rid[:2] = (70000, 0)                                      # 0x011170 and 0: three bytes differ
        return rid, zero + 77
    if name == "pos_edges":
        return rng.integers(0, 3, n), rng.choice(np.array([-1, 0, 1, 2 ** 31 - 2]), n)
    assert name == "random"
    return rng.integers(-1, 25, n), rng.integers(-1, 2 ** 31 - 1, n)


PATTERNS = ["equal", "sorted", "reversed", "16keys", "byte3", "ref-1or0", "ref70000", "pos_edges", "random"]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(s, n):
    check38(s, *pattern("random", n))


@pytest.mark.parametrize("n", [x for x in SIZES if x >= 65])
@pytest.mark.parametrize("name", [p for p in PATTERNS if p != "random"])
def test_key_patterns(s, name, n):
    perm = check38(s, *pattern(name, n))
    if name == "equal":
        assert perm == list(range(n)) and s.n_passes == 0
    if name == "byte3":
        assert s.n_passes == 1
    if name == "ref70000":
        assert s.n_passes == 3                                    # refID bytes 0..2 are key bytes 4..6; pos is constant
    if name == "16keys":
        assert len({(a, b) for a, b in zip(*pattern(name, n))}) == 16


# ---- record lengths ----
def check_records(s, recs):
    perm, stream, so = sort_reference(recs)
    got, got_perm, got_so = s.sort(b"".join(recs), offsets_of(recs))
    assert got_perm.tolist() == perm and got_so.tolist() == so
    assert got == stream
    return got


def varied(n, seed, long=()):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n):
        size = 38 + (i * 37 + int(rng.integers(0, 363))) % 363    # 38 .. 400
        recs.append(make_record(int(rng.integers(-1, 3)), int(rng.integers(-1, 5000)), b"q", rng.bytes(size - 38)))
    for at, size in long:
        recs[at] = make_record(1, 2500 + at, b"L", rng.bytes(size - 38))
    return recs


def test_lengths_cover_every_residue(s):
    recs = varied(3000, 1)
    assert {len(r) % 16 for r in recs} == set(range(16)) and min(map(len, recs)) >= 38 and max(map(len, recs)) <= 400
    check_records(s, recs)


def test_long_records_among_short_ones(s):
    check_records(s, varied(1500, 2, long=((3, 70000), (700, 200000), (701, 70000), (1499, 200000))))


def test_one_record_of_a_mebibyte(s):
    big = make_record(0, 9, b"M", np.random.default_rng(3).bytes((1 << 20) - 38))
    assert len(big) == 1 << 20
    check_records(s, [big])
    check_records(s, [make_record(0, 10, b"a"), big, make_record(0, 8, b"b", b"xyz")])


# ---- a context used again ----
def test_small_after_large_and_a_refusal_between(s):
    from bucket_map_amd import bamsort
    check38(s, *pattern("random", 70001))
    small = varied(70, 4)
    bad = offsets_of(small)
    bad[5] += 1
    with pytest.raises(bamsort.BmsError) as e:
        s.sort(b"".join(small), bad)
    assert e.value.code == bamsort.BMS_ERR_ARG
    with pytest.raises(bamsort.BmsError) as e:
        s.sort_deflate(b"".join(small), offsets_of(small), block_bytes=0)
    assert e.value.code == bamsort.BMS_ERR_ARG
    check_records(s, small)


def test_large_after_small_on_a_fresh_context():
    from bucket_map_amd import bamsort
    fresh = bamsort.Sorter(0)
    try:
        check_records(fresh, varied(70, 4))
        check38(fresh, *pattern("random", 70001))
        got, perm, so = fresh.sort(b"", [0])
        assert (got, perm.tolist(), so.tolist()) == (b"", [], [0])
        assert fresh.sort_deflate(b"", [0])[0] == b""
    finally:
        fresh.close()


# ---- bms_sort_deflate ----
@pytest.mark.parametrize("case", ["two blocks", "four blocks", "small blocks"])
def test_sort_deflate_equals_the_rule(s, case):
    n, block = {"two blocks": (300, R.BLOCK_MAX), "four blocks": (1000, R.BLOCK_MAX), "small blocks": (40, 300)}[case]
    recs = varied(n, 6, long=((5, 30000),) if case == "four blocks" else ())
    perm, stream, so = sort_reference(recs)
    assert len(stream) <= 4 * R.BLOCK_MAX and (case != "four blocks" or len(stream) > 3 * R.BLOCK_MAX)
    got, got_perm, got_so = s.sort_deflate(b"".join(recs), offsets_of(recs), block)
    assert got_perm.tolist() == perm and got_so.tolist() == so
    assert got == R.deflate(stream, block)[0]
    assert s.ms_deflate > 0 and s.ms_gather > 0


def test_sort_deflate_of_many_records(s):
    from bucket_map_amd import bgzf
    rid, pos = pattern("random", 300001)
    stream, off = stream38(rid, pos).tobytes(), np.arange(300002, dtype=np.uint64) * 38
    sorted_stream, perm, so = s.sort(stream, off)
    got, got_perm, got_so = s.sort_deflate(stream, off)
    assert np.array_equal(got_perm, perm) and np.array_equal(got_so, so)
    z = bgzf.Compressor(0)
    try:
        assert got == z.deflate(sorted_stream)[0]
    finally:
        z.close()


# ---- the tools ----
def run(exe, d, args, out, extra=(), env=None, limit=120):
    r = subprocess.run([exe, *args, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, timeout=limit,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return r.stderr


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    out = tool_jobs(tmp_path_factory)
    d, args = out[0][2], out[0][3]
    for k, (which, extra) in enumerate(GPU_ONLY_RUNS):
        out.append((f"gpuonly{k}", which, d, args, list(extra)))
    return out


@pytest.fixture(scope="module")
def product(jobs):
    """The product's one-run --sort files of a job, made once."""
    made = {}

    def get(k):
        if k not in made:
            name, which, d, args, extra = jobs[k]
            err = run(TOOLS[(which, "gpu")], d, args, f"{name}.g.bam", [*extra, "--sort"])
            assert "in 1 run(s)" in err and "radix pass" in err
            made[k] = pair_of(d, f"{name}.g")
        return made[k]
    return get


N_JOBS = len(RUNS) + 1 + len(GPU_ONLY_RUNS)


@pytest.mark.parametrize("k", range(N_JOBS))
def test_gpu_tool_sorts_its_own_records(jobs, product, k):
    name, which, d, args, extra = jobs[k]
    bam, bai = product(k)
    run(TOOLS[(which, "gpu")], d, args, f"{name}.gu.bam", extra)
    unsorted = raw_records(d / f"{name}.gu.bam")
    got = check_sorted_file(bam, bai, 10, seed=k)
    assert len(got) > 10 and got == [unsorted[i] for i in sort_reference(unsorted)[0]]


@pytest.mark.parametrize("k", range(len(RUNS) + 1))
def test_gpu_tool_writes_the_oracle_tools_sorted_files(jobs, product, k):
    name, which, d, args, extra = jobs[k]
    run(TOOLS[(which, "oracle")], d, args, f"{name}.o.bam", [*extra, "--sort"])
    assert product(k) == pair_of(d, f"{name}.o")


@pytest.mark.parametrize("k", range(N_JOBS))
def test_gpu_tool_two_contexts_and_several_runs(jobs, product, k):
    name, which, d, args, extra = jobs[k]
    run(TOOLS[(which, "gpu")], d, args, f"{name}.gg.bam", [*extra, "--sort", "--gpus", "0,0"])
    assert pair_of(d, f"{name}.gg") == product(k)
    err = run(TOOLS[(which, "gpu")], d, args, f"{name}.gr.bam", [*extra, "--sort"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert "in 1 run(s)" not in err
    assert pair_of(d, f"{name}.gr") == product(k)
