"""bmc_begin / bmc_add / bmc_finish / bmc_runs / bmc_depth_at on the MI355X against the rule in plain Python
(tests/depth_rule.py) -- runs, the seven sums per reference and the depths themselves, all exactly --, and the product tools'
--depth / --coverage files and BAM against the oracle-backed tools' (whose counting is host/depth.h): the rule is exact, so the
files are equal.  Every tool run has its own time limit; nothing is retried."""
import numpy as np
import pytest

import depth_rule as D
from depth_cases import EDGE_REFS, REF_LENS, SIZES, edge_records, many_ops_record, random_records
from test_bamsort import offsets_of, pair_of
from test_markdup_gpu import rec, rec_ops, run
from test_sam_golden import TOOLS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def c():
    from bucket_map_amd import depth
    ctx = depth.Depth(0)
    yield ctx
    ctx.close()


def check(c, recs, ref_len, skip=None, cuts=None, want=None):
    """The device's result for the records (added in the stretches cuts names) is the rule's; returns the rule's."""
    want = D.count(recs, ref_len, skip) if want is None else want
    cuts = [0, len(recs)] if cuts is None else cuts
    c.begin(ref_len)
    for a, b in zip(cuts, cuts[1:]):
        c.add(b"".join(recs[a:b]), offsets_of(recs[a:b]), None if skip is None else skip[a:b])
    n_runs, stats = c.finish()
    assert stats.tolist() == want.stats
    assert n_runs == len(want.runs)
    assert [tuple(r) for r in c.runs().tolist()] == want.runs
    for r, length in enumerate(ref_len):                 # the depths themselves: whole references, and a stretch inside one
        if length <= 100000:
            assert np.array_equal(c.depth_at(r, 0, length), want.depth[r]), r
        lo, n = length // 3, min(length - length // 3, 5000)
        assert np.array_equal(c.depth_at(r, lo, n), want.depth[r][lo: lo + n]), r
        assert np.array_equal(c.depth_at(r, length - 1, 1), want.depth[r][-1:]) and c.depth_at(r, length, 0).size == 0
    if n_runs > 2:
        assert [tuple(r) for r in c.runs(1, n_runs - 2).tolist()] == want.runs[1:-1] and c.runs(n_runs, 0).shape == (0, 4)
    return want


@pytest.mark.parametrize("n", SIZES)
def test_sizes(c, n):
    recs = random_records(n, 300 + n)
    want = check(c, recs, REF_LENS)
    if n >= 257:
        assert all(s[0] for s in want.stats[1:]) and len(want.runs) > 50 and sum(s[5] for s in want.stats) > 1000
    if n:
        assert c.ms_add > 0 and c.ms_finish > 0


def test_depth_beyond_16_bits(c):
    recs = [rec(1, 5, 0, "1M", bytes([k % 256]), b"d%d" % k) for k in range(70001)] + [rec(1, 3, 0, "4M", bytes(4)), rec(0, 0, 0, "9M", b"")]
    want = check(c, recs, [9, 10])
    assert want.runs == [(0, 0, 9, 1), (1, 3, 5, 1), (1, 5, 6, 70002), (1, 6, 7, 1)] and want.stats[1][0] == 70002


def test_one_block_carried_across_many_scan_tiles(c):
    """600000M on 600 001 bases: one +1 carried over 293 tiles of 2 048, the second trip of the scan's sums kernel."""
    long = rec(0, 0, 0, "600000M", b"", b"long")
    want = check(c, [long, rec(1, 2, 0, "3M", b"abc")], [600001, 7])
    assert want.runs == [(0, 0, 600000, 1), (1, 2, 5, 1)] and want.stats[0][1:3] == [600000, 600000]
    assert c.depth_at(0, 599990, 11).tolist() == [1] * 10 + [0]


def test_a_record_of_many_ops_beside_short_ones(c):
    refs = [90000, 300]
    recs = random_records(150, 5, refs) + [many_ops_record(0, 17)] + random_records(150, 6, refs) + [many_ops_record(0, 60000, with_sequence=False)]
    want = check(c, recs, refs)
    assert want.stats[0][2] > 50000 and want.stats[0][5] > 50000
    # a long block with a sequence: the wave shares its quality bytes; with it a record whose blocks start beyond the end
    qual = np.random.default_rng(3).integers(0, 256, 200003).astype(np.uint8)
    wide = [rec(0, 1000, 0, "3S200000M", qual.tobytes(), b"wide"), rec(0, 89990, 0, "5M20D70000M", qual[:70005].tobytes(), b"off")]
    want = check(c, recs[:20] + wide + recs[20:40], refs)
    assert want.stats[0][5] > 89000


def test_edge_list(c):
    recs = edge_records()
    assert {len(r) % 16 for r in recs} == set(range(16))
    want = check(c, recs, EDGE_REFS)
    assert want.stats[1][6] == 1 and (0, 100, 120, 1) in D.count(recs[17:19], EDGE_REFS).runs
    for size in (1, 7, 40):                              # the same records as the first and the last of a stream
        check(c, recs[:size], EDGE_REFS)
        check(c, recs[-size:], EDGE_REFS)
    for r in recs[:33]:                                  # and each alone
        check(c, [r], EDGE_REFS)


def test_skip_bytes_equal_removing_the_records(c):
    recs = random_records(3000, 77)
    skip = [int(k % 3 == 1) for k in range(3000)]
    want = check(c, recs, REF_LENS, skip)
    kept = [r for r, s in zip(recs, skip) if not s]
    assert check(c, kept, REF_LENS, want=want) is want
    assert want.stats != D.count(recs, REF_LENS).stats


def test_cutting_and_order_do_not_matter(c):
    recs = random_records(3001, 21)
    want = check(c, recs, REF_LENS)
    check(c, recs, REF_LENS, cuts=[0, 1000, 1002, 3001], want=want)
    check(c, recs, REF_LENS, cuts=[0, 0, 1, 3001], want=want)
    order = np.random.default_rng(4).permutation(3001)
    check(c, [recs[i] for i in order], REF_LENS, cuts=[0, 64, 3001], want=want)


def test_small_after_large_and_refusals_between(c):
    from bucket_map_amd import depth
    big = [3000000, 70000, 5]
    check(c, random_records(20001, 31, big), big)
    small = edge_records()
    check(c, small, EDGE_REFS)                            # nothing stale: smaller references, fewer records
    good = random_records(300, 8, EDGE_REFS)
    want = D.count(good, EDGE_REFS)
    c.begin(EDGE_REFS)
    c.add(b"".join(good[:100]), offsets_of(good[:100]))
    bad_off = offsets_of(good)
    bad_off[5] += 1
    refusals = [(b"".join(good), bad_off), ([rec_ops(0, 0, 0, [3 << 4 | 9], b"")], None), ([rec(0, 5, 0, "3M", b"ab")], None),
                ([rec(3, 5, 0, "3M", b"")], None)]
    for stream, off in refusals:                         # a refused add leaves what was added before
        if off is None:
            stream, off = b"".join(stream), offsets_of(stream)
        with pytest.raises(depth.BmcError) as e:
            c.add(stream, off)
        assert e.value.code == depth.BMC_ERR_ARG
    for call in (lambda: c.runs(0, 0), lambda: c.depth_at(0, 0, 1)):
        with pytest.raises(depth.BmcError) as e:
            call()
        assert e.value.code == depth.BMC_ERR_ARG and "no bmc_finish" in str(e.value)
    c.add(b"".join(good[100:]), offsets_of(good[100:]))
    n_runs, stats = c.finish()
    assert stats.tolist() == want.stats and [tuple(r) for r in c.runs().tolist()] == want.runs
    for call in (c.finish, lambda: c.add(b"".join(good), offsets_of(good)), lambda: c.runs(n_runs, 1), lambda: c.runs(0, n_runs + 1),
                 lambda: c.depth_at(3, 0, 1), lambda: c.depth_at(1, 45, 6), lambda: c.depth_at(2, 1, 1)):
        with pytest.raises(depth.BmcError) as e:
            call()
        assert e.value.code == depth.BMC_ERR_ARG
    assert [tuple(r) for r in c.runs().tolist()] == want.runs            # the result is still there
    for lens in ([], [4, 0], [2 ** 32 - 2 ** 20, 1]):
        with pytest.raises(depth.BmcError) as e:
            c.begin(lens)
        assert e.value.code == depth.BMC_ERR_ARG
    assert [tuple(r) for r in c.runs().tolist()] == want.runs
    check(c, small, EDGE_REFS)


def test_large_after_small_on_a_fresh_context():
    from bucket_map_amd import depth
    fresh = depth.Depth(0)
    try:
        with pytest.raises(depth.BmcError) as e:
            fresh.add(b"", [0])
        assert e.value.code == depth.BMC_ERR_ARG and "no bmc_begin" in str(e.value)
        with pytest.raises(depth.BmcError) as e:
            fresh.finish()
        assert e.value.code == depth.BMC_ERR_ARG
        fresh.begin([7])
        fresh.add(b"", [0])                              # no record: succeeds
        n_runs, stats = fresh.finish()
        assert n_runs == 0 and stats.tolist() == [[0] * 7] and fresh.runs().shape == (0, 4) and fresh.depth_at(0, 0, 7).tolist() == [0] * 7
        check(fresh, edge_records(), EDGE_REFS)
        big = [5, 3000000, 70000]
        check(fresh, random_records(20001, 33, big), big)
    finally:
        fresh.close()


# ---- the tools ----
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_markdup import markdup_jobs
    return markdup_jobs(tmp_path_factory)


def files_of(d, stem):
    return (d / f"{stem}.bedgraph").read_text(), (d / f"{stem}.cov").read_text(), pair_of(d, stem)


@pytest.mark.parametrize("k", [0, 1])
def test_gpu_tool_writes_the_oracle_tools_files(jobs, k):
    from test_depth import parse_coverage_line
    name, which, d, args, extra = jobs[k]
    opts = lambda stem: ["--depth", f"{stem}.bedgraph", "--coverage", f"{stem}.cov"]
    for mark in ([], ["--markdup"]):
        tag = name + ("m" if mark else "")
        err = run(TOOLS[(which, "oracle")], d, args, f"{tag}.co.bam", [*extra, *mark, *opts(f"{tag}.co")])
        want, told = files_of(d, f"{tag}.co"), parse_coverage_line(err)
        assert want[0].count("\n") > 10 and told[0] > 0
        err = run(TOOLS[(which, "gpu")], d, args, f"{tag}.c.bam", [*extra, *mark, *opts(f"{tag}.c")])
        assert "in 1 run(s)" in err and parse_coverage_line(err) == told
        assert files_of(d, f"{tag}.c") == want
        run(TOOLS[(which, "gpu")], d, args, f"{tag}.cg.bam", [*extra, *mark, *opts(f"{tag}.cg"), "--gpus", "0,0"])
        assert files_of(d, f"{tag}.cg") == want
        err = run(TOOLS[(which, "gpu")], d, args, f"{tag}.cr.bam", [*extra, *mark, *opts(f"{tag}.cr")], env=dict(BM_SORT_RUN_BYTES="2000"))
        assert "in 1 run(s)" not in err and parse_coverage_line(err) == told
        assert files_of(d, f"{tag}.cr") == want
    assert files_of(d, f"{name}.c")[:2] != files_of(d, f"{name}m.c")[:2]          # the duplicates are left out
