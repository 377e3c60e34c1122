"""bmq_begin / bmq_add / bmq_finish / bmq_table on the MI355X against the rule in plain Python (tests/stats_rule.py) -- all 35
tallies and every row of the eight tables, exactly --, with the counters in LDS (the default window, a window of 64 and of 20
cycles) and with every cell by global atomics (BMQ_LDS_CYCLES=0), and the product tools' --stats file and stderr line against
the oracle-backed tools' (whose counter is host/stats.h): the rule is exact, so the files are equal.  Every tool run has its own
time limit; nothing is retried."""
import os

import numpy as np
import pytest

import stats_rule as Q
from stats_cases import DESIGNED, border_reads, long_read, ops_record, qrec, random_set, short_reads
from test_bamsort import offsets_of, pair_of
from test_markdup_gpu import rec, rec_ops, run
from test_sam_golden import TOOLS
from test_stats import stats_line

pytestmark = pytest.mark.gpu

WINDOWS = ("default", "0", "64", "20")                   # BMQ_LDS_CYCLES: unset, every cell global, one wave's worth, a border inside a 40-base read


def context(window):
    """A fresh bmq_ctx made under BMQ_LDS_CYCLES=window (the variable is read when the context is made)."""
    from bucket_map_amd import stats
    before = os.environ.pop("BMQ_LDS_CYCLES", None)
    try:
        if window != "default":
            os.environ["BMQ_LDS_CYCLES"] = window
        return stats.Stats(0)
    finally:
        os.environ.pop("BMQ_LDS_CYCLES", None)
        if before is not None:
            os.environ["BMQ_LDS_CYCLES"] = before


@pytest.fixture(scope="module")
def ctxs():
    made = {w: context(w) for w in WINDOWS}
    yield made
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def c(ctxs):
    return ctxs["default"]


def tables_of(c):
    return {name: c.table(name).astype(np.int64) for name in Q.TABLES}


def same(got, want):
    (t, tab), (want_t, want_tab) = got, want
    assert [int(x) for x in t] == [int(x) for x in want_t], [(Q.NAMES[k], int(a), int(b)) for k, (a, b) in enumerate(zip(t, want_t)) if int(a) != int(b)]
    for name in Q.TABLES:
        a, b = tab[name], want_tab[name]
        assert a.shape == b.shape, name
        assert np.array_equal(a, b), (name, [(r, col, int(a[r, col]), int(b[r, col])) for r, col in np.argwhere(a != b)[:6].tolist()])


def count(c, recs, skip=None, cuts=None, **params):
    """(tallies, tables) of the device for the records, added in the stretches cuts names."""
    cuts = [0, len(recs)] if cuts is None else cuts
    c.begin(**params)
    for a, b in zip(cuts, cuts[1:]):
        c.add(b"".join(recs[a:b]), offsets_of(recs[a:b]), None if skip is None else skip[a:b])
    t = c.finish()
    return t, tables_of(c)


def check(c, recs, skip=None, cuts=None, want=None, **params):
    want = Q.run(recs, skip, **params) if want is None else want
    same(count(c, recs, skip, cuts, **params), want)
    return want


def three(n):
    """Uneven cuts of n records into three stretches (some may be empty)."""
    return [0, n // 7, n // 7 + (2 * n + 2) // 3, n]


def device_rule(c):
    """The device as the engine of the designed cases, after everything has been compared with the Python rule too."""
    def rule(records, skip=None, **params):
        got = count(c, records, skip, **params)
        same(got, Q.run(records, skip, **params))
        return got
    return rule


_WANT = {}


def wanted(name, make, **params):
    """The record set `name` and the rule's result for it, computed once for all the tests that use it."""
    key = (name, tuple(sorted(params.items())))
    if name not in _WANT:
        _WANT[name] = make()
    if key not in _WANT:
        _WANT[key] = Q.run(_WANT[name], **params)
    return _WANT[name], _WANT[key]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("case", DESIGNED, ids=lambda f: f.__name__[5:])
def test_designed_cases(ctxs, case, window):
    case(device_rule(ctxs[window]))


@pytest.mark.parametrize("size", [1, 63, 64, 65, 257])
def test_random_records(ctxs, size):
    recs, want = wanted(f"random{size}", lambda: random_set(size, 70 + size))
    for window in WINDOWS:
        check(ctxs[window], recs, want=want)
    check(ctxs["default"], recs, cuts=three(size), want=want)
    check(ctxs["0"], recs, cuts=three(size), want=want)
    skip = [int(k % 3 == 1) for k in range(size)]
    check(ctxs["64"], recs, skip=skip, cuts=three(size))
    recs, want = wanted(f"random{size}", None, max_cycle=37, max_insert=50)      # the borders of C and I inside the data, and C below the windows
    for window in WINDOWS:
        check(ctxs[window], recs, want=want, max_cycle=37, max_insert=50)


@pytest.mark.parametrize("window", ["default", "0", "64"])
def test_many_short_reads(ctxs, window):
    """20 000 records of 150 bases: more than one trip of the grid-stride loops, and every workgroup flushes."""
    recs, want = wanted("short", lambda: short_reads(20000))
    assert want[0][Q.T["records"]] == 20000 and want[0][Q.T["pairs_in_is"]] == 10000 and want[1]["QC"][149].sum() > 15000
    check(ctxs[window], recs, want=want)
    if window != "64":
        check(ctxs[window], recs, cuts=three(20000), want=want)


@pytest.mark.parametrize("n_ops", [300, 5000])
def test_a_record_of_many_ops(ctxs, n_ops):
    recs, want = wanted(f"ops{n_ops}", lambda: [ops_record(n_ops, n_ops)])
    assert want[0][Q.T["aligned_records"]] == 1 and want[0][Q.T["insertions"]] > n_ops // 40
    for window in WINDOWS:
        check(ctxs[window], recs, want=want)
    more = recs + random_set(70, 5)
    check(ctxs["default"], more, cuts=three(71))
    check(ctxs["default"], more, max_cycle=100)


@pytest.mark.parametrize("max_cycle", [65535, 100])
def test_a_record_of_many_bases(ctxs, max_cycle):
    recs, want = wanted("long", lambda: [long_read(), long_read(9000, 12, 0)], max_cycle=max_cycle)
    assert want[0][Q.T["bases_beyond_cycle"]] == (70000 - 65535 if max_cycle == 65535 else 70000 + 9000 - 200)
    for window in ("default", "0", "64"):
        check(ctxs[window], recs, want=want, max_cycle=max_cycle)


def test_stretches_of_the_tables(c):
    recs, want = wanted("random257", lambda: random_set(257, 70 + 257))
    check(c, recs, want=want)
    whole = tables_of(c)
    for k, name in enumerate(Q.TABLES):
        n = whole[name].shape[0]
        for first, cnt in ((0, 1), (n // 3, n // 2), (n - 1, 1), (n, 0), (0, 0), (5, 17)):
            assert np.array_equal(c.table(k, first, cnt).astype(np.int64), whole[name][first: first + cnt]), (name, first, cnt)
    assert c.table("QC").shape == (1024, 64) and c.table("IS").shape == (8001, 3) and c.table("RL").shape == (1025, 1)


def test_reused_context_after_a_larger_batch(ctxs):
    from bucket_map_amd import stats
    recs, want = wanted("short", lambda: short_reads(20000))
    small = [qrec(0x61, "5M", "ACGTN", tlen=7), qrec(0x10, "2S3=", "GGCAT", [1, 2, 3, 4, 0xFF]), qrec(0x904, "", "AC")]
    for window in ("default", "0"):
        c = ctxs[window]
        check(c, recs, want=want)
        check(c, small, max_cycle=4, max_insert=9)       # exactly the rule's tables: nothing of the larger batch is left
        for which, rows in (("RL", 5), ("IS", 10), ("BC", 4), ("QC", 4), ("MC", 4), ("MAPQ", 256), ("GC", 101), ("ID", 256)):
            assert c.table(which, rows - 1, 1).shape[0] == 1
            for first, cnt in ((rows, 1), (rows - 1, 2), (0, rows + 1), (rows + 1, 0)):
                with pytest.raises(stats.BmqError) as e:
                    c.table(which, first, cnt)
                assert e.value.code == stats.BMQ_ERR_ARG and "bmq_table" in str(e.value)
        check(c, recs[:300])                             # ... and it grows again


def test_refusals_leave_the_earlier_records_counted(c):
    from bucket_map_amd import stats
    recs = random_set(65, 12)
    want = Q.run(recs)

    def refused(call, word):
        with pytest.raises(stats.BmqError) as e:
            call()
        assert e.value.code == stats.BMQ_ERR_ARG and word in str(e.value), str(e.value)

    c.begin()
    refused(lambda: c.table("MAPQ", 0, 1), "no bmq_finish")
    c.add(b"".join(recs[:40]), offsets_of(recs[:40]))
    bad_op = rec_ops(0, 0, 0, [3 << 4 | 9], b"")
    refused(lambda: c.add(recs[0] + bad_op, offsets_of([recs[0], bad_op])), "a CIGAR op is 0 .. 8")
    short = rec(0, 5, 0, "3M", b"ab")
    refused(lambda: c.add(recs[1] + short, offsets_of([recs[1], short])), "query bases")
    refused(lambda: c.add(recs[2], [0, len(recs[2]) - 1]), "bmq_add")
    refused(lambda: c.add(recs[2], [1, len(recs[2])]), "rec_offset[0]")
    refused(lambda: c.begin(max_cycle=0), "max_cycle")           # a refused bmq_begin starts nothing over
    refused(lambda: c.begin(max_insert=65536), "max_insert")
    c.max_cycle, c.max_insert = 1024, 8000
    c.add(b"", [0])                                      # no records: fine
    c.add(b"".join(recs[40:]), offsets_of(recs[40:]))
    t = c.finish()
    same((t, tables_of(c)), want)
    refused(lambda: c.finish(), "it has run already")
    refused(lambda: c.add(recs[0], offsets_of(recs[:1])), "bmq_finish has run")
    refused(lambda: c.table(8, 0, 1), "table 8")
    refused(lambda: c.table("GC", 101, 1), "bmq_table")
    same((t, tables_of(c)), want)                        # the tables are still there
    fresh = context("default")
    try:
        refused(lambda: fresh.add(recs[0], offsets_of(recs[:1])), "no bmq_begin")
        refused(lambda: fresh.finish(), "no bmq_begin")
        refused(lambda: fresh.table(0, 0, 1), "no bmq_finish")
        check(fresh, recs, want=want)
    finally:
        fresh.close()


def test_window_settings_give_equal_outputs_and_times_are_reported(ctxs):
    recs, want = wanted("border", border_reads, max_cycle=30)
    seen = []
    for window in WINDOWS:
        t, tab = count(ctxs[window], recs, max_cycle=30)
        seen.append(([int(x) for x in t], {k: v.tolist() for k, v in tab.items()}))
        assert ctxs[window].ms_add > 0 and ctxs[window].ms_finish >= 0
    assert all(s == seen[0] for s in seen[1:])
    same((seen[0][0], {k: np.asarray(v, np.int64).reshape(want[1][k].shape) for k, v in seen[0][1].items()}), want)
    big = context("100000")                              # more than the LDS holds: counts as the largest window
    try:
        check(big, recs, want=want, max_cycle=30)
        recs600, want600 = wanted("long", lambda: [long_read(), long_read(9000, 12, 0)], max_cycle=600)
        check(big, recs600, want=want600, max_cycle=600)  # the window's border at cycle 512
    finally:
        big.close()


# ---- the tools ----
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_markdup import markdup_jobs
    return markdup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", range(3))
def test_gpu_tool_writes_the_oracle_tools_file(jobs, k):
    name, which, d, args, extra = jobs[k]
    for tag, opts, env in (("one", [], None), ("runs", ["--markdup"], dict(BM_SORT_RUN_BYTES="2000"))):
        files = {}
        for kind in ("oracle", "gpu"):
            stem = f"{name}.{tag}.{kind}"
            err = run(TOOLS[(which, kind)], d, args, f"{stem}.bam", [*extra, *opts, "--stats", f"{stem}.txt"], env=env)
            assert ("in 1 run(s)" in err) == (env is None)
            files[kind] = (stats_line(err), (d / f"{stem}.txt").read_text(), pair_of(d, stem))
        assert files["gpu"] == files["oracle"]
        told, text = files["gpu"][:2]
        assert text.startswith("# bucketmap --stats 1\nSN\trecords\t") and int(told.split()[1]) > 20
        assert (tag == "runs") == (" 0 duplicates" not in told)


def test_gpu_tool_without_the_option_is_what_it_was(jobs):
    name, which, d, args, extra = jobs[0]
    err0 = run(TOOLS[(which, "gpu")], d, args, "n0.gpu.bam", [*extra, "--sort"])
    err = run(TOOLS[(which, "gpu")], d, args, "n1.gpu.bam", [*extra, "--stats", "n1.gpu.txt", "--stats-max-cycle", "100"])
    assert "Stats:" not in err0 and pair_of(d, "n0.gpu") == pair_of(d, "n1.gpu") and "\nBCC\t100\t" in (d / "n1.gpu.txt").read_text()
    assert "\nBCC\t101\t" not in (d / "n1.gpu.txt").read_text() and stats_line(err)
