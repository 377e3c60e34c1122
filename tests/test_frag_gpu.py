"""The fragment range learned from the data, on the GPU: the span kernel against the plain-numpy contract verify.frag_spans,
the histogram kernel (both of its paths) against np.bincount, bmv_paired_begin + bmv_paired_finish against bmv_align_paired,
the histograms of two shares against the whole batch's, and the tool's --frag-auto against the oracle-backed tool's."""
import os
import subprocess

import numpy as np
import pytest

from test_frag import SMALL_GROUPS, flatten_frag, frag_edge_cases
from test_pair import random_pairs
from test_pair_gpu import SIZES, _arrays, build_pairs_batch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GPU_TOOL = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
ORACLE_TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")
LDS_BINS = 16384                # bmv_frag.hip.h: cap + 1 up to this is counted in LDS


def _check_spans(v, arrays, cap, contig, what):
    from bucket_map_amd import verify
    ts, tl, trc, ql, ed, en, off = arrays
    got = v.frag_spans(ts, tl, trc, ql, ed, en, off, cap, contig)
    want = verify.frag_spans(ts, tl, trc, ql, ed, en, off, cap, contig)
    bad = np.flatnonzero(got["span"] != want)
    assert bad.size == 0, f"{what}: span differs at {bad[:8]}: got {got['span'][bad[:8]]}, want {want[bad[:8]]}"
    assert np.array_equal(got["hist"], verify.frag_histogram(want, cap)), f"{what}: the histogram differs"
    assert v.frag_stats()["n_informative"] == int((want != 0).sum()) == int(got["hist"][1:].sum()), what
    return got


def _sized_frag_pairs():
    """test_pair_gpu._sized_pairs' construction for the settled test: every ordered pair of group sizes out of SIZES; all
    candidates of a group lie at ONE locus (the same alignment through windows shifted by k) but for at most one, at the first,
    the last, the 64th or the 65th index of either group -- the lane-chunk borders --, which lies 7 bases further.  The winner
    (edits 0) is never the off-locus one unless the group has one candidate."""
    ts, tl, trc, ql, ed, en, off, where = [], [], [], [], [], [], [0], []
    spots = lambda size: [None] + sorted({x for x in (0, size - 1, 63, 64) if 0 <= x < size and size > 1})      # noqa: E731
    for sa in SIZES:
        for sb in SIZES:
            for pa in spots(sa):
                for pb in spots(sb):
                    for size, at, rc in ((sa, pa, 0), (sb, pb, 1)):
                        win = 1 if at == 0 else 0
                        for k in range(size):
                            m, away = 100, (7 if k == at else 0)
                            # forward: R = 1 100 + away whatever k; reverse: L = 1 300 + away whatever k
                            if rc == 0:
                                ts.append(1000 - 5 - k + away); tl.append(m + 15 + k); en.append(m + 5 + k)
                            else:
                                ts.append(1300 - 10 + away); tl.append(m + 15 + k); en.append(m + 5 + k)
                            trc.append(rc); ql.append(m)
                            ed.append(0 if k == win else 3)
                        off.append(len(ts))
                    where.append((sa, sb, pa, pb))
    return _arrays(ts, tl, trc, ql, ed, en, off), where


@pytest.mark.gpu
def test_span_kernel_over_group_sizes():
    """Groups of 0, 1, 2, 63, 64, 65 and 130 candidates in every order, the one candidate that unsettles a group at the chunk
    borders of either mate."""
    from bucket_map_amd import verify
    arrays, where = _sized_frag_pairs()
    v = verify.Verifier()
    got = _check_spans(v, arrays, 1000, None, "sizes")["span"]
    for p, (sa, sb, pa, pb) in enumerate(where):
        assert got[p] == (400 if sa and sb and pa is None and pb is None else 0), (sa, sb, pa, pb)
    assert (got == 400).sum() == 36
    # the off-locus candidates unknown: every pair of two non-empty groups is informative again
    ts, tl, trc, ql, ed, en, off = (x.copy() for x in arrays)
    at = 0
    for p, (sa, sb, pa, pb) in enumerate(where):
        for size, spot in ((sa, pa), (sb, pb)):
            if spot is not None:
                ed[at + spot] = verify.BEYOND
            at += size
    got = _check_spans(v, (ts, tl, trc, ql, ed, en, off), 1000, None, "off-locus candidates unknown")["span"]
    assert all(got[p] == (400 if sa and sb else 0) for p, (sa, sb, _, _) in enumerate(where))
    v.close()


@pytest.mark.gpu
def test_span_kernel_edge_cases_and_random_pairs():
    from bucket_map_amd import verify
    v = verify.Verifier()
    cases = frag_edge_cases()
    arrays = _arrays(*flatten_frag(cases.values()))
    got = _check_spans(v, arrays, 500, None, "edge cases")
    assert dict(zip(cases, got["span"].tolist())) == {k: c[2] for k, c in cases.items()}
    ctg = np.zeros(len(arrays[0]), np.uint32)
    ctg[arrays[6][1]] = 7
    assert _check_spans(v, arrays, 500, ctg, "edge cases, contigs")["span"][0] == 0
    rng = np.random.default_rng(20251001)
    for kind in (dict(), SMALL_GROUPS):                                    # the CPU test's pairs
        ts, tl, trc, ql, ed, en, ctg, off = random_pairs(rng, 400, **kind)
        for contig in (np.array(ctg, np.uint32), None):
            for cap in (1, 300, 1000, 65535):
                _check_spans(v, _arrays(ts, tl, trc, ql, ed, en, off), cap, contig, f"the CPU test's pairs, cap {cap}")
    # refusals: nothing ran, the context stays usable and bmv_frag keeps what it held
    arrays = _arrays(ts, tl, trc, ql, ed, en, off)
    held = _check_spans(v, arrays, 700, None, "before the refusals")
    odd = np.append(arrays[6], arrays[6][-1])
    for bad, cap, words in (((*arrays[:6], odd), 700, "groups"), (arrays, 0, "cap"), (arrays, 65536, "cap")):
        with pytest.raises(verify.BmvError) as e:
            v.frag_spans(*bad, cap)
        assert e.value.code == 1 and words in str(e.value)
    after = v.frag(len(arrays[6]) // 2, 700)
    assert np.array_equal(after["span"], held["span"]) and np.array_equal(after["hist"], held["hist"])
    # n_groups = 0
    empty = v.frag_spans(*(np.zeros(0, t) for t in (np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32)), np.zeros(1, np.uint32), 300)
    assert len(empty["span"]) == 0 and len(empty["hist"]) == 301 and empty["hist"].sum() == 0
    assert v.frag_stats()["n_informative"] == 0
    v.close()


def _span_pairs(spans):
    """One pair per span: a forward candidate with L = 1 000 and a reverse one with R = 1 000 + span (span 0: an empty second
    group) -- numbers whose span is known beforehand."""
    spans = np.asarray(spans, np.int64)
    n = len(spans)
    some = spans > 0
    m = np.where(some, np.minimum(spans, 50), 50)
    ts, tl, trc, ql, ed, en = (np.zeros(2 * n, t) for t in (np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32))
    ts[0::2], tl[0::2], ql[0::2], en[0::2] = 1000, m + 10, m, m                         # forward: R = 1 000 + m, L = 1 000
    ts[1::2], tl[1::2], ql[1::2], en[1::2], trc[1::2] = 1000 + spans - m, m + 10, m, m + 10, 1    # reverse: L = ts, R = ts + m
    keep = np.ones(2 * n, bool)
    keep[1::2] = some
    off = np.concatenate([[0], np.cumsum(keep)]).astype(np.uint32)
    return tuple(x[keep] for x in (ts, tl, trc, ql, ed, en)) + (off,)


@pytest.mark.gpu
def test_histogram_against_bincount():
    """Both paths of the histogram kernel -- private bins in LDS up to 16 384 of them, global atomics beyond --, contention,
    pair counts around the block size, and a reused context after a larger batch and after a larger cap."""
    from bucket_map_amd import verify
    v = verify.Verifier()
    rng = np.random.default_rng(20251020)

    def run(spans, cap, what):
        got = _check_spans(v, _span_pairs(spans), cap, None, what)
        want = np.bincount(np.asarray(spans, np.int64), minlength=cap + 1).astype(np.uint64)
        assert np.array_equal(got["span"], np.asarray(spans, np.uint32)), what
        assert np.array_equal(got["hist"], want), what
        assert got["hist"].sum() == len(spans), what

    spread = rng.integers(0, 10_001, 20_000)
    spread[:3] = (0, 1, 10_000)
    wide = rng.integers(0, 65_536, 20_000)
    wide[:3] = (0, 1, 65_535)
    run(wide, 65_535, "20 000 pairs over cap 65 535: global atomics")
    run(spread, 10_000, "20 000 pairs over cap 10 000: LDS bins, after a larger cap")           # stale bins would show here
    run(np.full(20_000, 777), 10_000, "20 000 pairs in one bin: contention in LDS")
    run(np.full(20_000, 40_000), 65_535, "20 000 pairs in one bin: contention on one global counter")
    run([], 10_000, "0 pairs")
    run([5], 10_000, "1 pair, after a larger batch")
    run([0], 10_000, "1 uninformative pair")
    run([1, 0, 1], 1, "cap 1")
    run(rng.integers(0, 301, 256 * 8 + 1), 300, "one pair more than a block's share")
    run(rng.integers(0, 301, 255), 300, "less than a block")
    run(rng.integers(0, LDS_BINS, 5000), LDS_BINS - 1, "the largest cap counted in LDS")
    run(rng.integers(0, LDS_BINS + 1, 5000), LDS_BINS, "the smallest cap counted by global atomics")
    run(spread, 10_000, "the first batch again")
    v.close()


@pytest.fixture(scope="module")
def frag_batch():
    """test_pair_gpu's 300-pair batch with a verifier that holds its genome."""
    from bucket_map_amd import verify
    genome, batch, off, margin = build_pairs_batch()
    v = verify.Verifier()
    v.load_genome(genome)
    return {"v": v, "genome": genome, "batch": batch, "off": off, "margin": margin}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), f"{what}: {key} differs"


@pytest.mark.gpu
def test_begin_and_finish_equal_align_paired(frag_batch):
    from bucket_map_amd import verify
    fb = frag_batch
    v, batch, off, margin = fb["v"], fb["batch"], fb["off"], fb["margin"]
    sizes = np.maximum(np.diff(off.astype(np.int64)), 1)
    contig = (batch[1] >= 15_000).astype(np.uint32)
    n_pairs = (len(off) - 1) // 2
    spans = None
    for hint_name, hint in (("none", None), ("last", (sizes - 1).astype(np.uint32))):
        for lo, hi in ((200, 800), (1, 400)):
            want = v.align_paired(*batch, off, margin, lo, hi, hint, contig)
            want_stats = v.best_stats()
            frag = v.paired_begin(*batch, off, margin, 1000, hint, contig)
            got = v.paired_finish(lo, hi)
            _same(got, want, f"hint {hint_name}, {lo}..{hi}")
            stats = v.best_stats()
            assert {k: stats[k] for k in stats if not k.startswith("ms")} == {k: want_stats[k] for k in stats if not k.startswith("ms")}
            # the spans: frag_spans over what bmv_best returns, whatever the hint
            ref = verify.frag_spans(batch[1], batch[2], batch[3], batch[5], want["edits"], want["end"], off, 1000, contig)
            assert np.array_equal(frag["span"], ref) and np.array_equal(frag["hist"], verify.frag_histogram(ref, 1000))
            assert spans is None or np.array_equal(spans, ref)
            spans = ref
    assert (spans != 0).sum() > 50, "the fixture shows nothing: hardly any informative pair"
    assert v.frag_stats()["n_informative"] == int((spans != 0).sum())
    # cap = 0 skips the frag kernels: bmv_frag keeps what it returned before
    v.frag_spans(batch[1][:0], batch[2][:0], batch[3][:0], batch[5][:0], [], [], [0, 0, 0], 7)
    assert v.paired_begin(*batch, off, margin, 0, None, contig) is None
    kept = v.frag(1, 7)
    assert kept["span"].tolist() == [0] and kept["hist"].tolist() == [1] + [0] * 7
    _same(v.paired_finish(200, 800), v.align_paired(*batch, off, margin, 200, 800, None, contig), "cap 0")
    # a refused begin (cap beyond 65 535, an odd number of groups) ends the begin before it: finish has nothing to finish
    for bad_off, bad_margin, cap, words in ((off, margin, 65_536, "cap"),
                                            (np.append(off, off[-1]), np.append(margin, 1).astype(np.uint32), 1000, "groups")):
        v.paired_begin(*batch, off, margin, 1000, None, contig)
        with pytest.raises(verify.BmvError) as e:
            v.paired_begin(*batch, bad_off, bad_margin, cap)
        assert e.value.code == 1 and words in str(e.value)
        with pytest.raises(verify.BmvError) as e:
            v.paired_finish(200, 800)
        assert e.value.code == 3 and "bmv_paired_finish" in str(e.value)
    v.paired_begin(*batch, off, margin, 1000, None, contig)
    _same(v.paired_finish(200, 800), v.align_paired(*batch, off, margin, 200, 800, None, contig), "after the refused begins")
    assert n_pairs == 300


@pytest.mark.gpu
def test_state_rules_of_begin_and_finish(frag_batch):
    from bucket_map_amd import verify
    fb = frag_batch
    batch, off, margin = fb["batch"], fb["off"], fb["margin"]
    v = verify.Verifier()
    v.load_genome(fb["genome"])

    def refused_for_state():
        with pytest.raises(verify.BmvError) as e:
            v.paired_finish(200, 800)
        assert e.value.code == 3 and "bmv_paired_finish" in str(e.value)

    refused_for_state()                                                     # finish without begin
    want = v.align_paired(*batch, off, margin, 200, 800)
    refused_for_state()                                                     # align_paired leaves nothing pending
    v.paired_begin(*batch, off, margin, 1000)
    _same(v.paired_finish(200, 800), want, "begin + finish")
    refused_for_state()                                                     # finish twice
    _same(v._pairs(len(off) - 1), {k: want[k] for k in ("pick", "proper", "s1", "s2", "winner")}, "a refused finish changes nothing")
    v.paired_begin(*batch, off, margin, 1000)
    few = tuple(x[:4] for x in batch[1:])
    v.align(batch[0], *few)                                                 # bmv_align in between
    refused_for_state()
    # bmv_frag_spans, bmv_pair and the accessors in between are fine, also with larger arrays than the batch's
    frag = v.paired_begin(*batch, off, margin, 1000)
    rp = random_pairs(np.random.default_rng(5), 2000)
    big = _arrays(*rp[:6], rp[7])
    v.frag_spans(*big, 300)
    v.pair(*big, 1, 1000)
    v.frag_stats(), v.pair_stats(), v.best_stats(), v.stats()
    _same(v.paired_finish(200, 800), want, "after frag_spans and pair in between")
    # a refused finish (min > max) leaves the begin pending
    v.paired_begin(*batch, off, margin, 1000)
    with pytest.raises(verify.BmvError) as e:
        v.paired_finish(801, 800)
    assert e.value.code == 1 and "min_frag" in str(e.value)
    _same(v.paired_finish(200, 800), want, "after a refused finish")
    again = v.frag(len(off) // 2, 1000)
    assert np.array_equal(again["span"], frag["span"]) and np.array_equal(again["hist"], frag["hist"])
    v.close()


@pytest.mark.gpu
def test_histograms_of_two_shares_add_up(frag_batch):
    """The batch cut at a pair border into two begin calls on two contexts: the summed histograms are the whole batch's, and
    either share's picks under one range are the whole batch's."""
    from bucket_map_amd import verify
    fb = frag_batch
    v, batch, off, margin = fb["v"], fb["batch"], fb["off"], fb["margin"]
    reads, ts, tl, trc, qs, ql = batch
    whole = v.paired_begin(*batch, off, margin, 1000)
    want = v.paired_finish(200, 800)
    w = verify.Verifier()
    w.load_genome(fb["genome"])
    g = 2 * 117                                                             # the first 117 pairs, the other 183
    a = int(off[g])
    first = v.paired_begin(reads, ts[:a], tl[:a], trc[:a], qs[:a], ql[:a], off[: g + 1], margin[:g], 1000)
    second = w.paired_begin(reads, ts[a:], tl[a:], trc[a:], qs[a:], ql[a:], off[g:] - off[g], margin[g:], 1000)
    assert np.array_equal(first["hist"] + second["hist"], whole["hist"])
    assert np.array_equal(np.concatenate([first["span"], second["span"]]), whole["span"])
    r1, r2 = v.paired_finish(200, 800), w.paired_finish(200, 800)
    assert np.array_equal(np.concatenate([r1["pick"], r2["pick"] + np.where(r2["pick"] == verify.BEYOND, 0, a).astype(np.uint32)]), want["pick"])
    assert np.array_equal(np.concatenate([r1["score"], r2["score"]]), want["score"])
    w.close()


@pytest.mark.gpu
def test_tool_equals_the_oracle_backed_tool(tmp_path):
    """bucketmap_align --frag-auto writes, byte for byte, what the oracle-backed tool writes on the CPU test's files -- SAM and
    range lines --, in one block and in blocks of 16 reads; --gpus 0,0 learns the same range and writes the same bytes."""
    from test_frag import make_frag_fixture, parse_range_lines, run_frag_tool
    d = tmp_path
    make_frag_fixture(d)
    for name, block, extra in (("one", "4096", ["--frag-auto", "--frag-min-pairs", "20"]), ("blocks", "16", ["--frag-cap", "2200", "--frag-min-pairs", "4"])):
        cpu = run_frag_tool(ORACLE_TOOL, d, "pairs.fastq", f"cpu_{name}.sam", *extra, block=block)
        gpu = run_frag_tool(GPU_TOOL, d, "pairs.fastq", f"gpu_{name}.sam", *extra, block=block)
        two = run_frag_tool(GPU_TOOL, d, "pairs.fastq", f"gpu2_{name}.sam", *extra, "--gpus", "0,0", block=block)
        want = parse_range_lines(cpu.stderr)
        assert want and any(x["learned"] for x in want)
        assert parse_range_lines(gpu.stderr) == want and parse_range_lines(two.stderr) == want, name
        assert "best per pair" in gpu.stderr and "the span and histogram kernels" in gpu.stderr
        assert (d / f"gpu_{name}.sam").read_bytes() == (d / f"cpu_{name}.sam").read_bytes(), name
        assert (d / f"gpu2_{name}.sam").read_bytes() == (d / f"gpu_{name}.sam").read_bytes(), f"{name}: --gpus 0,0 differs from --gpus 0"


@pytest.mark.gpu
def test_tool_rescues_under_the_learned_range(tmp_path):
    """The mate of a 2 kbp pair that no k-mer finds: under the default range rescue looks 1 000 bases far and misses it, under
    the range its block learned it is found, at its true place."""
    from test_frag import make_frag_fixture, parse_range_lines, run_frag_tool, sam_records
    d = tmp_path
    make_frag_fixture(d)
    run_frag_tool(GPU_TOOL, d, "rescue.fastq", "default.sam", "--rescue")
    mates = [r for r in sam_records(d / "default.sam") if r[0] == "r0"]
    assert not any("XR:i:1" in r for r in mates) and all(int(r[1]) & 0x2 == 0 for r in mates)
    r = run_frag_tool(GPU_TOOL, d, "rescue.fastq", "auto.sam", "--rescue", "--frag-auto", "--frag-min-pairs", "20")
    line = parse_range_lines(r.stderr)[0]
    assert line["learned"] and line["min"] <= 1900 and line["max"] >= 2300
    mates = [r for r in sam_records(d / "auto.sam") if r[0] == "r0"]
    assert len(mates) == 2 and all(int(r[1]) & 0x3 == 0x3 for r in mates)
    assert int(mates[0][3]) == 5001 and int(mates[1][3]) == 5000 + 2100 - 150 + 1 and "XR:i:1" in mates[1] and "XR:i:1" not in mates[0]
    cpu = run_frag_tool(ORACLE_TOOL, d, "rescue.fastq", "cpu_auto.sam", "--rescue", "--frag-auto", "--frag-min-pairs", "20")
    assert parse_range_lines(cpu.stderr) == parse_range_lines(r.stderr)
    assert (d / "cpu_auto.sam").read_bytes() == (d / "auto.sam").read_bytes()
