"""bmb_begin / bmb_add / bmb_annotate / bmb_cells_at on the MI355X against the rule in plain Python (tests/bias_rule.py) -- all
five cells at every position and all 16 words of every annotation, exactly --, bmb's strand counts against bmg's on the device,
and the product tools' --vcf-bias files and stderr line against the oracle-backed tools' (whose annotating is host/bias.h): the
rule is exact, so the files are equal.  Every tool run has its own time limit; nothing is retried."""
import numpy as np
import pytest

import bias_rule as B
import genotype_rule as G
import pileup_rule as P
from pileup_cases import EDGE_REFS, REF_LENS, edge_bases, edge_records, many_ops_record, random_records, rec_letters, rec_seq, references
from test_bamsort import offsets_of, pair_of
from test_bias import bias_line, check_planted_lines, planted_pairs, variant_lines
from test_genotype import site, sites_for
from test_markdup_gpu import rec, rec_ops, run
from test_sam_golden import TOOLS

pytestmark = pytest.mark.gpu

STRICT = dict(min_mapq=20, min_bq=14)


@pytest.fixture(scope="module")
def c():
    from bucket_map_amd import bias
    ctx = bias.Bias(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def tables():
    from bucket_map_amd import bias
    return bias.tables()


@pytest.fixture(scope="module")
def ref_bases():
    return references()


def same_cells(c, want, ref_len):
    fwd, rev, n, S = want
    for r, length in enumerate(ref_len):
        strand, mapq = c.cells_at(r, 0, length)
        s_want, m_want = B.packed_strand(fwd[r], rev[r]), B.packed_mapq(n[r], S[r])
        assert np.array_equal(strand, s_want), (r, np.flatnonzero((strand != s_want).any(axis=1))[:10])
        assert np.array_equal(mapq, m_want), (r, np.flatnonzero(mapq != m_want)[:10])
        lo, count = length // 3, min(length - length // 3, 5000)
        part = c.cells_at(r, lo, count)
        assert np.array_equal(part[0], s_want[lo: lo + count]) and np.array_equal(part[1], m_want[lo: lo + count])
        assert c.cells_at(r, length, 0)[0].shape == (0, 4)


def same_notes(c, called, notes):
    got = c.annotate(np.asarray(called, np.uint32).reshape(-1, 24))
    assert got.shape == (len(called), 16)
    if got.tolist() != [list(x) for x in notes]:
        bad = [i for i, (a, b) in enumerate(zip(got.tolist(), notes)) if tuple(a) != tuple(b)][:3]
        assert False, [(i, got[i].tolist(), notes[i]) for i in bad]


def check(c, tables, recs, ref_len, called, skip=None, cuts=None, want=None, **params):
    """The device's cells and annotations for the records (added in the stretches cuts names) are the rule's; returns the rule's."""
    if want is None:
        cells = B.cells(recs, ref_len, skip, **params)
        want = (cells, B.annotate(called, *cells, *tables))
    cuts = [0, len(recs)] if cuts is None else cuts
    c.begin(ref_len, **params)
    for a, b in zip(cuts, cuts[1:]):
        c.add(b"".join(recs[a:b]), offsets_of(recs[a:b]), None if skip is None else skip[a:b])
    same_cells(c, want[0], ref_len)
    same_notes(c, called, want[1])
    return want


def calls_for(recs, ref_len, bases, **params):
    """bmg's calls by the Python rule at the pileup's sites under loose thresholds: variants, hom-ref calls and sites that are not
    genotyped."""
    sites = sites_for(recs, ref_len, bases, min_bq=0)
    return G.genotype(recs, ref_len, sites, **params)[2]


def kinds_of(notes):
    """(annotated with FS, annotated without, not annotated)"""
    return (sum(1 for b in notes if b[10] == 1), sum(1 for b in notes if b[10] == 3), sum(1 for b in notes if b[10] == 0))


@pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 257, 3001])
def test_sizes(c, tables, ref_bases, size):
    recs = random_records(size, 300 + size, bases=ref_bases)
    called = calls_for(recs, REF_LENS, ref_bases) if size > 1 else []
    (fwd, rev, n, S), notes = check(c, tables, recs, REF_LENS, called)
    if size >= 257:
        assert all(k > 3 for k in kinds_of(notes)[1:]) and sum(int(x.sum()) for x in fwd) > 1000 and sum(int(x.sum()) for x in rev) > 1000
        assert len({b[8] for b in notes}) > 20 and (size < 3001 or (kinds_of(notes)[0] > 3 and len({b[9] for b in notes}) > 3))
    if size:
        assert c.ms_add > 0 and (not called or c.ms_annotate > 0)


def test_edge_list(c, tables):
    recs, bases = edge_records(), edge_bases()
    assert {len(r) % 16 for r in recs} == set(range(16))
    for pr in ({}, STRICT, dict(min_bq=0), dict(min_bq=256, min_mapq=31)):
        called = calls_for(recs, EDGE_REFS, bases, **pr)
        check(c, tables, recs, EDGE_REFS, called, **pr)
    for size in (1, 7, 40):                              # the same records as the first and the last of a stream
        check(c, tables, recs[:size], EDGE_REFS, [], **STRICT)
        check(c, tables, recs[-size:], EDGE_REFS, [], **STRICT)


def test_a_record_of_many_ops_beside_short_ones(c, tables):
    """60 001 ops: 938 trips of the wave walk; the record is on the reverse strand, the short ones on either."""
    refs = [90000, 300]
    bases = references(refs, 4)
    long_rev = bytearray(many_ops_record(0, 60001, seed=8))
    long_rev[18] |= 0x10
    long_rev[13] = 255
    recs = random_records(150, 5, refs, bases) + [many_ops_record(0, 17)] + random_records(150, 6, refs, bases) + [bytes(long_rev)]
    called = calls_for(recs, refs, bases)
    (fwd, rev, n, S), notes = check(c, tables, recs, refs, called)
    assert int(rev[0].sum()) > 10000 and int(fwd[0].sum()) > 500 and int(S[0].max()) >= 255 * 255 and sum(kinds_of(notes)[:2]) > 100


def test_one_long_block_at_an_odd_position_with_odd_l_seq(c, tables):
    """70 001 bases in one op: the wave's aligned word loads of qualities and packed sequence, at every alignment of the two, on
    either strand, with mapq 0 and 255."""
    rng = np.random.default_rng(11)
    refs = [70100, 9]
    codes = rng.choice(np.array([1, 2, 4, 8, 15, 0], np.uint8), 70001 + 7)
    qual = rng.choice(np.array([0, 12, 13, 40, 61, 93, 255], np.uint8), 70001 + 7)
    for (lead, name), flag, mapq in zip(((0, b""), (3, b"x"), (1, b"xy"), (2, b"xyz"), (5, b"xyzw")), (0, 16, 0, 16, 16), (255, 0, 1, 254, 255)):
        size = 70001
        ops = ([lead << 4 | 4] if lead else []) + [size << 4 | 0]
        one = rec_seq(0, 33, flag, ops, codes[: lead + size], qual[: lead + size].tobytes(), b"long" + name, mapq=mapq)
        recs = [rec_letters(1, 0, "4M", "ACGT"), one, rec_letters(1, 2, "5M", "TTTTT", flag=16, mapq=0)]
        (fwd, rev, n, S), _ = check(c, tables, recs, refs, [])
        mine = rev if flag else fwd
        assert 30000 < int(mine[0].sum()) < 50000 and int(S[0].max()) == mapq * mapq and int(S[1][2]) == 900 and n[1][2] == 2
    over = rec_seq(0, 70000, 16, [40 << 4 | 4, 5000 << 4 | 0], codes[:5040], qual[:5040].tobytes(), b"over")
    (fwd, rev, n, S), _ = check(c, tables, [over, over], refs, [])
    assert not rev[0][:70000].any() and 80 < int(rev[0].sum()) < 200 and not fwd[0].any()


def stream_of(parts):
    """(stream, offsets) of [(record, times)] without a Python object per record."""
    sizes = np.concatenate([np.full(times, len(r), np.uint64) for r, times in parts]) if parts else np.zeros(0, np.uint64)
    return b"".join(r * times for r, times in parts), np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes, dtype=np.uint64)])


def planted(tables_abcd, alt="C", mapqs=(30, 30, 30, 30)):
    """One-base records that give position p of one reference the table tables_abcd[p] of A (reference) and alt, and the cells
    they make, worked out without the walk."""
    length = len(tables_abcd)
    parts = []
    fwd, rev = np.zeros((length, 4), np.int64), np.zeros((length, 4), np.int64)
    n, S = np.zeros(length, np.int64), np.zeros(length, np.int64)
    for p, t in enumerate(tables_abcd):
        for count, letter, flag, mapq in zip(t, ("A", "A", alt, alt), (0, 16, 0, 16), mapqs):
            if count:
                parts.append((rec_letters(0, p, "1M", letter, flag=flag, mapq=mapq, name=b"p"), count))
                (rev if flag else fwd)[p, "ACGT".index(letter)] += count
                n[p] += count
                S[p] += count * mapq * mapq
    return stream_of(parts), ([fwd], [rev], [n], [S])


def call_at(pos, g=(0, 1), R=0, flags=3):
    return (0, pos, R, flags, g[0], g[1]) + (0,) * 18


TABLES = [(1, 1, 1, 1),                                  # x in 0 .. 2, each margin 2
          (0, 1, 1, 0), (1, 0, 0, 1),                    # x in 0 .. 1: the observed table at either end
          (40, 22, 5000, 9000), (3, 60, 900, 70), (10, 3000, 54, 10),          # ranges of 63, 64 and 65 (the smallest margin + 1), lopsided
          (31, 31, 31, 31), (32, 31, 31, 32), (32, 32, 33, 32),                # ... and even
          (3000, 0, 1, 3500), (0, 3000, 3500, 1), (1500, 1500, 1700, 1800),    # several thousand x; the observed at either end and in the middle
          (3, 1, 1, 3), (1, 3, 3, 1), (10, 2, 2, 10), (2, 10, 10, 2),          # exact ties: x and its mirror are equally probable
          (30000, 20000, 10000, 5535), (30000, 20000, 10000, 5536),            # N = 65 535 and 65 536
          (5, 0, 7, 0), (0, 0, 4, 4), (4, 4, 0, 0), (0, 9, 0, 9),              # a zero margin
          (40, 0, 0, 40), (20, 20, 20, 20)]


def test_annotations_of_planted_tables(c, tables):
    LF, E = tables
    (stream, off), cells = planted(TABLES, mapqs=(60, 0, 255, 7))
    c.begin([len(TABLES)])
    c.add(stream, off)
    same_cells(c, cells, [len(TABLES)])
    ranges = [min(a + b, c_ + d, a + c_, b + d) + 1 for a, b, c_, d in TABLES]
    assert {2, 63, 64, 65} <= set(ranges) and max(ranges) > 3000 and int(cells[2][0].max()) == 65536
    called = [call_at(p) for p in range(len(TABLES))]
    notes = B.annotate(called, *cells, LF, E)
    same_notes(c, called, notes)
    by_table = dict(zip(TABLES, notes))
    assert by_table[(30000, 20000, 10000, 5535)][10] == 1 and by_table[(30000, 20000, 10000, 5536)][10] == 3
    assert all(by_table[t][10] == 3 and by_table[t][9] == 0 for t in ((5, 0, 7, 0), (0, 0, 4, 4), (4, 4, 0, 0), (0, 9, 0, 9)))
    assert by_table[(3, 1, 1, 3)][9] == by_table[(1, 3, 3, 1)][9] > 0 and by_table[(10, 2, 2, 10)][9] == by_table[(2, 10, 10, 2)][9] > 500
    assert by_table[(40, 0, 0, 40)][9] == 6000 and by_table[(20, 20, 20, 20)][9] == 0 and by_table[(1, 1, 1, 1)][9] == 0
    assert by_table[(3000, 0, 1, 3500)][9] == 6000
    # MQ: a of mapq 60, b of 0, c of 255, d of 7
    a, b, c_, d = 1500, 1500, 1700, 1800
    assert by_table[(a, b, c_, d)][8] == B.mq(a + b + c_ + d, 3600 * a + 65025 * c_ + 49 * d) > 10000
    # calls that are no variant between the others, the list backwards, a call asked for twice, lists of every size
    mixed = []
    for k, x in enumerate(called):
        mixed += [x] + ([call_at(k, flags=1)] if k % 3 == 0 else []) + ([call_at(k, flags=0, g=(0, 0))] if k % 4 == 0 else [])
    want = B.annotate(mixed, *cells, LF, E)
    assert sum(1 for b in want if b[10] == 0) > 8
    same_notes(c, mixed, want)
    same_notes(c, mixed[::-1], want[::-1])
    many = (mixed * 40)[:1000]
    many_want = (want * 40)[:1000]
    for count in (0, 1, 3, 4, 5, 63, 64, 65, 1000):
        same_notes(c, many[:count], many_want[:count])
    # two alternative letters: c and d are summed over both
    (stream, off), _ = planted([(5, 6, 7, 8)], alt="G")
    c.add(stream, off)                                   # on top of the (1, 1, 1, 1) of A and C at position 0
    got = c.annotate([call_at(0, g=(1, 2))])[0].tolist()
    assert got[:8] == [6, 1, 7, 0, 7, 1, 8, 0] and got[10:] == [1, 30, 6, 7, 8, 9] and got[9] == B.fs(6, 7, 8, 9, LF, E)


def test_counts_beyond_16_bits_on_one_position(c, tables):
    (stream, off), cells = planted([(70000, 1, 2, 66000), (1, 1, 1, 1)], mapqs=(255, 255, 255, 0))
    c.begin([2], min_bq=40)
    c.add(stream, off)
    same_cells(c, cells, [2])
    strand, mapq = c.cells_at(0, 0, 1)
    assert strand[0].tolist() == [70000 << 32 | 1, 2 << 32 | 66000, 0, 0] and int(mapq[0]) == 136003 << 40 | 70003 * 65025
    same_notes(c, [call_at(0), call_at(1)], B.annotate([call_at(0), call_at(1)], *cells, *tables))


def test_cutting_and_order_do_not_matter(c, tables, ref_bases):
    recs = random_records(3001, 21, bases=ref_bases)
    called = calls_for(recs, REF_LENS, ref_bases)
    want = check(c, tables, recs, REF_LENS, called)
    check(c, tables, recs, REF_LENS, called, cuts=[0, 1000, 1002, 3001], want=want)
    check(c, tables, recs, REF_LENS, called, cuts=[0, 0, 1, 64, 65, 1000, 2000, 3001], want=want)
    order = np.random.default_rng(4).permutation(3001)
    check(c, tables, [recs[i] for i in order], REF_LENS, called, cuts=[0, 64, 2000, 3001], want=want)
    check(c, tables, [recs[i] for i in order[::-1]], REF_LENS, called, cuts=[0, 300, 301, 700, 1500, 1501, 2999, 3001], want=want)


def test_skip_bytes_equal_removing_the_records(c, tables, ref_bases):
    recs = random_records(3000, 77, bases=ref_bases)
    called = calls_for(recs, REF_LENS, ref_bases)
    skip = [int(k % 3 == 1) for k in range(3000)]
    want = check(c, tables, recs, REF_LENS, called, skip)
    kept = [r for r, s in zip(recs, skip) if not s]
    assert check(c, tables, kept, REF_LENS, called, want=want) is want
    assert want[1] != B.annotate(called, *B.cells(recs, REF_LENS), *tables)


def test_records_at_both_borders_of_every_reference(c, tables):
    """The last base of a reference and the first of the next lie side by side in both arrays."""
    refs = [100, 1, 7, 300]
    recs, called = [], []
    for r, length in enumerate(refs):
        for p in sorted({0, length - 1}):
            alt = "ACGT"[(r + p + 1) % 4]
            recs += [rec_letters(r, p, "1M", alt, [20 + 7 * r + k], name=b"b%d_%d_%d" % (r, p, k), flag=16 * (k % 2), mapq=10 * r + k) for k in range(1 + r)]
            recs.append(rec_letters(r, p, "3M", "ACG", name=b"o%d_%d" % (r, p), flag=16))        # runs over the end at the last base
            called += [(r, q, (r + q) % 4, 3, min((r + q) % 4, (r + q + 1) % 4), max((r + q) % 4, (r + q + 1) % 4)) + (0,) * 18
                       for q in sorted({0, 1, length - 2, length - 1} & set(range(length)))]
    (fwd, rev, n, S), notes = check(c, tables, recs, refs, called)
    assert [int(x.sum()) for x in n] == [1 + 3 + 1 + 1, 2 + 1, 2 * 3 + 3 + 1, 2 * 4 + 3 + 1] and kinds_of(notes)[2] == 0


def test_strand_cells_add_up_to_bmgs_counts_on_the_device(ref_bases):
    """fwd + rev of the strand cells is bmg's n, and n of the mapq cell their sum, at every position when the thresholds are equal."""
    from bucket_map_amd import bias, genotype
    recs = random_records(3001, 5, bases=ref_bases)
    g, b = genotype.Genotype(0), bias.Bias(0)
    try:
        for th in (dict(min_mapq=0, min_bq=13), dict(min_mapq=20, min_bq=41), dict(min_mapq=0, min_bq=0)):
            stream, off = b"".join(recs), offsets_of(recs)
            g.begin(REF_LENS, **th)
            g.add(stream, off)
            b.begin(REF_LENS, **th)
            b.add(stream, off)
            total = 0
            for r, length in enumerate(REF_LENS):
                cells, (strand, mapq) = g.cells_at(r, 0, length), b.cells_at(r, 0, length)
                both = (strand >> np.uint64(32)) + (strand & np.uint64(0xFFFFFFFF))
                assert np.array_equal(both, cells >> np.uint64(32)), (th, r)
                assert np.array_equal(mapq >> np.uint64(40), both.sum(axis=1)), (th, r)
                total += int(both.sum())
            assert total > 20000
    finally:
        g.close()
        b.close()


def test_small_after_large_and_refusals_between(c, tables):
    from bucket_map_amd import bias
    big = [3000000, 70000, 5]
    big_bases = references(big, 9)
    big_recs = random_records(5001, 31, big, big_bases)
    big_called = calls_for(big_recs, big, big_bases)
    check(c, tables, big_recs, big, big_called)
    small, bases = edge_records(), edge_bases()
    small_called = calls_for(small, EDGE_REFS, bases)
    check(c, tables, small, EDGE_REFS, small_called, **STRICT)   # nothing stale: smaller references, fewer records and calls, other parameters
    check(c, tables, big_recs[::-1], big, big_called[::-1])     # and larger again
    good = random_records(300, 8, EDGE_REFS, bases)
    called = calls_for(good, EDGE_REFS, bases)
    first = B.cells(good[:100], EDGE_REFS)
    c.begin(EDGE_REFS)
    c.add(b"".join(good[:100]), offsets_of(good[:100]))
    same_notes(c, called, B.annotate(called, *first, *tables))   # an annotation in the middle does not end the counting
    bad_off = offsets_of(good)
    bad_off[5] += 1
    refusals = [(b"".join(good), bad_off), ([rec_ops(0, 0, 0, [3 << 4 | 9], b"")], None), ([rec(0, 5, 0, "3M", b"ab")], None),
                ([rec(3, 5, 0, "3M", b"")], None)]
    for stream, off in refusals:                         # a refused add leaves what was added before
        if off is None:
            stream, off = b"".join(stream), offsets_of(stream)
        with pytest.raises(bias.BmbError) as e:
            c.add(stream, off)
        assert e.value.code == bias.BMB_ERR_ARG
    variant = lambda ref, pos, R=0, g=(0, 1): (ref, pos, R, 3, g[0], g[1]) + (0,) * 18
    for call in (lambda: c.annotate([variant(3, 0)]), lambda: c.annotate(called + [variant(1, 50)]), lambda: c.annotate([variant(2, 1)] + called),
                 lambda: c.annotate([variant(0, 0, R=4)]), lambda: c.annotate([variant(0, 0, g=(0, 4))]),
                 lambda: c.cells_at(3, 0, 1), lambda: c.cells_at(1, 45, 6), lambda: c.cells_at(2, 1, 1)):
        with pytest.raises(bias.BmbError) as e:
            call()
        assert e.value.code == bias.BMB_ERR_ARG
    assert c.annotate([(3, 0, 9, 1, 7, 7) + (0,) * 18]).tolist() == [[0] * 16]     # a call that is no variant is not looked at
    for lens in ([], [4, 0], [2 ** 32 - 2 ** 20, 1]):
        a, t = np.asarray(lens, np.uint32), np.array([0, 13], np.uint32)
        rc = bias.lib().bmb_begin(c._h, a.ctypes.data_as(bias._u32p), len(lens), t.ctypes.data_as(bias._u32p))
        assert rc == bias.BMB_ERR_ARG, lens
    same_cells(c, first, EDGE_REFS)                       # the state is intact
    c.add(b"".join(good[100:]), offsets_of(good[100:]))  # ... and an add after an annotation keeps counting
    cells = B.cells(good, EDGE_REFS)
    same_cells(c, cells, EDGE_REFS)
    notes = B.annotate(called, *cells, *tables)
    same_notes(c, called, notes)
    same_notes(c, called[::2], notes[::2])
    same_notes(c, [], [])
    same_notes(c, called, notes)
    check(c, tables, small, EDGE_REFS, small_called)


def test_large_after_small_on_a_fresh_context(tables):
    from bucket_map_amd import bias
    fresh = bias.Bias(0)
    try:
        for call in (lambda: fresh.add(b"", [0]), lambda: fresh.annotate([call_at(0)]), lambda: fresh.annotate([]), lambda: fresh.cells_at(0, 0, 1)):
            with pytest.raises(bias.BmbError) as e:
                call()
            assert e.value.code == bias.BMB_ERR_ARG and "no bmb_begin" in str(e.value)
        fresh.begin([7])
        fresh.add(b"", [0])                              # no record: succeeds
        assert not fresh.cells_at(0, 0, 7)[0].any() and not fresh.cells_at(0, 0, 7)[1].any() and fresh.annotate([]).shape == (0, 16)
        assert fresh.annotate([call_at(6)]).tolist() == [[0] * 10 + [3] + [0] * 5]    # a variant call on nothing: no FS, MQ 0
        recs, bases = edge_records(), edge_bases()
        check(fresh, tables, recs, EDGE_REFS, calls_for(recs, EDGE_REFS, bases))
        big = [5, 3000000, 70000]
        bases = references(big, 10)
        recs = random_records(5001, 33, big, bases)
        check(fresh, tables, recs, big, calls_for(recs, big, bases))
    finally:
        fresh.close()


# ---- the tools ----
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_pileup import pileup_jobs
    return pileup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_gpu_tool_writes_the_oracle_tools_files(jobs, k):
    name, which, d, args, extra = jobs[k]
    loose = ["--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--pileup-min-bq", "0"]
    for tag, opts, env in ((name, [], None), (name + "r", [*loose, "--vcf-max-fs", "2", "--vcf-min-mq", "40", "--vcf-indels"], dict(BM_SORT_RUN_BYTES="2000"))):
        files = ["--vcf", f"{tag}.go.vcf", "--gvcf", f"{tag}.go.g.vcf", "--vcf-bias"]
        err = run(TOOLS[(which, "oracle")], d, args, f"{tag}.go.bam", [*extra, *opts, *files], env=env)
        want, want_g, told = (d / f"{tag}.go.vcf").read_text(), (d / f"{tag}.go.g.vcf").read_text(), bias_line(err)
        assert name == "plain" or (len(variant_lines(want)) > 3 and "ADF:ADR" in want)
        files = ["--vcf", f"{tag}.g.vcf", "--gvcf", f"{tag}.g.g.vcf", "--vcf-bias"]
        err = run(TOOLS[(which, "gpu")], d, args, f"{tag}.g.bam", [*extra, *opts, *files], env=env)
        assert ("in 1 run(s)" in err) == (env is None) and bias_line(err) == told
        assert (d / f"{tag}.g.vcf").read_text() == want and (d / f"{tag}.g.g.vcf").read_text() == want_g and pair_of(d, f"{tag}.g") == pair_of(d, f"{tag}.go")
        err = run(TOOLS[(which, "gpu")], d, args, f"{tag}.gg.bam", [*extra, *opts, "--gvcf", f"{tag}.gg.g.vcf", "--vcf-bias"], env=env)   # --gvcf alone
        assert (d / f"{tag}.gg.g.vcf").read_text() == want_g and bias_line(err) == told


def test_gpu_tool_flags_a_snv_on_one_strand_only(tmp_path):
    args, extra = planted_pairs(tmp_path)
    opts = [*extra, "--vcf-bias", "--vcf-max-fs", "30"]
    err = run(TOOLS[("bucketmap_align", "oracle")], tmp_path, args, "o.bam", [*opts, "--vcf", "o.vcf", "--gvcf", "o.g.vcf"])
    told = bias_line(err)
    err = run(TOOLS[("bucketmap_align", "gpu")], tmp_path, args, "g.bam", [*opts, "--vcf", "g.vcf", "--gvcf", "g.g.vcf"])
    assert bias_line(err) == told == "Bias: 2 variants annotated (1 StrandBias, 0 LowMQ, 0 without FS)"
    assert (tmp_path / "g.vcf").read_text() == (tmp_path / "o.vcf").read_text() and (tmp_path / "g.g.vcf").read_text() == (tmp_path / "o.g.vcf").read_text()
    check_planted_lines((tmp_path / "g.vcf").read_text())
    assert variant_lines((tmp_path / "g.g.vcf").read_text()) == variant_lines((tmp_path / "g.vcf").read_text())
