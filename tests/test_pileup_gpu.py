"""bmp_begin / bmp_add / bmp_finish / bmp_sites / bmp_counts_at on the MI355X against the rule in plain Python
(tests/pileup_rule.py) -- all eight counters at every position, the site list and the six sums per reference, all exactly --,
and the product tools' --pileup file and stderr line against the oracle-backed tools' (whose counting is host/pileup.h): the
rule is exact, so the files are equal.  Every tool run has its own time limit; nothing is retried."""
import numpy as np
import pytest

import pileup_rule as P
from pileup_cases import EDGE_REFS, REF_LENS, SIZES, edge_bases, edge_records, many_ops_record, random_records, rec_letters, rec_seq, references
from test_bamsort import offsets_of, pair_of
from test_markdup_gpu import rec, rec_ops, run
from test_sam_golden import TOOLS

pytestmark = pytest.mark.gpu

STRICT = dict(min_mapq=20, min_bq=13, min_alt=1, min_frac_ppm=250000)
TILE = 2048                                              # positions per workgroup of the site passes


@pytest.fixture(scope="module")
def c():
    from bucket_map_amd import pileup
    ctx = pileup.Pileup(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ref_bases():
    return references()


def same(c, want, ref_len):
    """What the context holds after finish() is the rule's: the stats, the sites, and every counter of every position."""
    n_sites, stats = c.last
    assert stats.tolist() == want.stats
    for r, length in enumerate(ref_len):
        got = c.counts_at(r, 0, length)
        assert np.array_equal(got, want.counts[r]), (r, np.flatnonzero((got != want.counts[r]).any(axis=1))[:10])
        lo, n = length // 3, min(length - length // 3, 5000)
        assert np.array_equal(c.counts_at(r, lo, n), want.counts[r][lo: lo + n]) and c.counts_at(r, length, 0).shape == (0, 8)
    assert n_sites == len(want.sites)
    assert [tuple(s) for s in c.sites().tolist()] == want.sites
    if n_sites > 2:
        assert [tuple(s) for s in c.sites(1, n_sites - 2).tolist()] == want.sites[1:-1] and c.sites(n_sites, 0).shape == (0, 12)


def check(c, recs, ref_len, bases, skip=None, cuts=None, want=None, **th):
    """The device's result for the records (added in the stretches cuts names) is the rule's; returns the rule's."""
    want = P.pile(recs, ref_len, bases, skip, **th) if want is None else want
    cuts = [0, len(recs)] if cuts is None else cuts
    c.begin(ref_len, bases, **th)
    for a, b in zip(cuts, cuts[1:]):
        c.add(b"".join(recs[a:b]), offsets_of(recs[a:b]), None if skip is None else skip[a:b])
    c.last = c.finish()
    same(c, want, ref_len)
    return want


def kinds_of(want):
    return [sum(1 for s in want.sites if s[11] & b) for b in (1, 2, 4)]


@pytest.mark.parametrize("n", SIZES)
def test_sizes(c, ref_bases, n):
    recs = random_records(n, 300 + n, bases=ref_bases)
    want = check(c, recs, REF_LENS, ref_bases)
    if n >= 257:                                         # neither no site nor every position
        assert all(kinds_of(want)) and len(want.sites) < sum(REF_LENS) // 10 and all(s[0] for s in want.stats[1:])
    if n:
        assert c.ms_add > 0 and c.ms_finish > 0


def test_edge_list(c):
    recs, bases = edge_records(), edge_bases()
    assert {len(r) % 16 for r in recs} == set(range(16))
    for th in ({}, STRICT, dict(min_frac_ppm=0, min_alt=1), dict(min_frac_ppm=1000000, min_bq=0), dict(min_bq=256, min_mapq=31)):
        want = check(c, recs, EDGE_REFS, bases, **th)
    assert want.stats[0][1] > 40 and want.stats[0][0] == 0                        # every MAPQ 30 record is below 31
    want = check(c, recs, EDGE_REFS, bases, **STRICT)
    assert all(kinds_of(want)) and want.stats[1][2] == 1
    for size in (1, 7, 40):                              # the same records as the first and the last of a stream
        check(c, recs[:size], EDGE_REFS, bases, **STRICT)
        check(c, recs[-size:], EDGE_REFS, bases, **STRICT)
    for r in recs[:33] + recs[-35:]:                     # and each alone
        check(c, [r], EDGE_REFS, bases, **STRICT)


def test_a_record_of_many_ops_beside_short_ones(c):
    """60 000 ops: 938 trips of the wave walk, the cursors and the anchor flag carried from each to the next."""
    refs = [90000, 300]
    bases = references(refs, 4)
    recs = random_records(150, 5, refs, bases) + [many_ops_record(0, 17)] + random_records(150, 6, refs, bases) + [many_ops_record(0, 60001, seed=8)]
    want = check(c, recs, refs, bases)
    assert want.stats[0][3] > 60000 and int(want.counts[0][:, 5].sum()) > 5000 and int(want.counts[0][:, 6].sum()) > 3000
    check(c, [many_ops_record(0, 17)], refs, bases, min_alt=1, min_frac_ppm=0)


def test_one_long_block_at_an_odd_position_with_odd_l_seq(c):
    """70 001 bases in one op: the wave's aligned word loads of qualities and packed sequence, at every alignment of the two."""
    rng = np.random.default_rng(11)
    refs = [70100, 9]
    bases = references(refs, 5)
    codes = rng.choice(np.array([1, 2, 4, 8, 15, 0], np.uint8), 70001 + 7)
    qual = rng.choice(np.array([0, 12, 13, 40, 255], np.uint8), 70001 + 7)
    for lead, name in ((0, b""), (3, b"x"), (1, b"xy"), (2, b"xyz"), (5, b"xyzw")):   # odd and even query offsets, record alignments 0 .. 3
        n = 70001
        ops = ([lead << 4 | 4] if lead else []) + [n << 4 | 0]
        one = rec_seq(0, 33, 0, ops, codes[: lead + n], qual[: lead + n].tobytes(), b"long" + name)
        want = check(c, [rec_letters(1, 0, "4M", "ACGT"), one, rec_letters(1, 2, "5M", "TTTTT")], refs, bases, min_alt=1)
        assert want.stats[0][3] + want.stats[0][4] == 70001 and want.stats[0][4] > 20000 and len(want.sites) > 1000
    # a long block that runs over the end of the reference, and a long deletion shared by the wave
    over = rec_seq(0, 70000, 0, [40 << 4 | 4, 5000 << 4 | 0], codes[:5040], qual[:5040].tobytes(), b"over")
    gap = rec_seq(0, 100, 0, [3 << 4 | 0, 60000 << 4 | 2, 3 << 4 | 0], codes[:6], bytes([40] * 6), b"gap")
    want = check(c, [over, gap, gap], refs, bases)
    assert want.stats[0][3] + want.stats[0][4] == 100 + 12 and int(want.counts[0][:, 5].sum()) == 120000


def test_counts_beyond_16_bits(c):
    recs = [rec_seq(1, 5, 0, [1 << 4], [(1, 2, 4, 8)[k % 4]], bytes([40]), b"d%d" % k) for k in range(70000)]
    recs += [rec_letters(1, 3, "4M", "ACGT"), rec_letters(0, 0, "9M", "ACGTACGTA")]
    want = check(c, recs, [9, 10], [b"ACGTACGTA", b"ACGTACGTAC"], min_alt=17501, min_frac_ppm=250000)
    assert want.counts[1][5].tolist() == [17500, 17500, 17501, 17500, 0, 0, 0, 0] and [s[:2] for s in want.sites] == [(1, 5)]
    assert want.stats[1] == [70001, 0, 0, 70004, 0, 1]


def site_read(ref, p, ref_letter, name):
    return rec_letters(ref, p, "1M", "ACGTA"["ACGT".index(ref_letter) + 1], name=name)


def test_sites_against_tiles_and_reference_borders(c):
    """Sites at the last slot of a tile and the first of the next, a tile where every position is a site and one with none,
    sites on the last base of a reference and the first of the next -- the references lie back to back in the state, so the
    second reference starts in the middle of a tile."""
    refs = [3 * TILE + 100, 5, 2 * TILE]
    bases = [bytes(b"ACGT"[p % 4] for p in range(n)) for n in refs]
    letter = lambda p: "ACGT"[p % 4]
    spots = [(0, TILE - 1), (0, TILE), (0, 2 * TILE - 1), (0, refs[0] - 1), (1, 0), (1, 4), (2, 0), (2, refs[2] - 1), (2, TILE - 105 - 1), (2, TILE - 105)]
    recs = [site_read(r, p, letter(p), b"s%d_%d_%d" % (r, p, k)) for r, p in spots for k in range(2)]
    want = check(c, recs, refs, bases)
    assert [s[:2] for s in want.sites] == sorted(spots) and [s[5] for s in want.stats] == [4, 2, 4]
    # every position of the second tile of reference 0 a site (one read of 2 048 wrong bases, twice), none in the first and third
    wrong = "".join("ACGTA"["ACGT".index(letter(p)) + 1] for p in range(TILE, 2 * TILE))
    full = [rec_letters(0, TILE, "%dM" % TILE, wrong, name=b"full%d" % k) for k in range(2)]
    want = check(c, full, refs, bases)
    assert [s[:2] for s in want.sites] == [(0, p) for p in range(TILE, 2 * TILE)] and want.stats[0][5] == TILE
    want = check(c, full + recs, refs, bases)
    assert len(want.sites) == TILE + len(spots) - 2


def test_thresholds_that_make_every_covered_position_a_site_and_none(c, ref_bases):
    recs = random_records(1025, 55, bases=ref_bases)
    every = check(c, recs, REF_LENS, ref_bases, min_bq=0, min_alt=1, min_frac_ppm=0)
    assert len(every.sites) > 500
    none = check(c, recs, REF_LENS, ref_bases, min_alt=2 ** 32 - 1)
    assert none.sites == [] and [s[5] for s in none.stats] == [0] * len(REF_LENS) and none.stats[5][3] == every.stats[5][3] + every.stats[5][4] - none.stats[5][4]
    # a reference of the wrong letters throughout: every covered position with a reference allele is a site
    flipped = [bytes(b"ACGTA"[b"ACGT".index(x) + 1] if x in b"ACGT" else x for x in b.upper()) for b in ref_bases]
    want = check(c, recs, REF_LENS, flipped, min_alt=1, min_frac_ppm=0)
    covered = sum(int((cnt[:, :4].sum(axis=1) > 0).sum()) for cnt in want.counts)
    assert len(want.sites) > 0.8 * covered
    low = check(c, recs, REF_LENS, ref_bases, min_mapq=256)
    assert low.sites == [] and sum(s[0] for s in low.stats) == 0 and sum(s[1] for s in low.stats) > 500 and not any(cnt.any() for cnt in low.counts)


def test_cutting_and_order_do_not_matter(c, ref_bases):
    recs = random_records(3001, 21, bases=ref_bases)
    want = check(c, recs, REF_LENS, ref_bases)
    check(c, recs, REF_LENS, ref_bases, cuts=[0, 1000, 1002, 3001], want=want)
    check(c, recs, REF_LENS, ref_bases, cuts=[0, 0, 1, 64, 65, 1000, 2000, 3001], want=want)
    order = np.random.default_rng(4).permutation(3001)
    check(c, [recs[i] for i in order], REF_LENS, ref_bases, cuts=[0, 64, 2000, 3001], want=want)
    check(c, [recs[i] for i in order[::-1]], REF_LENS, ref_bases, cuts=[0, 300, 301, 700, 1500, 1501, 2999, 3001], want=want)


def test_skip_bytes_equal_removing_the_records(c, ref_bases):
    recs = random_records(3000, 77, bases=ref_bases)
    skip = [int(k % 3 == 1) for k in range(3000)]
    want = check(c, recs, REF_LENS, ref_bases, skip)
    kept = [r for r, s in zip(recs, skip) if not s]
    assert check(c, kept, REF_LENS, ref_bases, want=want) is want
    assert want.stats != P.pile(recs, REF_LENS, ref_bases).stats


def test_small_after_large_and_refusals_between(c):
    from bucket_map_amd import pileup
    big = [3000000, 70000, 5]
    big_bases = references(big, 9)
    check(c, random_records(5001, 31, big, big_bases), big, big_bases)
    small, bases = edge_records(), edge_bases()
    check(c, small, EDGE_REFS, bases, **STRICT)           # nothing stale: smaller references, fewer records, other thresholds
    check(c, random_records(5001, 32, big, big_bases), big, big_bases)   # and larger again
    good = random_records(300, 8, EDGE_REFS, bases)
    want = P.pile(good, EDGE_REFS, bases)
    c.begin(EDGE_REFS, bases)
    c.add(b"".join(good[:100]), offsets_of(good[:100]))
    bad_off = offsets_of(good)
    bad_off[5] += 1
    refusals = [(b"".join(good), bad_off), ([rec_ops(0, 0, 0, [3 << 4 | 9], b"")], None), ([rec(0, 5, 0, "3M", b"ab")], None),
                ([rec(3, 5, 0, "3M", b"")], None)]
    for stream, off in refusals:                         # a refused add leaves what was added before
        if off is None:
            stream, off = b"".join(stream), offsets_of(stream)
        with pytest.raises(pileup.BmpError) as e:
            c.add(stream, off)
        assert e.value.code == pileup.BMP_ERR_ARG
    for call in (lambda: c.sites(0, 0), lambda: c.counts_at(0, 0, 1)):
        with pytest.raises(pileup.BmpError) as e:
            call()
        assert e.value.code == pileup.BMP_ERR_ARG and "no bmp_finish" in str(e.value)
    c.add(b"".join(good[100:]), offsets_of(good[100:]))
    c.last = c.finish()
    same(c, want, EDGE_REFS)
    n_sites = c.last[0]
    for call in (c.finish, lambda: c.add(b"".join(good), offsets_of(good)), lambda: c.sites(n_sites, 1), lambda: c.sites(0, n_sites + 1),
                 lambda: c.counts_at(3, 0, 1), lambda: c.counts_at(1, 45, 6), lambda: c.counts_at(2, 1, 1)):
        with pytest.raises(pileup.BmpError) as e:
            call()
        assert e.value.code == pileup.BMP_ERR_ARG
    same(c, want, EDGE_REFS)                              # the result is still there
    for lens, some, th in (([], [], {}), ([4, 0], [b"ACGT", b""], {}), ([2 ** 32 - 2 ** 20, 1], [b"", b"A"], {}), ([4], [b"ACGT"], dict(min_alt=0)),
                           ([4], [b"ACGT"], dict(min_frac_ppm=1000001))):
        keep, ptrs = pileup.base_pointers([b if b else b"A" for b in some])
        a, t = np.asarray(lens, np.uint32), np.array([{**pileup.DEFAULTS, **th}[k] for k in pileup.THRESHOLDS], np.uint32)
        rc = pileup.lib().bmp_begin(c._h, a.ctypes.data_as(pileup._u32p), len(lens), ptrs, t.ctypes.data_as(pileup._u32p))
        assert rc == pileup.BMP_ERR_ARG, lens
    same(c, want, EDGE_REFS)
    check(c, small, EDGE_REFS, bases)


def test_large_after_small_on_a_fresh_context():
    from bucket_map_amd import pileup
    fresh = pileup.Pileup(0)
    try:
        with pytest.raises(pileup.BmpError) as e:
            fresh.add(b"", [0])
        assert e.value.code == pileup.BMP_ERR_ARG and "no bmp_begin" in str(e.value)
        with pytest.raises(pileup.BmpError) as e:
            fresh.finish()
        assert e.value.code == pileup.BMP_ERR_ARG
        fresh.begin([7], [b"ACGTACG"])
        fresh.add(b"", [0])                              # no record: succeeds
        n_sites, stats = fresh.finish()
        assert n_sites == 0 and stats.tolist() == [[0] * 6] and fresh.sites().shape == (0, 12) and not fresh.counts_at(0, 0, 7).any()
        check(fresh, edge_records(), EDGE_REFS, edge_bases())
        big = [5, 3000000, 70000]
        bases = references(big, 10)
        check(fresh, random_records(5001, 33, big, bases), big, bases)
    finally:
        fresh.close()


# ---- the tools ----
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_pileup import pileup_jobs
    return pileup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_gpu_tool_writes_the_oracle_tools_file(jobs, k):
    from test_pileup import HEADER, pileup_line
    name, which, d, args, extra = jobs[k]
    loose = ["--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--pileup-min-bq", "0"]
    # the defaults in one run and in several; then looser thresholds, duplicates left out, --depth beside it
    for tag, opts, env in ((name, [], None), (name + "r", [], dict(BM_SORT_RUN_BYTES="2000")),
                           (name + "m", ["--markdup", *loose, "--depth", f"{name}m.g.bedgraph"], None)):
        err = run(TOOLS[(which, "oracle")], d, args, f"{tag}.go.bam", [*extra, *opts, "--pileup", f"{tag}.go.tsv"], env=env)
        want, told = (d / f"{tag}.go.tsv").read_text(), pileup_line(err)
        assert want.startswith(HEADER) and (name == "plain" or want.count("\n") > 4)
        err = run(TOOLS[(which, "gpu")], d, args, f"{tag}.g.bam", [*extra, *opts, "--pileup", f"{tag}.g.tsv"], env=env)
        assert ("in 1 run(s)" in err) == (env is None) and pileup_line(err) == told
        assert (d / f"{tag}.g.tsv").read_text() == want and pair_of(d, f"{tag}.g") == pair_of(d, f"{tag}.go")
    assert (d / f"{name}.g.tsv").read_text() == (d / f"{name}r.g.tsv").read_text()
    assert name == "plain" or (d / f"{name}.g.tsv").read_text() != (d / f"{name}m.g.tsv").read_text()
