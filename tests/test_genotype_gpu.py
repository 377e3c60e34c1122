"""bmg_begin / bmg_add / bmg_call / bmg_cells_at on the MI355X against the rule in plain Python (tests/genotype_rule.py) -- all
four cells at every position and all 24 words of every call, exactly --, bmg's counts against bmp's on the device, and the
product tools' --vcf file and stderr line against the oracle-backed tools' (whose calling is host/genotype.h): the rule is
exact, so the files are equal.  Every tool run has its own time limit; nothing is retried."""
import numpy as np
import pytest

import genotype_rule as G
import pileup_rule as P
from pileup_cases import EDGE_REFS, REF_LENS, edge_bases, edge_records, many_ops_record, random_records, rec_letters, rec_seq, references
from test_bamsort import offsets_of, pair_of
from test_genotype import PARAM_SETS, genotypes_line, site, sites_for
from test_markdup_gpu import rec, rec_ops, run
from test_sam_golden import TOOLS

pytestmark = pytest.mark.gpu

STRICT = dict(min_mapq=20, min_bq=13, q_cap=40, q_absent=7, prior=1234)


@pytest.fixture(scope="module")
def c():
    from bucket_map_amd import genotype
    ctx = genotype.Genotype(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ref_bases():
    return references()


def flipped(bases):
    """The references with the wrong letter throughout: every covered position with a reference allele becomes an SNV site."""
    return [bytes(b"ACGTA"[b"ACGT".index(x) + 1] if x in b"ACGT" else x for x in b.upper()) for b in bases]


def same_cells(c, n, Q, ref_len):
    for r, length in enumerate(ref_len):
        got, want = c.cells_at(r, 0, length), G.packed(n[r], Q[r])
        assert np.array_equal(got, want), (r, np.flatnonzero((got != want).any(axis=1))[:10])
        lo, count = length // 3, min(length - length // 3, 5000)
        assert np.array_equal(c.cells_at(r, lo, count), want[lo: lo + count]) and c.cells_at(r, length, 0).shape == (0, 4)


def same_calls(c, sites, called):
    got = c.call(np.asarray(sites, np.uint32).reshape(-1, 12))
    assert got.shape == (len(sites), 24)
    if got.tolist() != [list(x) for x in called]:
        bad = [i for i, (a, b) in enumerate(zip(got.tolist(), called)) if tuple(a) != b][:3]
        assert False, [(i, got[i].tolist(), called[i]) for i in bad]


def check(c, recs, ref_len, sites, skip=None, cuts=None, want=None, **params):
    """The device's cells and calls for the records (added in the stretches cuts names) are the rule's; returns the rule's."""
    want = G.genotype(recs, ref_len, sites, skip, **params) if want is None else want
    cuts = [0, len(recs)] if cuts is None else cuts
    c.begin(ref_len, **params)
    for a, b in zip(cuts, cuts[1:]):
        c.add(b"".join(recs[a:b]), offsets_of(recs[a:b]), None if skip is None else skip[a:b])
    same_cells(c, want[0], want[1], ref_len)
    same_calls(c, sites, want[2])
    return want


def kinds_of(called):
    """(variant, genotyped but the reference's, not genotyped)"""
    return sum(1 for x in called if x[3] & 2), sum(1 for x in called if x[3] == 1), sum(1 for x in called if x[3] == 0)


@pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 257, 3001])
def test_sizes(c, ref_bases, size):
    recs = random_records(size, 300 + size, bases=ref_bases)
    sites = sites_for(recs, REF_LENS, ref_bases) if size > 1 else [site(0, 0, 0), site(5, REF_LENS[5] - 1, 2)]
    n, Q, called = check(c, recs, REF_LENS, sites)
    if size >= 257:
        assert all(k > 5 for k in kinds_of(called)) and any(x[4] != x[5] for x in called) and any(x[3] & 2 and x[4] == x[5] for x in called)
    if size:
        assert c.ms_add > 0 and c.ms_call > 0


def test_edge_list(c):
    recs, bases = edge_records(), edge_bases()
    assert {len(r) % 16 for r in recs} == set(range(16))
    sites = sites_for(recs, EDGE_REFS, bases, min_bq=0) + [site(r, p, p % 4) for r, length in enumerate(EDGE_REFS) for p in (0, length - 1)]
    for pr in (*PARAM_SETS, STRICT):
        n, Q, called = check(c, recs, EDGE_REFS, sites, **pr)
    assert all(kinds_of(called))
    for size in (1, 7, 40):                              # the same records as the first and the last of a stream
        check(c, recs[:size], EDGE_REFS, sites, **STRICT)
        check(c, recs[-size:], EDGE_REFS, sites, **STRICT)
    for r in recs[:33] + recs[-35:]:                     # and each alone
        check(c, [r], EDGE_REFS, sites, **STRICT)


def test_a_record_of_many_ops_beside_short_ones(c):
    """60 001 ops: 938 trips of the wave walk with the cursors carried from each to the next; here without the anchor flag."""
    refs = [90000, 300]
    bases = references(refs, 4)
    recs = random_records(150, 5, refs, bases) + [many_ops_record(0, 17)] + random_records(150, 6, refs, bases) + [many_ops_record(0, 60001, seed=8)]
    sites = sites_for(recs, refs, bases)
    n, Q, called = check(c, recs, refs, sites)
    assert int(n[0].sum()) > 60000 and kinds_of(called)[0] > 1000
    check(c, [many_ops_record(0, 17)], refs, sites, prior=0)


def test_one_long_block_at_an_odd_position_with_odd_l_seq(c):
    """70 001 bases in one op: the wave's aligned word loads of qualities and packed sequence, at every alignment of the two,
    with qualities that are capped, absent, below and at min_bq."""
    rng = np.random.default_rng(11)
    refs = [70100, 9]
    bases = references(refs, 5)
    codes = rng.choice(np.array([1, 2, 4, 8, 15, 0], np.uint8), 70001 + 7)
    qual = rng.choice(np.array([0, 12, 13, 40, 61, 93, 255], np.uint8), 70001 + 7)
    for lead, name in ((0, b""), (3, b"x"), (1, b"xy"), (2, b"xyz"), (5, b"xyzw")):   # odd and even query offsets, record alignments 0 .. 3
        size = 70001
        ops = ([lead << 4 | 4] if lead else []) + [size << 4 | 0]
        one = rec_seq(0, 33, 0, ops, codes[: lead + size], qual[: lead + size].tobytes(), b"long" + name)
        recs = [rec_letters(1, 0, "4M", "ACGT"), one, rec_letters(1, 2, "5M", "TTTTT")]
        sites = P.pile(recs, refs, bases, min_alt=1).sites[::3] + [site(0, p, p % 4) for p in (0, 32, 33, 34, 70033, 70034, 70099)]
        n, Q, called = check(c, recs, refs, sites)
        assert 30000 < int(n[0].sum()) < 50000 and int(Q[0].max()) == 60 and {30, 13, 40} <= set(np.unique(Q[0]).tolist()) and kinds_of(called)[0] > 1000
    # a long block that runs over the end of the reference
    over = rec_seq(0, 70000, 0, [40 << 4 | 4, 5000 << 4 | 0], codes[:5040], qual[:5040].tobytes(), b"over")
    n, Q, called = check(c, [over, over], refs, [site(0, p, 0) for p in range(69990, 70100)])
    assert not n[0][:70000].any() and 80 < int(n[0].sum()) < 200 and kinds_of(called)[0] > 10


def test_counts_and_quality_sums_beyond_16_bits(c):
    recs = [rec_seq(1, 5, 0, [1 << 4], [2 if k % 16 else 4], bytes([40 if k % 3 else 255]), b"d%d" % k) for k in range(70000)]
    recs += [rec_letters(1, 3, "4M", "ACGT"), rec_letters(0, 0, "9M", "ACGTACGTA")]
    sites = [site(1, 5, 0), site(1, 5, 1), site(1, 5, 2), site(1, 4, 1), site(0, 8, 0)]
    n, Q, called = check(c, recs, [9, 10], sites)
    assert n[1][5].tolist() == [0, 65625, 4375 + 1, 0] and Q[1][5][1] > 2 ** 21 and called[0][22] == 70001      # 65 625 > 2^16 in one cell
    assert called[0][7] > 2 ** 27 and called[1][3] == 1 and called[1][7] == 0 and called[4][22] == 1


def test_cutting_and_order_do_not_matter(c, ref_bases):
    recs = random_records(3001, 21, bases=ref_bases)
    sites = sites_for(recs, REF_LENS, ref_bases)
    want = check(c, recs, REF_LENS, sites)
    check(c, recs, REF_LENS, sites, cuts=[0, 1000, 1002, 3001], want=want)
    check(c, recs, REF_LENS, sites, cuts=[0, 0, 1, 64, 65, 1000, 2000, 3001], want=want)
    order = np.random.default_rng(4).permutation(3001)
    check(c, [recs[i] for i in order], REF_LENS, sites, cuts=[0, 64, 2000, 3001], want=want)
    check(c, [recs[i] for i in order[::-1]], REF_LENS, sites, cuts=[0, 300, 301, 700, 1500, 1501, 2999, 3001], want=want)


def test_skip_bytes_equal_removing_the_records(c, ref_bases):
    recs = random_records(3000, 77, bases=ref_bases)
    sites = sites_for(recs, REF_LENS, ref_bases)
    skip = [int(k % 3 == 1) for k in range(3000)]
    want = check(c, recs, REF_LENS, sites, skip)
    kept = [r for r, s in zip(recs, skip) if not s]
    assert check(c, kept, REF_LENS, sites, want=want) is want
    assert want[2] != G.genotype(recs, REF_LENS, sites)[2]


def test_small_after_large_and_refusals_between(c):
    from bucket_map_amd import genotype
    big = [3000000, 70000, 5]
    big_bases = references(big, 9)
    big_recs = random_records(5001, 31, big, big_bases)
    big_sites = sites_for(big_recs, big, big_bases)
    check(c, big_recs, big, big_sites)
    small, bases = edge_records(), edge_bases()
    small_sites = sites_for(small, EDGE_REFS, bases, min_bq=0)
    check(c, small, EDGE_REFS, small_sites, **STRICT)     # nothing stale: smaller references, fewer records and sites, other parameters
    check(c, big_recs[::-1], big, big_sites[::-1])        # and larger again
    good = random_records(300, 8, EDGE_REFS, bases)
    sites = sites_for(good, EDGE_REFS, bases)
    n, Q, called = G.genotype(good, EDGE_REFS, sites)
    first = G.genotype(good[:100], EDGE_REFS, sites)
    c.begin(EDGE_REFS)
    c.add(b"".join(good[:100]), offsets_of(good[:100]))
    same_calls(c, sites, first[2])                        # a call in the middle does not end the counting
    bad_off = offsets_of(good)
    bad_off[5] += 1
    refusals = [(b"".join(good), bad_off), ([rec_ops(0, 0, 0, [3 << 4 | 9], b"")], None), ([rec(0, 5, 0, "3M", b"ab")], None),
                ([rec(3, 5, 0, "3M", b"")], None)]
    for stream, off in refusals:                         # a refused add leaves what was added before
        if off is None:
            stream, off = b"".join(stream), offsets_of(stream)
        with pytest.raises(genotype.BmgError) as e:
            c.add(stream, off)
        assert e.value.code == genotype.BMG_ERR_ARG
    for call in (lambda: c.call([site(3, 0, 0)]), lambda: c.call(sites + [site(1, 50, 0)]), lambda: c.call([site(2, 1, 0)] + sites),
                 lambda: c.cells_at(3, 0, 1), lambda: c.cells_at(1, 45, 6), lambda: c.cells_at(2, 1, 1)):
        with pytest.raises(genotype.BmgError) as e:
            call()
        assert e.value.code == genotype.BMG_ERR_ARG
    for lens, pr in (([], {}), ([4, 0], {}), ([2 ** 32 - 2 ** 20, 1], {}), ([4], dict(q_cap=0)), ([4], dict(q_cap=94)), ([4], dict(q_absent=61))):
        a, t = np.asarray(lens, np.uint32), np.array([{**genotype.DEFAULTS, **pr}[k] for k in genotype.PARAMS], np.uint32)
        rc = genotype.lib().bmg_begin(c._h, a.ctypes.data_as(genotype._u32p), len(lens), t.ctypes.data_as(genotype._u32p))
        assert rc == genotype.BMG_ERR_ARG, lens
    same_cells(c, first[0], first[1], EDGE_REFS)          # the state is intact
    c.add(b"".join(good[100:]), offsets_of(good[100:]))  # ... and an add after a call keeps counting
    same_cells(c, n, Q, EDGE_REFS)
    same_calls(c, sites, called)
    # two calls with different lists are independent of each other
    half, other = sites[::2], sites[1::2][::-1]
    same_calls(c, half, called[::2])
    same_calls(c, other, called[1::2][::-1])
    same_calls(c, [], [])
    same_calls(c, sites, called)
    check(c, small, EDGE_REFS, small_sites)


def test_large_after_small_on_a_fresh_context():
    from bucket_map_amd import genotype
    fresh = genotype.Genotype(0)
    try:
        for call in (lambda: fresh.add(b"", [0]), lambda: fresh.call([site(0, 0, 0)]), lambda: fresh.call([]), lambda: fresh.cells_at(0, 0, 1)):
            with pytest.raises(genotype.BmgError) as e:
                call()
            assert e.value.code == genotype.BMG_ERR_ARG and "no bmg_begin" in str(e.value)
        fresh.begin([7])
        fresh.add(b"", [0])                              # no record: succeeds
        assert not fresh.cells_at(0, 0, 7).any() and fresh.call([]).shape == (0, 24)
        assert fresh.call([site(0, 6, 1)]).tolist() == [[0, 6, 1] + [0] * 21]
        recs, bases = edge_records(), edge_bases()
        check(fresh, recs, EDGE_REFS, sites_for(recs, EDGE_REFS, bases))
        big = [5, 3000000, 70000]
        bases = references(big, 10)
        recs = random_records(5001, 33, big, bases)
        check(fresh, recs, big, sites_for(recs, big, bases))
    finally:
        fresh.close()


def test_calls_at_the_borders_of_references(c):
    """The last base of a reference and the first of the next lie side by side in the state."""
    refs = [100, 1, 7, 300]
    recs = []
    for r, length in enumerate(refs):
        for p in sorted({0, length - 1}):
            alt = "ACGT"[(r + p + 1) % 4]
            recs += [rec_letters(r, p, "1M", alt, [20 + 7 * r + k], name=b"b%d_%d_%d" % (r, p, k)) for k in range(1 + r)]
    sites = [site(r, p, (r + p) % 4) for r, length in enumerate(refs) for p in sorted({0, 1, length - 2, length - 1} & set(range(length)))]
    n, Q, called = check(c, recs, refs, sites, prior=100)
    assert [x[22] for x in called] == [1, 0, 0, 1, 2, 3, 0, 0, 3, 4, 0, 0, 4] and kinds_of(called) == (7, 0, 6)
    assert len({(x[0], x[7]) for x in called if x[3] & 2}) == 4      # each reference's two calls are equal, the references' differ


def many_sites():
    """More than 65 535 sites: every covered position of a reference whose every letter is wrong."""
    refs = [90000, 300]
    bases = references(refs, 4)
    recs = random_records(12001, 41, refs, bases)
    sites = P.pile(recs, refs, flipped(bases), min_alt=1, min_frac_ppm=0).sites
    return refs, recs, sites


def test_site_lists_of_every_size(c):
    refs, recs, sites = many_sites()
    assert len(sites) > 65535 + 256
    n, Q, called = check(c, recs, refs, sites)
    assert kinds_of(called)[0] > 40000 and kinds_of(called)[1] > 1000
    for count in (0, 1, 255, 256, 257, 65535, 65536, 65537):
        same_calls(c, sites[7: 7 + count], called[7: 7 + count])
    # sites that are no SNV sites or have no reference allele between the others; then the list backwards
    mixed, want = [], []
    for k, (s, x) in enumerate(zip(sites[:3000], called[:3000])):
        mixed.append(s), want.append(x)
        if k % 3 == 0:
            other = site(s[0], s[1], s[2], kind=2 + 4 * (k % 2)) if k % 2 else site(s[0], s[1], 4)
            mixed.append(other), want.append(G.call_one(n[s[0]][s[1]].tolist(), Q[s[0]][s[1]].tolist(), other, G.DEFAULTS["prior"]))
    assert sum(1 for x in want if x[3] == 0) >= 1000
    same_calls(c, mixed, want)
    same_calls(c, mixed[::-1], want[::-1])
    same_calls(c, sites[::-1], called[::-1])
    same_calls(c, sites[:500] * 3, called[:500] * 3)       # a site may be asked for more than once


def test_counts_are_the_pileups_on_the_device(ref_bases):
    """n of the cells is bmp's A, C, G, T at every position when MAPQ and base-quality thresholds are equal."""
    from bucket_map_amd import genotype, pileup
    recs = random_records(3001, 5, bases=ref_bases)
    g, p = genotype.Genotype(0), pileup.Pileup(0)
    try:
        for th in (dict(min_mapq=0, min_bq=13), dict(min_mapq=20, min_bq=41), dict(min_mapq=0, min_bq=0)):
            stream, off = b"".join(recs), offsets_of(recs)
            g.begin(REF_LENS, **th)
            g.add(stream, off)
            p.begin(REF_LENS, ref_bases, **th)
            p.add(stream, off)
            p.finish()
            total = 0
            for r, length in enumerate(REF_LENS):
                cells, counts = g.cells_at(r, 0, length), p.counts_at(r, 0, length)
                assert np.array_equal((cells >> np.uint64(32)).astype(np.uint32), counts[:, :4]), (th, r)
                total += int(counts[:, :4].sum())
            assert total > 20000                         # about a third of the records are counted, with some 45 bases each
    finally:
        g.close()
        p.close()


# ---- the tools ----
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_pileup import pileup_jobs
    return pileup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_gpu_tool_writes_the_oracle_tools_file(jobs, k):
    name, which, d, args, extra = jobs[k]
    implied = ["--annotate"] if which == "bucketmap_align" else []
    loose = ["--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--pileup-min-bq", "0"]
    # the defaults in one run and in several; then looser thresholds, duplicates left out, --depth and --pileup beside it
    for tag, opts, env in ((name, [], None), (name + "r", ["--vcf-prior", "10"], dict(BM_SORT_RUN_BYTES="2000")),
                           (name + "m", ["--markdup", *loose, "--depth", f"{name}m.g.bedgraph", "--pileup", f"{name}m.g.tsv", "--vcf-min-qual", "60"], None)):
        err = run(TOOLS[(which, "oracle")], d, args, f"{tag}.go.bam", [*extra, *opts, "--vcf", f"{tag}.go.vcf"], env=env)
        want, told = (d / f"{tag}.go.vcf").read_text(), genotypes_line(err)
        assert want.startswith("##fileformat=VCFv4.2\n") and (name == "plain" or sum(1 for l in want.split("\n") if l and l[0] != "#") > 3)
        err = run(TOOLS[(which, "gpu")], d, args, f"{tag}.g.bam", [*extra, *opts, "--vcf", f"{tag}.g.vcf"], env=env)
        assert ("in 1 run(s)" in err) == (env is None) and genotypes_line(err) == told
        assert (d / f"{tag}.g.vcf").read_text() == want and pair_of(d, f"{tag}.g") == pair_of(d, f"{tag}.go")
    run(TOOLS[(which, "gpu")], d, args, f"{name}.gs.bam", [*extra, *implied, "--sort"])
    assert pair_of(d, f"{name}.gs") == pair_of(d, f"{name}.g")                   # --vcf changes neither the BAM nor its index
    assert name == "plain" or (d / f"{name}.g.vcf").read_text() != (d / f"{name}m.g.vcf").read_text()
