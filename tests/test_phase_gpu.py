"""bmk_begin / bmk_add / bmk_finish / bmk_phase / bmk_links on the MI355X against the rule in plain Python (tests/phase_rule.py)
-- every link counter and all eight words of every site, exactly --, and the product tools' --vcf-phase files and stderr line
against the oracle-backed tools' (whose phasing is host/phase.h): the rule is exact, so the files are equal.  Every tool run has
its own time limit; nothing is retried."""
import numpy as np
import pytest

import phase_rule as K
from phase_cases import DESIGNED, chain, het, hom, no_variant, planted_calls, reads_over
from pileup_cases import EDGE_REFS, REF_LENS, edge_records, many_ops_record, random_records, rec_letters, rec_seq, references
from test_bamsort import offsets_of, pair_of
from test_markdup_gpu import rec, rec_ops, run
from test_phase import edge_calls, phase_line, planted_haplotypes, truth_case
from test_sam_golden import TOOLS

pytestmark = pytest.mark.gpu

STRICT = dict(min_mapq=20, min_bq=14)


@pytest.fixture(scope="module")
def c():
    from bucket_map_amd import phase
    ctx = phase.Phase(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ref_bases():
    return references()


def same(c, want):
    """After bmk_finish: every counter, every word, and stretches of both."""
    sites, link, words, sums = want
    H = len(sites)
    assert c.n_sites == H
    got = c.links()
    assert got.shape == link.shape and np.array_equal(got, link), np.argwhere(got != link)[:10].tolist()
    out = c.phase()
    assert out.shape == (H, 8)
    if out.tolist() != [list(w) for w in words]:
        bad = [j for j, (a, b) in enumerate(zip(out.tolist(), words)) if tuple(a) != tuple(b)][:3]
        assert False, [(j, out[j].tolist(), words[j]) for j in bad]
    lo, count = H // 3, min(H - H // 3, 700)
    assert np.array_equal(c.phase(lo, count), out[lo: lo + count]) and np.array_equal(c.links(lo, count), got[lo: lo + count])
    assert c.phase(H, 0).shape == (0, 8) and c.links(H, 0).shape[0] == 0


def check(c, recs, ref_len, called, skip=None, cuts=None, want=None, **params):
    """The device's counters, words and sums for the records (added in the stretches cuts names) are the rule's; returns the rule's."""
    if want is None:
        want = K.run(recs, ref_len, called, skip, **params)
    cuts = [0, len(recs)] if cuts is None else cuts
    assert c.begin(ref_len, called, **params) == len(want[0])
    for a, b in zip(cuts, cuts[1:]):
        c.add(b"".join(recs[a:b]), offsets_of(recs[a:b]), None if skip is None else skip[a:b])
    assert np.array_equal(c.links(), want[1])            # the counters can be read before bmk_finish
    assert c.finish().tolist() == want[3]
    same(c, want)
    return want


def device_rule(c):
    """The device as the engine of the designed cases: what bmk_links, bmk_phase and bmk_finish give, after every counter and
    word has been compared with the Python rule too."""
    from bucket_map_amd import phase

    def rule(reads, calls, ref_len=(16,), **params):
        try:
            c.begin(list(ref_len), calls, **params)
        except phase.BmkError as e:
            assert e.code == phase.BMK_ERR_ARG
            with pytest.raises(K.Refused):               # ... and the Python rule refuses the same
                K.run(reads, list(ref_len), calls, **params)
            raise K.Refused(str(e))
        c.add(b"".join(reads), offsets_of(reads))
        sums = c.finish().tolist()
        want = K.run(reads, list(ref_len), calls, **params)
        assert sums == want[3]
        same(c, want)
        return c.links().astype(np.int64), [tuple(w) for w in c.phase().tolist()], sums
    return rule


@pytest.mark.parametrize("case", DESIGNED, ids=lambda f: f.__name__[5:])
def test_designed_cases(c, case):
    """A tie, min_links one short, min_frac_ppm exactly met and one below, a 1/2 het, a third letter and a low quality, a
    bridged false het, interleaved blocks, reach against the distance: the hand-worked values, on the device."""
    case(device_rule(c))


def test_truth_two_planted_haplotypes(c):
    truth_case(device_rule(c))


@pytest.mark.parametrize("bridged", [False, True])
@pytest.mark.parametrize("H", [0, 1, 2, 63, 64, 65, 257, 5000])
def test_chains(c, H, bridged):
    """One fully linked chain of H sites: 5 000 needs 13 jumping rounds and crosses workgroups.  bridged: every second link ties
    and the chain runs at d = 2 over it."""
    recs, ref_len, calls, haps = chain(H, 100 + H, bridged)
    sites, link, words, sums = check(c, recs, ref_len, calls)
    assert sums[:3] == [H, H if H > 1 else 0, 1 if H > 1 else 0]
    if H:
        assert [w[K.W_HAP] ^ haps[0] for w in words] == haps and {w[K.W_ROOT] for w in words} == {0}
        assert {w[K.W_D] for w in words[1:]} == ({1, 2} if bridged and H > 2 else {1} if H > 1 else set())
    if H > 1:
        assert c.ms_add > 0 and c.ms_finish > 0


@pytest.mark.parametrize("reach", [1, 4, 8])
@pytest.mark.parametrize("size", [65, 3001])
def test_random_records_over_planted_hets(c, ref_bases, size, reach):
    recs = random_records(size, 300 + size, bases=ref_bases)
    called = planted_calls(REF_LENS, ref_bases, 7 + size)
    sites, link, words, sums = check(c, recs, REF_LENS, called, reach=reach)
    if size == 3001:
        flags = [w[K.W_FLAGS] for w in words]
        assert flags.count(K.PHASED) > 20 and flags.count(K.ROOT) > 20 and sums[3] > 2000 and {w[K.W_HAP] for w in words} == {0, 1}
        assert {w[K.W_D] for w in words} == set(range(reach + 1)) or reach == 8
        for pr in (STRICT, dict(min_bq=0, min_links=1, min_frac_ppm=500001), dict(min_bq=256, min_mapq=200, min_frac_ppm=1000000)):
            check(c, recs, REF_LENS, called, reach=reach, **pr)


def test_edge_list(c):
    recs = edge_records()
    assert {len(r) % 16 for r in recs} == set(range(16))
    for pr in ({}, STRICT, dict(min_bq=0, reach=8), dict(min_bq=256, min_mapq=31, reach=1)):
        check(c, recs, EDGE_REFS, edge_calls(), **pr)
    for size in (1, 7, 40):                              # the same records as the first and the last of a stream
        check(c, recs[:size], EDGE_REFS, edge_calls(), **STRICT)
        check(c, recs[-size:], EDGE_REFS, edge_calls(), **STRICT)


def designed_edges():
    """Two references of 40 and 30 bases with a het at EVERY position (site number = position, + 40 on the second), alleles by
    position; records from two haplotypes over every kind of place a site can lie at."""
    refs = [40, 30]
    alleles = lambda p: (p % 4, (p + 1 + p // 4 % 3) % 4)
    calls = [het(r, p, *alleles(p + 7 * r)) for r, n in enumerate(refs) for p in range(n)]
    planted = np.random.default_rng(3).integers(0, 2, 70).tolist()

    def letters(r, pos, cigar, h, spoil=()):
        """The query of a record of haplotype h: at a block base the site's allele of that haplotype; spoil: query indices that
        get a third letter."""
        out, p = [], pos
        num = ""
        for ch in cigar:
            if ch.isdigit():
                num += ch
                continue
            n, num = int(num), ""
            for _ in range(n):
                if ch in "M=X":
                    a = alleles((p % refs[r]) + 7 * r)[h ^ planted[p % refs[r] + 40 * r]]
                    out.append("ACGT"[a])
                    p += 1
                elif ch in "IS":
                    out.append("ACGT"[(len(out) + h) % 4])
                elif ch in "DN":
                    p += 1
        for k in spoil:
            a = alleles((pos + k) % refs[r] + 7 * r)
            out[k] = "ACGT"[next(x for x in range(4) if x not in a)]
        return "".join(out)

    places = [(0, 10, "5M"),                             # sites at its first and last base
              (0, 36, "4M"), (0, 36, "9M"), (0, 39, "1M"), (0, 39, "6M"),   # the last base of a reference; past its end
              (1, 0, "3M"), (1, 26, "4M"), (1, 28, "7M"),                   # the first base of the next one; its end
              (0, 2, "2M3D2M"), (0, 12, "2M3N2M"), (0, 20, "2M2I2M"), (0, 25, "3S4M"), (0, 30, "2H1S3M2S"),
              (0, 0, "1=1X1=1X1=1X1=1X1=1X1=1X1=1X1=1X1=1X1=1X"),           # 20 ops: shared by the wave
              (0, 5, "30M"), (1, 3, "20M")]                                 # more than reach + 1 sites inside one op
    recs = []
    for k, (r, pos, cigar) in enumerate(places):
        for h in (0, 1):
            for copy in range(2):
                recs.append(rec_letters(r, pos, cigar, letters(r, pos, cigar, h), name=b"e%d_%d_%d" % (k, h, copy), flag=16 * copy))
    base = letters(0, 5, "30M", 0)
    quals = [40] * 30
    quals[3], quals[4], quals[5] = 12, 13, 255           # just below min_bq, at it, 0xFF
    recs += [rec_letters(0, 5, "30M", base, quals, name=b"q%d" % k) for k in range(3)]
    recs += [rec_letters(0, 5, "30M", letters(0, 5, "30M", 1, spoil=(2, 9)), name=b"third%d" % k) for k in range(3)]
    recs += [rec_letters(0, 5, "30M", base[:6] + "N" + base[7:10] + "=" + base[11:], name=b"ncode%d" % k) for k in range(3)]
    left_out = [rec_letters(0, 5, "30M", base, name=b"dup", flag=0x400), rec_letters(0, 5, "30M", base, name=b"sec", flag=0x100),
                rec_letters(0, 5, "30M", base, name=b"unmapped", flag=4), rec_letters(0, 5, "30M", base, name=b"low", mapq=19),
                rec_seq(0, 5, 0, [30 << 4 | 4, 30 << 4 | 3], [1] * 30, bytes([40] * 30), b"placeholder")]
    return refs, calls, recs, left_out


def test_sites_at_every_kind_of_place(c):
    refs, calls, recs, left_out = designed_edges()
    skip_one = rec_letters(0, 5, "30M", "A" * 30, name=b"skipped")
    everything = recs + left_out + [skip_one]
    skip = [0] * (len(everything) - 1) + [1]
    sites, link, words, sums = check(c, everything, refs, calls, skip, min_mapq=20)
    assert len(sites) == 70 and sums[3] > 500
    # what is left out counts nothing: the same counters without those records
    assert np.array_equal(K.run(recs, refs, calls, min_mapq=20)[1], link) and not np.array_equal(K.run(everything, refs, calls)[1], link)
    # no link and no parent across the border of the two references
    for d in range(1, 5):
        assert not link[40 - d, d - 1:].any()
    assert words[40][K.W_FLAGS] & K.ROOT and all(w[K.W_ROOT] >= 40 for w in words[40:]) and all(w[K.W_ROOT] < 40 for w in words[:40])
    assert sum(1 for w in words if w[K.W_FLAGS] & K.PHASED) > 40
    for reach in (1, 8):
        check(c, everything, refs, calls, skip, min_mapq=20, reach=reach)


def test_a_record_of_many_ops_and_a_long_block_beside_short_ones(c):
    """60 001 ops (938 trips of the wave walk) and 70 001 bases in one op at an odd position with an odd l_seq, in waves with
    short records; a het every fifth base or so: thousands of sites inside one op."""
    rng = np.random.default_rng(11)
    refs = [90000, 300]
    bases = references(refs, 4)
    codes = rng.choice(np.array([1, 2, 4, 8, 15, 0], np.uint8), 70001 + 3, p=[0.24, 0.24, 0.24, 0.24, 0.02, 0.02])
    qual = rng.choice(np.array([0, 12, 13, 40, 61, 93, 255], np.uint8), 70001 + 3)
    long_block = rec_seq(0, 33, 16, [3 << 4 | 4, 70001 << 4 | 0], codes, qual.tobytes(), b"long", mapq=60)
    over = rec_seq(0, 89990, 0, [40 << 4 | 0], codes[:40], qual[:40].tobytes(), b"over")
    recs = random_records(150, 5, refs, bases) + [many_ops_record(0, 17), long_block] + random_records(150, 6, refs, bases) + [many_ops_record(0, 0, 60001, seed=8), over,
                                                                                                             rec_letters(0, 100, "3M50000N3M", "ACGTAC", name=b"long_N"), rec_letters(0, 200, "3M40000D3M", "ACGTAC", name=b"long_D")]   # short records: thousands of sites under one N or D
    called = planted_calls(refs, bases, 3, gap=5)
    sites, link, words, sums = check(c, recs, refs, called)
    assert len(sites) > 10000 and sums[3] > 10000 and sums[1] > 500
    check(c, recs[::-1], refs, called, cuts=[0, 1, 150, 152, len(recs)], want=(sites, link, words, sums))


def test_cutting_and_order_do_not_matter(c, ref_bases):
    recs = random_records(3001, 21, bases=ref_bases)
    called = planted_calls(REF_LENS, ref_bases, 5)
    want = check(c, recs, REF_LENS, called)
    check(c, recs, REF_LENS, called, cuts=[0, 0, 1, 64, 65, 1000, 1002, 3001], want=want)
    check(c, recs[::-1], REF_LENS, called, cuts=[0, 300, 301, 700, 1500, 1501, 2999, 3001], want=want)
    order = np.random.default_rng(4).permutation(3001)
    check(c, [recs[i] for i in order], REF_LENS, called, cuts=[0, 64, 2000, 3001], want=want)


def test_skip_bytes_equal_removing_the_records(c, ref_bases):
    recs = random_records(3000, 77, bases=ref_bases)
    called = planted_calls(REF_LENS, ref_bases, 6)
    skip = [int(k % 3 == 1) for k in range(3000)]
    want = check(c, recs, REF_LENS, called, skip)
    kept = [r for r, s in zip(recs, skip) if not s]
    assert check(c, kept, REF_LENS, called, want=want) is want
    assert not np.array_equal(want[1], K.run(recs, REF_LENS, called)[1])


def refused(phase, call, word=None):
    with pytest.raises(phase.BmkError) as e:
        call()
    assert e.value.code == phase.BMK_ERR_ARG and (word is None or word in str(e.value)), str(e.value)


def test_small_after_large_and_refusals_between(c):
    from bucket_map_amd import phase
    big = [3000000, 70000, 5]
    big_bases = references(big, 9)
    big_recs = random_records(5001, 31, big, big_bases)
    big_called = planted_calls(big, big_bases, 8, gap=40)
    check(c, big_recs, big, big_called, reach=8)
    small = edge_records()
    check(c, small, EDGE_REFS, edge_calls(), **STRICT)    # nothing stale: fewer sites, a shorter reach, fewer records
    check(c, big_recs[::-1], big, big_called)
    bases = references(EDGE_REFS, 2)
    good = random_records(300, 8, EDGE_REFS, bases)
    called = planted_calls(EDGE_REFS, bases, 2, gap=3)
    c.begin(EDGE_REFS, called)
    c.add(b"".join(good[:100]), offsets_of(good[:100]))
    first = K.links(good[:100], EDGE_REFS, called)[1]
    bad_off = offsets_of(good)
    bad_off[5] += 1
    for stream, off in ((b"".join(good), bad_off), ([rec_ops(0, 0, 0, [3 << 4 | 9], b"")], None), ([rec(0, 5, 0, "3M", b"ab")], None), ([rec(3, 5, 0, "3M", b"")], None)):
        if off is None:
            stream, off = b"".join(stream), offsets_of(stream)
        refused(phase, lambda: c.add(stream, off))       # a refused add leaves what was added before
    H = c.n_sites
    refused(phase, lambda: c.phase(0, 1), "no bmk_finish")
    refused(phase, lambda: c.links(H, 1))
    refused(phase, lambda: c.links(0, H + 1))
    # a refused begin leaves the context as it was
    for lens, calls, pr in (([], called, {}), ([4, 0], called, {}), (EDGE_REFS, called, dict(reach=0)), (EDGE_REFS, called, dict(reach=9)),
                            (EDGE_REFS, called, dict(min_links=0)), (EDGE_REFS, called, dict(min_frac_ppm=500000)), (EDGE_REFS, called, dict(min_frac_ppm=1000001)),
                            (EDGE_REFS, [het(3, 0)], {}), (EDGE_REFS, [het(0, EDGE_REFS[0])], {}), (EDGE_REFS, [het(0, 1, 4, 1)], {}),
                            (EDGE_REFS, [het(0, 5), het(0, 5)], {}), (EDGE_REFS, [het(1, 0), het(0, 7)], {})):
        a = np.asarray(lens, np.uint32)
        t = np.array([{**K.DEFAULTS, **pr}[k] for k in phase.PARAMS], np.uint32)
        s = np.asarray(calls, np.uint32).reshape(-1, 24)
        rc = phase.lib().bmk_begin(c._h, a.ctypes.data_as(phase._u32p), len(lens), t.ctypes.data_as(phase._u32p), s.ctypes.data_as(phase._u32p), s.shape[0], None)
        assert rc == phase.BMK_ERR_ARG, (lens, pr)
    assert np.array_equal(c.links(), first)              # the state is intact
    c.add(b"".join(good[100:]), offsets_of(good[100:]))
    want = K.run(good, EDGE_REFS, called)
    assert c.finish().tolist() == want[3]
    same(c, want)
    refused(phase, lambda: c.add(b"".join(good[:5]), offsets_of(good[:5])), "bmk_finish")   # after bmk_finish: refused until the next bmk_begin
    refused(phase, lambda: c.finish(), "bmk_begin")
    refused(phase, lambda: c.phase(H, 1))
    refused(phase, lambda: c.phase(1, H))
    same(c, want)
    check(c, small, EDGE_REFS, edge_calls())


def test_large_after_small_on_a_fresh_context():
    from bucket_map_amd import phase
    fresh = phase.Phase(0)
    try:
        for call in (lambda: fresh.add(b"", [0]), lambda: fresh.finish(), lambda: fresh.phase(0, 0), lambda: fresh.links(0, 0)):
            refused(phase, call, "no bmk_")
        recs = edge_records()
        # no call, and calls none of which is a phase site: every later call succeeds and launches nothing
        for calls in ([], [hom(0, 3), no_variant(0, 4), hom(9, 9, 9)]):
            assert fresh.begin(EDGE_REFS, calls) == 0
            fresh.add(b"".join(recs), offsets_of(recs))
            assert fresh.finish().tolist() == [0, 0, 0, 0] and fresh.phase().shape == (0, 8) and fresh.links().shape[0] == 0 and fresh.ms_add == 0 and fresh.ms_finish == 0
        assert fresh.begin([7], [het(0, 6)]) == 1
        fresh.add(b"", [0])                              # no record: succeeds
        assert fresh.finish().tolist() == [1, 0, 0, 0] and fresh.phase().tolist() == [[0, 0, 6, 0, K.ROOT, 0, 0, 0]] and not fresh.links().any()
        check(fresh, recs, EDGE_REFS, edge_calls())
        big = [5, 3000000, 70000]
        bases = references(big, 10)
        recs = random_records(5001, 33, big, bases)
        check(fresh, recs, big, planted_calls(big, bases, 9, gap=40))
    finally:
        fresh.close()


# ---- the tools ----
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp("phase_tools_gpu")
    args, extra = planted_haplotypes(d)
    return d, args, extra


MIXES = [("gi", ["--vcf-indels", "--gvcf", "gi.X.g.vcf"], None), ("b", ["--vcf-bias"], None), ("m", ["--markdup"], dict(BM_SORT_RUN_BYTES="2000"))]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_gpu_tool_writes_the_oracle_tools_files(planted, k):
    d, args, extra = planted
    tag, opts, env = MIXES[k]
    files = {}
    for kind in ("oracle", "gpu"):
        named = [o.replace("X", kind) for o in opts]
        err = run(TOOLS[("bucketmap_align", kind)], d, args, f"{tag}.{kind}.bam", [*extra, *named, "--vcf", f"{tag}.{kind}.vcf", "--vcf-phase"], env=env)
        assert ("in 1 run(s)" in err) == (env is None)
        files[kind] = (phase_line(err), (d / f"{tag}.{kind}.vcf").read_text(), (d / f"gi.{kind}.g.vcf").read_text() if k == 0 else "", pair_of(d, f"{tag}.{kind}"))
    assert files["gpu"] == files["oracle"]
    told, text = files["gpu"][:2]
    assert told.startswith("Phase: 5 of 5 het SNVs phased in 2 blocks (longest 46 bases, ") and text.count("|") == 5 and text.count(":PS\t") == 5
    assert k != 0 or files["gpu"][2].count("|") == 5
    assert k != 1 or "GT:DP:AD:ADF:ADR:GQ:PL:PS" in text


def test_gpu_tool_without_the_option_writes_the_unphased_file(planted):
    d, args, extra = planted
    err0 = run(TOOLS[("bucketmap_align", "gpu")], d, args, "n.gpu.bam", [*extra, "--vcf", "n.gpu.vcf"])
    assert "Phase:" not in err0 and "PS" not in (d / "n.gpu.vcf").read_text()
    run(TOOLS[("bucketmap_align", "gpu")], d, args, "p.gpu.bam", [*extra, "--vcf", "p.gpu.vcf", "--vcf-phase"])
    assert K.unphased_vcf((d / "p.gpu.vcf").read_text()) == (d / "n.gpu.vcf").read_text() and pair_of(d, "p.gpu") == pair_of(d, "n.gpu")
