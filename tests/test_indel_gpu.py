"""bmn_begin / bmn_add / bmn_finish and the lists behind them on the MI355X against the rule in plain Python
(tests/indel_rule.py): the unsorted events of every add, all eight words of every allele, all sixteen of every call, the
per-reference sums and cover at every position of small references, exactly; the sums against bmp's on the device; and the
product tools' --vcf-indels file and stderr line against the oracle-backed tools' (whose calling is host/indel.h).  Every tool
run has its own time limit; nothing is retried."""
import numpy as np
import pytest

import indel_rule as N
from indel_cases import (ABC, L, edge_placements, homopolymer_reads, ins_record, many_indel_ops, min_frac_records, same_anchor_records, threshold_records)
from pileup_cases import EDGE_REFS, REF_LENS, edge_records, random_records, rec_letters, references
from test_bamsort import offsets_of

pytestmark = pytest.mark.gpu

STRICT = dict(min_mapq=20, min_alt=1, min_frac_ppm=0, q_indel=17, prior=123)
LOOSE = dict(min_alt=1, min_frac_ppm=0)


@pytest.fixture(scope="module")
def c():
    from bucket_map_amd import indel
    ctx = indel.Indel(0)
    yield ctx
    ctx.close()


def rows(a):
    return [tuple(int(v) for v in x) for x in a]


def same_lists(c, want, ref_len, stats, windows=None):
    assert (c.n_events, c.n_alleles, c.n_calls) == (len(want.events), len(want.alleles), len(want.calls))
    assert stats.tolist() == want.stats
    got = rows(c.alleles())
    assert got == want.alleles, [(i, a, b) for i, (a, b) in enumerate(zip(got, want.alleles)) if a != b][:3]
    got = rows(c.calls())
    assert got == want.calls, [(i, a, b) for i, (a, b) in enumerate(zip(got, want.calls)) if a != b][:3]
    if c.n_calls > 2:
        assert rows(c.calls(1, c.n_calls - 2)) == want.calls[1:-1] and rows(c.alleles(c.n_alleles - 1, 1)) == want.alleles[-1:]
    assert c.calls(c.n_calls, 0).shape == (0, 16) and c.alleles(0, 0).shape == (0, 8)
    for r, length in enumerate(ref_len):
        for start, count in ([(0, length)] if windows is None else windows.get(r, [])):
            got = c.cover_at(r, start, count)
            assert np.array_equal(got, want.cover[r][start: start + count]), (r, start, np.flatnonzero(got != want.cover[r][start: start + count])[:10])


def check(c, recs, ref_len, skip=None, cuts=None, want=None, windows=None, **params):
    """The device's events, alleles, calls, sums and cover for the records (added in the stretches cuts names) are the rule's;
    returns the rule's."""
    in_order = want is None
    want = N.indels(recs, ref_len, skip, **params) if want is None else want
    cuts = [0, len(recs)] if cuts is None else cuts
    c.begin(ref_len, **params)
    n_adds = 0
    for a, b in zip(cuts, cuts[1:]):
        c.add(b"".join(recs[a:b]), offsets_of(recs[a:b]), None if skip is None else skip[a:b])
        n_adds += b > a
    assert c.n_adds() == n_adds
    events = [e for k in range(n_adds) for e in rows(c.events_of(k))]
    assert events == want.events if in_order else sorted(events) == sorted(want.events)
    same_lists(c, want, ref_len, c.finish(), windows)
    return want


@pytest.fixture(scope="module")
def ref_bases():
    return references()


@pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 257, 3001])
def test_sizes(c, ref_bases, size):
    recs = random_records(size, 300 + size, bases=ref_bases)
    want = check(c, recs, REF_LENS, **LOOSE)
    if size >= 257:
        assert len(want.events) > size // 20 and len(want.calls) > 5 and (size < 3001 or {x[6] for x in want.calls} == {0, 1, 2})
        check(c, recs, REF_LENS)                         # the defaults
        assert c.ms_add > 0 and c.ms_finish > 0


def test_cutting_and_order_do_not_matter(c, ref_bases):
    recs = random_records(3001, 21, bases=ref_bases)
    want = check(c, recs, REF_LENS, **LOOSE)
    check(c, recs, REF_LENS, cuts=[0, 1000, 1002, 3001], **LOOSE)
    check(c, recs, REF_LENS, cuts=[0, 0, 1, 64, 65, 1000, 2000, 3001], want=want, **LOOSE)
    order = np.random.default_rng(4).permutation(3001)
    check(c, [recs[i] for i in order], REF_LENS, cuts=[0, 64, 2000, 3001], want=want, **LOOSE)
    check(c, [recs[i] for i in order[::-1]], REF_LENS, cuts=[0, 300, 301, 700, 1500, 1501, 2999, 3001], want=want, **LOOSE)
    skip = [int(k % 3 == 1) for k in range(3001)]
    kept = check(c, recs, REF_LENS, skip, **LOOSE)
    check(c, [r for r, s in zip(recs, skip) if not s], REF_LENS, want=kept, **LOOSE)
    assert kept.alleles != want.alleles


def test_edge_list_of_the_pileup(c):
    recs = edge_records()
    for pr in (LOOSE, STRICT, {}):
        check(c, recs, EDGE_REFS, **pr)
    for r in recs:
        check(c, [r], EDGE_REFS, **STRICT)


@pytest.mark.parametrize("size", [1, 16, 31, 32, 33])
def test_insertion_lengths_at_even_and_odd_query_offsets(c, size):
    """Record alignments 0 .. 3 by name lengths; 33 bases become `other`."""
    rng = np.random.default_rng(size)
    recs = []
    for name in (b"", b"x", b"xy", b"xyz"):
        for lead in (3, 4):
            ins = "".join(ABC[k] for k in rng.integers(0, 4, size))
            recs += [ins_record(0, 10 + lead, lead, ins, name)] * 2
    assert {len(r) % 4 for r in recs} == {0, 1, 2, 3}
    want = check(c, recs, [100, 7], **LOOSE)
    assert len(want.events) == 16 and all(bool(a[2] & N.OTHER) == (size == 33) for a in want.alleles) and len(want.calls) == (0 if size == 33 else 2)


def test_other_codes_and_the_ends_of_the_sequence_key(c):
    recs = [ins_record(0, 5, 3, "ACNGT", b"n_inside"), ins_record(0, 5, 3, "ACNGT", b"n_inside2"), ins_record(0, 5, 3, "ACCGT", b"clean")]
    a, z = "A" * 31, "T" * 31
    recs += [ins_record(0, 20, 4, a + "C", b"last_c"), ins_record(0, 20, 4, a + "G", b"last_g"), ins_record(0, 20, 4, a + "G", b"last_g2")]
    recs += [ins_record(0, 40, 5, "C" + z, b"first_c"), ins_record(0, 40, 5, "G" + z, b"first_g"), ins_record(0, 40, 5, "C" + z, b"first_c2")]
    want = check(c, recs, [100], **LOOSE)
    assert [a[5] for a in want.alleles] == [1, 2, 1, 2, 2, 1] and want.alleles[1][2] & N.OTHER
    assert [(x[1], x[10], x[11]) for x in want.calls] == [(7, 1, 2), (23, 2, 1), (44, 2, 1)]
    assert want.calls[1][4] >> 30 == 2 and want.calls[2][3] & 3 == 1


def test_edge_placements(c):
    refs, recs, expect = edge_placements()
    for k, (r, n) in enumerate(zip(recs, expect)):
        assert len(N.indels([r], refs, **LOOSE).events) == n, k
    want = check(c, recs, refs, **LOOSE)
    both = [x for x in want.calls if x[:2] == (0, 22)]    # I then D on one anchor: two events of one read, n_ref saturates at 0
    assert both and both[0][9] == 0 and both[0][12] == 1 and both[0][11] == 1
    assert {(a[0], a[1]) for a in want.alleles} >= {(0, 0), (0, 48), (1, 28)} and not want.cover[0][49]
    for r in recs:
        check(c, [r], refs, **LOOSE)


def test_a_record_of_many_ops_beside_short_ones(c):
    """60 001 ops that alternate M / I / D: 938 trips of the wave walk with the cursors, the anchored flag and the event offset
    carried from each to the next; also 65 and 129 ops."""
    refs = [90000, 300]
    bases = references(refs, 4)
    long_one = many_indel_ops(0, 17, 60001, 3)
    recs = random_records(150, 5, refs, bases) + [long_one] + random_records(150, 6, refs, bases) + [many_indel_ops(0, 40000, 65, 4), many_indel_ops(1, 3, 129, 5)]
    want = check(c, recs, refs, **LOOSE)
    assert len(want.events) > 30000 + 32 + 64
    check(c, recs, refs, cuts=[0, 151, 300, 303], want=want, **LOOSE)
    alone = check(c, [long_one], refs, **LOOSE)
    assert len(alone.events) == 30000 and len(alone.calls) == 30000
    for n_ops in (65, 129, 64, 9):
        check(c, [many_indel_ops(1, 3, n_ops, 6)], refs, **LOOSE)


def test_many_alleles_and_many_events_on_one_anchor(c):
    recs = same_anchor_records(300, 5000)
    want = check(c, recs, [200, 64], **LOOSE)
    assert len(want.alleles) == 301 and len(want.calls) == 2 and want.calls[1][10] == 5000 and want.calls[0][11] == 299
    check(c, recs[::-1], [200, 64], cuts=[0, 2500, 5300], want=want, **LOOSE)


def test_anchors_beyond_slot_2_24(c):
    """Every digit of the second sort's key is live: slots on both sides of 2^24, a length above 2^16, both kinds."""
    refs = [17_000_000, 100]
    recs = [rec_letters(0, 3, "4M1I4M", "ACGTACGTA", name=b"low"), rec_letters(0, 300, "4M2D4M", "ACGTACGT", name=b"d300")]
    recs += [rec_letters(0, 70000, "5M70000D5M", "ACGTACGTAC", name=b"long_d%d" % k) for k in range(2)]
    for k, p in enumerate((2 ** 24 - 3, 2 ** 24 + 70000, 16_999_900, 16_999_990)):
        recs += [ins_record(0, p, 3, "GA", b"hi%d_%d" % (k, j)) for j in range(3)] + [rec_letters(0, p + 5, "2M3D4M", "ACGTAC", name=b"hd%d" % k)]
    recs += [rec_letters(1, 90, "5M1I5M", "ACGTACGTACG", name=b"next")] * 2
    windows = {0: [(0, 400), (69990, 40), (139990, 40), (2 ** 24 - 100, 200), (16_999_000, 1000)], 1: [(0, 100)]}
    want = check(c, recs, refs, windows=windows, **LOOSE)
    assert len(want.calls) == 12 and max(a[1] for a in want.alleles) > 16_999_990 and want.alleles[-1][0] == 1
    check(c, recs[::-1], refs, want=want, windows=windows, **LOOSE)


def test_thresholds_at_their_edges(c):
    recs = threshold_records()
    at3 = check(c, recs, [100], min_alt=3, min_frac_ppm=0)
    assert [x[1] for x in at3.calls] == [32]              # two reads at anchor 12, three at 32
    assert [x[1] for x in check(c, recs, [100], min_alt=2, min_frac_ppm=0).calls] == [12, 32]
    recs = min_frac_records()                             # one insertion among four spanning reads
    assert len(check(c, recs, [100], min_alt=1, min_frac_ppm=250000).calls) == 1
    assert len(check(c, recs, [100], min_alt=1, min_frac_ppm=250001).calls) == 0
    # RR against RA: one read with and one without, 100 q = 700 against 602 + prior
    pair = [ins_record(0, 10, 4, "C", b"with"), L(0, 10, "9M", "ACGTACGTA", name=b"without")]
    tie = check(c, pair, [100], min_alt=1, min_frac_ppm=0, q_indel=7, prior=98)
    assert tie.calls[0][6] == 0 and tie.calls[0][5] == 1 and tie.calls[0][7] == 0
    assert check(c, pair, [100], min_alt=1, min_frac_ppm=0, q_indel=7, prior=97).calls[0][6] == 1
    assert check(c, pair, [100], min_alt=1, min_frac_ppm=0, q_indel=7, prior=0).calls[0][6] == 1
    hom = check(c, pair[:1] * 3, [100], min_alt=1, min_frac_ppm=0, prior=0)
    assert hom.calls[0][6] == 2 and hom.calls[0][13] == 9000


def test_small_after_large_and_begin_again(c):
    from bucket_map_amd import indel
    big = [3000000, 70000, 5]
    big_recs = random_records(5001, 31, big, references(big, 9))
    want_big = check(c, big_recs, big, **LOOSE)
    small = edge_records()
    check(c, small, EDGE_REFS, **STRICT)                  # nothing stale: smaller references, fewer records, other parameters
    check(c, big_recs[::-1], big, want=want_big, **LOOSE)
    c.begin(EDGE_REFS, **LOOSE)
    c.add(b"".join(small[:20]), offsets_of(small[:20]))
    c.begin(EDGE_REFS, **LOOSE)                          # starts over: nothing of the twenty remains
    assert c.n_adds() == 0
    c.add(b"".join(small[20:]), offsets_of(small[20:]))
    bad_off = offsets_of(small)
    bad_off[5] += 1
    with pytest.raises(indel.BmnError) as e:
        c.add(b"".join(small), bad_off)
    assert e.value.code == indel.BMN_ERR_ARG
    with pytest.raises(indel.BmnError) as e:
        c.calls(0, 1)
    assert e.value.code == indel.BMN_ERR_ARG and "no bmn_finish" in str(e.value)
    want = N.indels(small[20:], EDGE_REFS, **LOOSE)
    same_lists(c, want, EDGE_REFS, c.finish())
    for call in (lambda: c.add(b"", [0]), lambda: c.finish(), lambda: c.cover_at(3, 0, 1), lambda: c.cover_at(1, 45, 6),
                 lambda: c.calls(c.n_calls, 1), lambda: c.alleles(1, c.n_alleles), lambda: c.events_of(1)):
        with pytest.raises(indel.BmnError) as e:
            call()
        assert e.value.code == indel.BMN_ERR_ARG
    same_lists(c, want, EDGE_REFS, np.array(want.stats, np.uint64))   # the lists are intact


def test_sums_are_the_pileups_on_the_device(ref_bases):
    from bucket_map_amd import indel, pileup
    recs = random_records(3001, 5, bases=ref_bases)
    stream, off = b"".join(recs), offsets_of(recs)
    n, p = indel.Indel(0), pileup.Pileup(0)
    try:
        for mapq in (0, 20, 200):
            n.begin(REF_LENS, min_mapq=mapq)
            n.add(stream, off)
            stats = n.finish()
            p.begin(REF_LENS, ref_bases, min_mapq=mapq)
            p.add(stream, off)
            assert np.array_equal(stats, p.finish()[1][:, :3]) and int(stats[:, 0].sum()) + int(stats[:, 1].sum()) > 500
    finally:
        n.close()
        p.close()


# ---- the tools ----
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_pileup import pileup_jobs
    return pileup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_gpu_tool_writes_the_oracle_tools_file(jobs, k):
    from test_bamsort import pair_of
    from test_indel import INFO_LINE, indels_line
    from test_markdup_gpu import run
    from test_sam_golden import TOOLS
    name, which, d, args, extra = jobs[k]
    loose = ["--pileup-min-alt", "1", "--pileup-min-frac", "0.000001", "--vcf-indel-qual", "9", "--vcf-indel-prior", "5"]
    # without the option the file is today's: the oracle-backed tool's and the product's own --vcf file
    run(TOOLS[(which, "oracle")], d, args, f"{name}.io0.bam", [*extra, "--vcf", f"{name}.io0.vcf"])
    err = run(TOOLS[(which, "gpu")], d, args, f"{name}.i0.bam", [*extra, "--vcf", f"{name}.i0.vcf"])
    today = (d / f"{name}.i0.vcf").read_text()
    assert today == (d / f"{name}.io0.vcf").read_text() and "Indels:" not in err and "INDEL" not in today
    # with it: the defaults in one run; looser thresholds in several runs with duplicates left out
    for tag, opts, env in ((name, [], None), (name + "r", ["--markdup", *loose], dict(BM_SORT_RUN_BYTES="2000"))):
        err = run(TOOLS[(which, "oracle")], d, args, f"{tag}.io.bam", [*extra, *opts, "--vcf", f"{tag}.io.vcf", "--vcf-indels"], env=env)
        want, told = (d / f"{tag}.io.vcf").read_text(), indels_line(err)
        assert INFO_LINE in want and (name == "plain") == (" from 0 events" in told)
        err = run(TOOLS[(which, "gpu")], d, args, f"{tag}.i.bam", [*extra, *opts, "--vcf", f"{tag}.i.vcf", "--vcf-indels"], env=env)
        assert ("in 1 run(s)" in err) == (env is None) and indels_line(err) == told
        assert (d / f"{tag}.i.vcf").read_text() == want and pair_of(d, f"{tag}.i") == pair_of(d, f"{tag}.io")
    assert pair_of(d, f"{name}.i") == pair_of(d, f"{name}.i0")                   # --vcf-indels changes neither the BAM nor its index
    assert [l for l in (d / f"{name}.i.vcf").read_text().split("\n") if "\tINDEL;" not in l and l != INFO_LINE] == today.split("\n")
    assert name == "plain" or sum(1 for l in (d / f"{name}r.i.vcf").read_text().split("\n") if "\tINDEL;" in l) >= 2


def test_one_deletion_in_a_homopolymer_from_both_strands(jobs):
    """Reads of both strands that lack one base of a run of five equal letters, each at another place of the run: with --affine
    --left-align every read shows the same deletion at the same anchor, and the file has one line for it."""
    from test_indel import indels_line
    from test_markdup_gpu import run
    from test_sam_golden import TOOLS
    name, which, d, args, extra = jobs[1]
    assert which == "bucketmap_align"
    text, ref, start, letter, before = homopolymer_reads((d / args[args.index("--genome") + 1]).read_text(), int(args[args.index("-r") + 1]))
    (d / "homo.fastq").write_text(text)
    args = list(args)
    args[args.index("-q") + 1] = "homo.fastq"
    opts = [*extra, "--affine", "--left-align", "--vcf-indels", "--pileup-min-alt", "1"]
    told = indels_line(run(TOOLS[(which, "oracle")], d, args, "homo.o.bam", [*opts, "--vcf", "homo.o.vcf"]))
    assert indels_line(run(TOOLS[(which, "gpu")], d, args, "homo.g.bam", [*opts, "--vcf", "homo.g.vcf"])) == told
    got = (d / "homo.g.vcf").read_text()
    assert got == (d / "homo.o.vcf").read_text()
    lines = [l.split("\t") for l in got.split("\n") if "\tINDEL;" in l]
    assert len(lines) == 1 and lines[0][:5] == [ref, str(start), ".", before + letter, before] and lines[0][9][:3] in ("0/1", "1/1"), lines
    assert told.startswith("Indels: 1 variants") and " at 1 sites from 12 events" in told
