"""bmr_run / bmr_blocks / bmr_conf_at on the MI355X against the rule in plain Python (tests/refblocks_rule.py): both words of
every position and all eight words of every block, exactly; and the product tools' --gvcf file and stderr line against the
oracle-backed tools' (whose blocks are host/refblocks.h): the rule is exact, so the files are equal.  Every tool run has its own
time limit; nothing is retried."""
import ctypes as C

import numpy as np
import pytest

import genotype_rule as G
import refblocks_rule as R
from pileup_cases import EDGE_REFS, REF_LENS, edge_bases, edge_records, random_records, rec_letters, references
from test_bamsort import offsets_of, pair_of
from test_genotype import PARAM_SETS
from test_markdup_gpu import run
from test_refblocks import blocks_line
from test_sam_golden import TOOLS

pytestmark = pytest.mark.gpu

STRICT = dict(min_mapq=20, min_bq=13, q_cap=40, q_absent=7, prior=1234)
SIXTEEN = tuple(range(3, 99, 6))
assert len(SIXTEEN) == 16


@pytest.fixture(scope="module")
def g():
    from bucket_map_amd import genotype
    ctx = genotype.Genotype(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def c():
    from bucket_map_amd import refblocks
    ctx = refblocks.RefBlocks(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ref_bases():
    return references()


def same(c, g, want, ref_len, bases, bands=R.DEFAULT_BANDS, exclude=()):
    """The device's run over the cells g holds gives the rule's per-position words and blocks."""
    word0, dp, blks = want
    assert c.run(g, bases, bands, exclude) == len(blks)
    got = c.blocks()
    assert got.shape == (len(blks), 8)
    if got.tolist() != [list(b) for b in blks]:
        bad = [i for i, (a, b) in enumerate(zip(got.tolist(), blks)) if tuple(a) != b][:3]
        assert False, [(i, got[i].tolist(), blks[i]) for i in bad]
    for r, length in enumerate(ref_len):
        conf, rule = c.conf_at(r, 0, length), R.conf_words(word0[r], dp[r])
        assert np.array_equal(conf, rule), (r, np.flatnonzero((conf != rule).any(axis=1))[:10])
        lo = length // 3
        assert np.array_equal(c.conf_at(r, lo, length - lo), rule[lo:]) and c.conf_at(r, length, 0).shape == (0, 2)
    if len(blks) > 2:
        assert c.blocks(1, len(blks) - 2).tolist() == [list(b) for b in blks[1:-1]] and c.blocks(len(blks), 0).shape == (0, 8)
    R.check_tiling(blks, word0)


def check(c, g, recs, ref_len, bases, bands=R.DEFAULT_BANDS, exclude=(), cuts=None, **params):
    n, Q = G.cells(recs, ref_len, **params)
    want = R.run(n, Q, bases, bands, exclude)
    cuts = [0, len(recs)] if cuts is None else cuts
    g.begin(ref_len, **params)
    for a, b in zip(cuts, cuts[1:]):
        g.add(b"".join(recs[a:b]), offsets_of(recs[a:b]))
    same(c, g, want, ref_len, bases, bands, exclude)
    return want


def column(ref, pos, letters_and_times, qual=30):
    """One-base reads at one position: [(letter, times)]."""
    return [rec_letters(ref, pos, "1M", letter, [qual], name=b"c%d_%d_%s%d" % (ref, pos, letter.encode(), k)) for letter, times in letters_and_times
            for k in range(times)]


@pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 257, 3001])
def test_sizes(c, g, ref_bases, size):
    recs = random_records(size, 300 + size, bases=ref_bases)
    word0, dp, blks = check(c, g, recs, REF_LENS, ref_bases)
    check(c, g, recs, REF_LENS, ref_bases, bands=())
    check(c, g, recs, REF_LENS, ref_bases, bands=SIXTEEN)
    assert c.ms_kernels > 0 and c.bytes_state >= 17 * sum(REF_LENS)
    if size >= 257:
        assert len({b[3] for b in blks}) > 5 and any(b[2] - b[1] > 64 for b in blks) and any(b[2] - b[1] == 1 for b in blks)


def test_edge_list(c, g):
    recs, bases = edge_records(), edge_bases()
    for pr in (*PARAM_SETS, STRICT):
        word0, dp, blks = check(c, g, recs, EDGE_REFS, bases, **pr)
    assert any((w & R.NO_ALLELE).any() for w in word0) and len(blks) > 5


def test_geometry_on_lane_wave_and_workgroup_borders(c, g):
    refs = [1, 63, 64, 65, 255, 256, 257, 2049, 300001, 70, 70, 4100]
    bases = [bytearray(b"ACGT"[k % 4: k % 4 + 1] * length) for k, length in enumerate(refs)]
    bases[3][0] = ord("N")                                # R = 4 at the first base, at the last base, and in a run
    bases[4][254] = ord("n")
    bases[7][1000:1100] = b"N" * 100
    bases[11][3000] = ord("R")
    bases = [bytes(b) for b in bases]
    recs = []
    letter = lambda r: "ACGT"[r % 4]
    # a depth step at 63/64/65, 255/256/257 and 2047/2048/2049 of reference 11: three reads end at each, gq falls by 9 from 81
    # to 0 and crosses a default bound every time
    for edge in (63, 64, 65, 255, 256, 257, 2047, 2048, 2049):
        recs += [rec_letters(11, 0, f"{edge}M", letter(11) * edge, [30] * edge, name=b"s%d_%d" % (edge, k)) for k in range(3)]
    recs += [rec_letters(7, 2040, "9M", letter(7) * 9, [30] * 9, name=b"t%d" % k) for k in range(12)]   # the last base of 7
    recs += column(0, 0, [(letter(0), 40)])              # the reference of one base, deep enough for 99
    word0, dp, blks = check(c, g, recs, refs, bases)
    assert [b for b in blks if b[0] == 8] == [(8, 0, 300001, 0, 0, 0, 0, 0)]                  # one block across many workgroups
    assert [b[:3] for b in blks if b[0] in (9, 10)] == [(9, 0, 70), (10, 0, 70)]              # two uncovered neighbours: two blocks
    assert blks[0] == (0, 0, 1, 11, 99, 40, 40, 0)
    assert [b[1] for b in blks if b[0] == 11][:10] == [0, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
    assert [b[4] for b in blks if b[0] == 11][:10] == [81, 72, 63, 54, 45, 36, 27, 18, 9, 0]
    check(c, g, recs, refs, bases, bands=(), exclude=[(8, 150000, 150001)])
    check(c, g, recs, refs, bases, bands=SIXTEEN, exclude=[(r, 0, 1) for r in range(len(refs))] + [(r, length - 1, length) for r, length in enumerate(refs)])


def test_blocks_of_one_base(c, g):
    refs = [4097, 3]
    bases = references(refs, 3)
    recs = random_records(200, 9, refs, bases)
    odd = [(r, p, p + 1) for r, length in enumerate(refs) for p in range(1, length, 2)]
    word0, dp, blks = check(c, g, recs, refs, bases, exclude=odd)
    assert len(blks) > 2000 and all(b[2] - b[1] == 1 for b in blks)


def test_intervals(c, g, ref_bases):
    recs = random_records(3001, 12, bases=ref_bases)
    last = len(REF_LENS) - 1
    messy = [(1, 50, 60), (1, 10, 20), (1, 55, 70), (1, 70, 80), (1, 15, 16), (last, 0, 1), (1, 0, 1), (1, REF_LENS[1] - 1, REF_LENS[1]),
             (last, REF_LENS[last] - 1, REF_LENS[last]), (1, 10, 20), (0, 0, 1)]
    check(c, g, recs, REF_LENS, ref_bases, exclude=messy)
    whole = [(r, 0, length) for r, length in enumerate(REF_LENS)]
    assert check(c, g, recs, REF_LENS, ref_bases, exclude=whole)[2] == []      # every reference covered: no blocks
    check(c, g, recs, REF_LENS, ref_bases, exclude=whole[1:])
    refs = [30011, 21000]
    bases = references(refs, 6)
    recs = random_records(1000, 13, refs, bases)
    check(c, g, recs, refs, bases, exclude=[(0, 12345, 22345)])                # one of 10 000 bases
    rng = np.random.default_rng(5)
    ones = [(1, int(p), int(p) + 1) for p in rng.permutation(21000)[:10000]]   # 10 000 of one base
    check(c, g, recs, refs, bases, exclude=ones)
    check(c, g, recs, refs, bases, exclude=ones + [(0, 12345, 22345)] + ones[:100])


def test_saturation_and_a_losing_rr(c, g):
    refs = [40, 9]
    bases = [b"A" * 40, b"ACGTNacgt"]
    recs = column(0, 3, [("A", 10)]) + column(0, 5, [("A", 40)]) + column(0, 7, [("A", 5), ("C", 5)]) + column(0, 9, [("A", 9)]) + column(0, 9, [("G", 1)], 20)
    recs += column(0, 11, [("A", 300)]) + column(1, 5, [("A", 12)]) + column(1, 4, [("C", 3)])
    word0, dp, blks = check(c, g, recs, refs, bases)
    assert [int(word0[0][p]) & 0xFF for p in (2, 3, 5, 7, 9, 11)] == [0, 30, 99, 0, 5, 99]
    assert int(dp[0][11]) == 300 and int(word0[1][4]) == R.NO_ALLELE and int(dp[1][4]) == 3


def test_context_reuse(c, g, ref_bases):
    from bucket_map_amd import genotype
    recs = random_records(3001, 21, bases=ref_bases)
    want = check(c, g, recs, REF_LENS, ref_bases)
    assert check(c, g, recs, REF_LENS, ref_bases, cuts=[0, 0, 1, 64, 65, 1000, 2000, 3001])[2] == want[2]      # however the records are cut
    # bmr_run, more bmg_add, bmr_run again: the blocks of everything added by then; the run changes no cell
    g.begin(REF_LENS)
    g.add(b"".join(recs[:1000]), offsets_of(recs[:1000]))
    n, Q = G.cells(recs[:1000], REF_LENS)
    same(c, g, R.run(n, Q, ref_bases), REF_LENS, ref_bases)
    assert np.array_equal(g.cells_at(0, 0, REF_LENS[0]), G.packed(n[0], Q[0]))
    g.add(b"".join(recs[1000:]), offsets_of(recs[1000:]))
    same(c, g, want, REF_LENS, ref_bases)
    same(c, g, want, REF_LENS, ref_bases)                 # and once more on the same state
    # bmg_begin with other references, larger and then smaller, on the same bmr_ctx
    big = [300000, 70000, 5]
    big_bases = references(big, 9)
    check(c, g, random_records(2001, 31, big, big_bases), big, big_bases, exclude=[(0, 1000, 250000)])
    small, bases = edge_records(), edge_bases()
    check(c, g, small, EDGE_REFS, bases, bands=(50,), **STRICT)
    # a second cells context on the same bmr_ctx
    other = genotype.Genotype(0)
    try:
        check(c, other, recs[:300], REF_LENS, ref_bases)
    finally:
        other.close()


def test_argument_errors_leave_both_contexts_usable(c, g, ref_bases):
    from bucket_map_amd import genotype, refblocks
    recs = random_records(300, 8, bases=ref_bases)
    want = check(c, g, recs, REF_LENS, ref_bases)
    n_ref = len(REF_LENS)
    refusals = [
        dict(bands=list(range(1, 18))), dict(bands=[0, 5]), dict(bands=[5, 100]), dict(bands=[5, 5]), dict(bands=[9, 5]),
        dict(exclude=[(n_ref, 0, 1)]), dict(exclude=[(0, 5, 5)]), dict(exclude=[(0, 6, 5)]), dict(exclude=[(0, 0, 1), (1, 0, REF_LENS[1] + 1)]),
    ]
    for kw in refusals:
        with pytest.raises(refblocks.BmrError) as e:
            c.run(g, ref_bases, **kw)
        assert e.value.code == refblocks.BMR_ERR_ARG and "bmr_run" in str(e.value), kw
        assert c.blocks().tolist() == [list(b) for b in want[2]]          # the run before it is still there
    L = refblocks.lib()
    keep = [np.frombuffer(b, np.uint8) for b in ref_bases]
    ptrs = (C.c_void_p * n_ref)(*[a.ctypes.data for a in keep])
    holes = (C.c_void_p * n_ref)(*[a.ctypes.data if k != 2 else None for k, a in enumerate(keep)])
    count = C.c_uint64(0)
    one = np.array([5], np.uint32).ctypes.data_as(refblocks._u32p)
    for args in ((None, g._h, ptrs, None, 0, None, 0, C.byref(count)), (c._h, None, ptrs, None, 0, None, 0, C.byref(count)),
                 (c._h, g._h, None, None, 0, None, 0, C.byref(count)), (c._h, g._h, ptrs, None, 0, None, 0, None),
                 (c._h, g._h, ptrs, None, 1, None, 0, C.byref(count)), (c._h, g._h, ptrs, one, 1, None, 1, C.byref(count)),
                 (c._h, g._h, holes, one, 1, None, 0, C.byref(count))):
        assert L.bmr_run(*args) == refblocks.BMR_ERR_ARG, args
    fresh = genotype.Genotype(0)                          # no bmg_begin on the cells context
    try:
        with pytest.raises(refblocks.BmrError) as e:
            c.run(fresh, ref_bases)
        assert e.value.code == refblocks.BMR_ERR_ARG and "no bmg_begin" in str(e.value)
    finally:
        fresh.close()
    for call in (lambda: c.blocks(0, len(want[2]) + 1), lambda: c.blocks(len(want[2]) + 1, 0), lambda: c.conf_at(n_ref, 0, 1),
                 lambda: c.conf_at(0, REF_LENS[0], 1), lambda: c.conf_at(1, 1, REF_LENS[1])):
        with pytest.raises(refblocks.BmrError) as e:
            call()
        assert e.value.code == refblocks.BMR_ERR_ARG
    young = refblocks.RefBlocks(0)                        # bmr_blocks and bmr_conf_at before a bmr_run
    try:
        for call in (lambda: young.blocks(0, 0), lambda: young.conf_at(0, 0, 1)):
            with pytest.raises(refblocks.BmrError) as e:
                call()
            assert e.value.code == refblocks.BMR_ERR_ARG and "no bmr_run" in str(e.value)
        same(young, g, want, REF_LENS, ref_bases)         # both contexts still work
    finally:
        young.close()
    same(c, g, want, REF_LENS, ref_bases)
    assert np.array_equal(g.cells_at(1, 0, REF_LENS[1]), G.packed(*[x[1] for x in G.cells(recs, REF_LENS)]))
    assert c.run(g, ref_bases, (), ()) > 0                # n_bands == 0 and n_exclude == 0 succeed


# ---- the tools ----
@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_pileup import pileup_jobs
    return pileup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_gpu_tool_writes_the_oracle_tools_file(jobs, k):
    name, which, d, args, extra = jobs[k]
    for tag, opts, env in ((name, [], None), (name + "r", ["--vcf", f"{name}r.TOOL.vcf", "--gvcf-bands", "5,60"], dict(BM_SORT_RUN_BYTES="2000")),
                           (name + "m", ["--markdup", "--vcf-indels", "--affine", "--left-align", "--pileup-min-alt", "1", "--pileup-min-frac", "0.000001"], None)):
        if which != "bucketmap_align":
            opts = [o for o in opts if o not in ("--affine", "--left-align")]
        texts = {}
        for tool in ("oracle", "gpu"):
            mine = [o.replace("TOOL", tool) for o in opts]
            err = run(TOOLS[(which, tool)], d, args, f"{tag}.r{tool}.bam", [*extra, *mine, "--gvcf", f"{tag}.r{tool}.g.vcf"], env=env)
            texts[tool] = ((d / f"{tag}.r{tool}.g.vcf").read_text(), blocks_line(err))
            if "--vcf" in mine:
                texts[tool] += ((d / f"{tag}.{tool}.vcf").read_text(),)
        assert texts["gpu"] == texts["oracle"]
        assert texts["oracle"][0].startswith("##fileformat=VCFv4.2\n##source=bucketmap --gvcf\n") and "<NON_REF>" in texts["oracle"][0]
        assert pair_of(d, f"{tag}.rgpu") == pair_of(d, f"{tag}.roracle")
