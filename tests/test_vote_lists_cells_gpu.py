"""The cells form of the k-mer lists vote (bmf_vote_kernel_cells, forced with BMF_LISTS_CELLS = 2 or 3): every id is counted
into its cell of 4 or 8 consecutive buckets first, an item none of whose cells reaches t = S - F + 1 leaves, an item that
keeps up to 8 cells counts hits per bucket of those cells alone, and one that keeps more is handed to the full-width
kernel through the overflow list.  What only this form can get wrong: two buckets of one cell, buckets on either side of a
cell boundary, a cell that reaches t although none of its buckets does, the first and the last cell (a partial one; at
NB = 65 535 the padding id's), exactly 8 and 9 kept cells, an overflow count or list left behind by an earlier run, and
tails walked in both phases.  Every case compares counts, ids below the count and the number of rows the reference ANDs,
bit for bit: the oracle, the index rows (BMF_FLAG_PLAIN_ROWS), forced lists with BMF_LISTS_CELLS = 0, 2 and 3, each under
1, 2 and 4 waves per item.  What a case claims to hold is asserted on the host before the GPU is asked.  q = 4, k = 5."""
import numpy as np
import pytest

import test_kmer_lists_gpu as kl
import test_vote_lists_coop_gpu as coop
import test_vote_lists_extents_gpu as ext
import test_vote_lists_inflight_gpu as inflight
from conftest import assert_same_candidates

pytestmark = pytest.mark.gpu

Q, G, K, READ_LEN, NB = coop.Q, coop.G, coop.K, coop.READ_LEN, coop.NB
GOOD = inflight.GOOD
KEEP = 8                                 # kCellsKeep: cells an item may keep
CELLS = (0, 2, 3)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def env_of(cells, W):
    return {**kl.FORCE, "BMF_LISTS_CELLS": str(cells), "BMF_LISTS_ITEM_WAVES": str(W)}


def every_form(rows, k2i, windows, kw, served=True):
    """The oracle's (counts, buckets) and {(cells, W): overflow items of the run}, after checking the index rows and the
    forced lists under every form and every W against the oracle.  served: whether the cells form can serve these S, F."""
    import bucket_map_amd as bma
    what = f"NB={kw['num_buckets']} S={kw['num_samples']} F={kw['num_fault']}"
    c_ref, b_ref, n_ref = kl.oracle_run(rows, k2i, windows, **kw)
    plain = kl.new_filter(rows, k2i, **{**kw, "flags": bma.BMF_FLAG_PLAIN_ROWS})
    assert plain.info()["derived_form"] == "rows" and plain.info()["lists_cells"] == 0
    c_p, b_p, n_p = kl.run_batch(plain, windows)
    plain.close()
    assert_same_candidates(c_ref, b_ref, c_p, b_p, what + ", index rows")
    assert n_p == n_ref
    over = {}
    for cells in CELLS:
        for W in coop.WAVES:
            flt = kl.new_filter(rows, k2i, env=env_of(cells, W), **kw)
            info = flt.info()
            assert info["derived_form"] == "kmer_lists" and info["lists_item_waves"] == W
            assert info["lists_cells"] == (cells if served else 0), (what, cells, W)
            b = flt.batch(*windows)
            b.run()
            c_l, b_l = b.download()
            n_l, over[(cells, W)] = b.rows_anded(), b.lists_overflow()
            b.close()
            flt.close()
            assert_same_candidates(c_ref, b_ref, c_l, b_l, f"{what}, cells {cells}, {W} waves per item")
            assert n_l == n_ref, (what, cells, W)
            if not cells or not served:
                assert over[(cells, W)] == 0
    return c_ref, b_ref, over


def plant(bits, table):
    """the rows of the q-grams `table` names (under both numberings, ext.gram) hold exactly the buckets given"""
    for text, buckets in table.items():
        for g in ext.gram(text):
            bits[g] = False
            bits[g, list(buckets)] = True


def list_of(rows, k2i, nb, text):
    """the buckets of k-mer `text`, the same under both numberings"""
    got = [np.flatnonzero(np.unpackbits(kl.kmer_and(rows, k2i, nb, Q, G, x), bitorder="little")[:nb]).tolist() for x in ext.gram(text)]
    assert got[0] == got[1]
    return got[0]


def repeat_windows(repeats):
    """one full-length, good-quality window per entry of `repeats` ("" : a window shorter than k, rejected)"""
    body = [np.frombuffer(((r * READ_LEN)[:READ_LEN] if r else "AC").encode(), np.uint8) for r in repeats]
    lens = np.array([len(x) for x in body], np.uint32)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    bases = np.concatenate(body)
    return bases, np.full(len(bases), GOOD, np.uint8), off[:-1].copy(), lens


def kept_cells(ids, shift):
    return len({i >> shift for i in ids})


def base_index(rng, nb, table, density=0.004, clear=()):
    """sparse random rows, those of the four one-base q-grams empty unless `table` plants them"""
    bits = ext.sparse_bits(rng, nb, density=density, clear=clear)
    plant(bits, {**{x * Q: [] for x in "ACGT"}, **table})
    return ext.pack(bits)


def test_two_buckets_of_one_cell():
    """8 m + 2 and 8 m + 3 lie in one cell of 8 and in one cell of 4.  A window of A alone hits both S times: both come
    back.  A window of A with one C in it hits the second through every sample but those whose k-mer holds the C; the
    oracle, on an index without the first bucket, names the positions of the C at which exactly one sample does: there
    the second bucket has one hit fewer and only the first comes back."""
    rng = np.random.default_rng(20100)
    S, F = 15, 6
    a, b = 8 * 100 + 2, 8 * 100 + 3
    with_c = ["A" * i + "C" + "A" * (Q - 1 - i) for i in range(Q)]
    bits = ext.sparse_bits(rng, NB, clear=[a, b])
    plant(bits, {**{x * Q: [] for x in "CGT"}, "AAAA": [a, b], **{t: [a] for t in with_c}})
    rows, k2i = ext.pack(bits)
    only_b = bits.copy()
    only_b[:, a] = False
    rows_b, k2i_b = ext.pack(only_b)
    texts = ["A"] + ["A" * p + "C" + "A" * (READ_LEN - 1 - p) for p in range(READ_LEN)]
    windows = repeat_windows(texts)
    has_all = kl.oracle_run(rows_b, k2i_b, windows, **coop.params(NB, S, 1))[0][:, 0] > 0       # b has S hits
    has_but_one = kl.oracle_run(rows_b, k2i_b, windows, **coop.params(NB, S, 2))[0][:, 0] > 0   # ... at least S - 1
    one_fewer = np.flatnonzero(has_but_one & ~has_all)
    assert has_all[0] and len(one_fewer) >= 1, "no position of the C costs exactly one sample"
    c_ref, b_ref, _ = every_form(rows, k2i, windows, coop.params(NB, S, F))
    assert c_ref[0, 0] == 2 and b_ref[0, 0, :2].tolist() == [a, b]
    assert (c_ref[one_fewer, 0] == 1).all() and (b_ref[one_fewer, 0, 0] == a).all()


def test_buckets_on_either_side_of_a_cell_boundary():
    """8 m - 1 and 8 m: two cells of 8 and two of 4.  4 m - 1 and 4 m with m odd: two cells of 4 inside one cell of 8."""
    rng = np.random.default_rng(20200)
    pair8, pair4 = [8 * 50 - 1, 8 * 50], [4 * 151 - 1, 4 * 151]
    rows, k2i = base_index(rng, NB, {"AAAA": pair8, "CCCC": pair4}, clear=pair8 + pair4)
    assert kept_cells(pair8, 3) == 2 and kept_cells(pair8, 2) == 2 and kept_cells(pair4, 3) == 1 and kept_cells(pair4, 2) == 2
    assert list_of(rows, k2i, NB, "A" * K) == pair8 and list_of(rows, k2i, NB, "C" * K) == pair4
    windows = ext.with_windows(rng, 40, ["A", "C"])
    c_ref, b_ref, _ = every_form(rows, k2i, windows, coop.params(NB, 15, 6))
    assert b_ref[-2, 0, :c_ref[-2, 0]].tolist() == pair8 and b_ref[-1, 0, :c_ref[-1, 0]].tolist() == pair4


@pytest.mark.parametrize("S, F", [(15, 6), (31, 12)])
def test_a_cell_that_reaches_t_for_nothing(S, F):
    """The window repeats ACG: its three k-mers hold one bucket each, three different buckets of one cell (of 8 and of 4).
    Every sample adds one to the cell, whose sum is S >= t, and the oracle says that no bucket reaches t: the item is
    empty, and the exact phase is what finds that out."""
    rng = np.random.default_rng(20300 + S)
    x, y, z = 8 * 77 + 1, 8 * 77 + 2, 8 * 77 + 3
    bits = ext.sparse_bits(rng, NB, clear=[x, y, z])
    plant(bits, {"ACGA": [x, z], "CGAC": [x, y], "GACG": [y, z], "CGTC": [], "GTCG": [], "TCGT": []})
    rows, k2i = ext.pack(bits)
    lists = [list_of(rows, k2i, NB, t) for t in ("ACGAC", "CGACG", "GACGA")]
    assert sorted(sum(lists, [])) == [x, y, z] and all(len(l) == 1 for l in lists)          # one id each: the cell's sum is S
    assert kept_cells([x, y, z], 3) == 1 and kept_cells([x, y, z], 2) == 1 and S >= S - F + 1 >= 1
    windows = ext.with_windows(rng, 40, ["ACG"])
    c_ref, _, _ = every_form(rows, k2i, windows, coop.params(NB, S, F))
    assert c_ref[-1].tolist() == [0, 0], "a bucket reaches t: the samples are not spread over the three k-mers"


@pytest.mark.parametrize("nb", [NB, NB + 4, kl.NB_MAX])
def test_first_and_last_cell(nb):
    """Bucket 0 and bucket NB - 1.  NB mod 8 is 1 and 5: the last cell of 8 is partial, and so is the last cell of 4.
    NB = 65 535: the padding id's cell is the last one, and the padding ids of the list's last unit count in it."""
    rng = np.random.default_rng(20400 + nb % 97)
    assert nb % 8 in (1, 5, 7)
    ends = [0, nb - 1]
    rows, k2i = base_index(rng, nb, {"AAAA": ends, "CCCC": [nb - 2, nb - 1], "GGGG": [0]}, density=0.002, clear=[0, nb - 2, nb - 1])
    assert list_of(rows, k2i, nb, "A" * K) == ends
    windows = ext.with_windows(rng, 40, ["A", "C"])
    c_ref, b_ref, _ = every_form(rows, k2i, windows, coop.params(nb, 15, 6))
    assert b_ref[-2, 0, :c_ref[-2, 0]].tolist() == ends and b_ref[-1, 0, :c_ref[-1, 0]].tolist() == [nb - 2, nb - 1]
    assert b_ref[-1, 1, :c_ref[-1, 1]].tolist() == [0]


def test_overflow_a_list_of_every_bucket():
    """ext.test_a_kmer_with_no_indexed_qgram_holds_every_bucket's case (S = 15, F = 1): every cell reaches t, the item
    goes to the full-width kernel, and the answer is the planted 24."""
    rng = np.random.default_rng(20500)
    S, F = 15, 1
    planted = [0, 1, 2, 3] + list(range(1000, 1016)) + [NB - 4, NB - 3, NB - 2, NB - 1]
    bits = ext.sparse_bits(rng, NB, clear=planted)
    none = sorted(set(ext.gram("TGTT") + ext.gram("TTGT")))
    plant(bits, {"GTTG": planted})
    rows, k2i = ext.pack(bits, unindexed=none)
    assert len(list_of(rows, k2i, NB, "TTGTT")) == NB
    windows = ext.with_windows(rng, 40, ["AAC"])
    c_ref, b_ref, over = every_form(rows, k2i, windows, coop.params(NB, S, F))
    assert c_ref[-1, 1] == 24 and b_ref[-1, 1, :24].tolist() == planted
    assert all(over[(cells, W)] >= 1 for cells in (2, 3) for W in coop.WAVES)


def overflow_index(rng):
    """A: two buckets of neighbouring cells; T: one bucket in each of exactly KEEP cells; G: in KEEP + 1 cells; C: none."""
    lists = {"A": [8 * 30 - 1, 8 * 30], "T": [16 * i + 5 for i in range(KEEP)], "G": [16 * i + 1000 for i in range(KEEP + 1)], "C": []}
    rows, k2i = base_index(rng, NB, {x * Q: ids for x, ids in lists.items()}, clear=sum(lists.values(), []))
    for x, ids in lists.items():
        assert list_of(rows, k2i, NB, x * K) == ids
    for shift in (2, 3):
        assert kept_cells(lists["T"], shift) == KEEP and kept_cells(lists["G"], shift) == KEEP + 1
    return rows, k2i, lists


def host_overflow(repeats, lists):
    """items that keep more than KEEP cells: a one-base window's S samples are one k-mer, its reverse complement's the
    complement's, and every cell its list touches holds S >= t"""
    return sum((kept_cells(lists[r], 3) > KEEP) + (kept_cells(lists[COMP[r]], 3) > KEEP) for r in repeats if r)


def test_overflow_at_and_above_the_cells_an_item_may_keep():
    """Exactly KEEP kept cells: the cells kernel answers.  KEEP + 1: the overflow kernel does.  A batch that mixes both
    with voting, empty and rejected items: the reported overflow count is the host's."""
    rng = np.random.default_rng(20600)
    rows, k2i, lists = overflow_index(rng)
    repeats = ["A", "G", "", "C", "T", "G", "A", "", "C", "C", "T"] * 7
    windows = repeat_windows(repeats)
    c_ref, b_ref, over = every_form(rows, k2i, windows, coop.params(NB, 15, 6))
    for i, r in enumerate(repeats):
        want = [lists[r], lists[COMP[r]]] if r else [[], []]
        assert [b_ref[i, o, :c_ref[i, o]].tolist() for o in (0, 1)] == want, (i, r)
    n_over = host_overflow(repeats, lists)
    assert n_over == 5 * 7
    assert all(over[(cells, W)] == n_over for cells in (2, 3) for W in coop.WAVES), over


def test_more_ties_than_max_candidates():
    """31 ties in 31 cells: more than KEEP, the overflow kernel clears the item.  31 ties in consecutive buckets: 4 cells
    of 8 and 8 of 4, the cells kernel clears it itself."""
    rng = np.random.default_rng(20700)
    spread, run = [16 * i + 3 for i in range(31)], list(range(1200, 1231))
    rows, k2i = base_index(rng, NB, {"AAAA": spread, "CCCC": run}, clear=spread + run)
    assert kept_cells(spread, 3) == 31 and kept_cells(run, 3) == 4 and kept_cells(run, 2) == KEEP
    windows = repeat_windows(["A", "C", "A"])
    kw = coop.params(NB, 15, 6)
    assert len(spread) > kw["max_candidates"]
    c_ref, _, over = every_form(rows, k2i, windows, kw)
    assert not c_ref.any()
    assert all(over[(cells, W)] == 2 for cells in (2, 3) for W in coop.WAVES), over


@pytest.fixture(scope="module")
def big_small_big():
    rng = np.random.default_rng(20800)
    rows, k2i, lists = overflow_index(rng)
    big_r = ["G", "A", "C", "T", ""] * 60
    small_r = ["A", "", "T", "A"] * 8
    kw = coop.params(NB, 15, 6)
    big, small = repeat_windows(big_r), repeat_windows(small_r)
    want_big, want_small = kl.oracle_run(rows, k2i, big, **kw), kl.oracle_run(rows, k2i, small, **kw)
    assert host_overflow(big_r, lists) == 120 and host_overflow(small_r, lists) == 0
    return rows, k2i, kw, big, small, want_big, want_small


@pytest.mark.parametrize("cells", [2, 3])
def test_one_context_big_then_small_then_big(big_small_big, cells):
    """Overflow items in big only: the count and the list of the larger run must not reach the smaller one's, through the
    context's map slots or through one batch's buffers."""
    rows, k2i, kw, big, small, want_big, want_small = big_small_big
    for W in coop.WAVES:
        flt = kl.new_filter(rows, k2i, env=env_of(cells, W), **kw)
        assert flt.info()["lists_cells"] == cells
        for step, (windows, want) in enumerate(((big, want_big), (small, want_small), (big, want_big), (small, want_small))):
            c, b = flt.map_windows(*windows)
            assert_same_candidates(want[0], want[1], c, b, f"cells {cells}, {W} waves per item, step {step}")
        for windows, want, n_over in ((big, want_big, 120), (small, want_small, 0)):
            batch = flt.batch(*windows)
            for again in range(2):
                batch.run()
                c, b = batch.download()
                assert_same_candidates(want[0], want[1], c, b, f"cells {cells}, {W} waves per item, batch run {again}")
                assert batch.lists_overflow() == n_over
            batch.close()
        flt.close()


@pytest.mark.parametrize("piece", ["64", "97", "100000"])
def test_host_buffer_entry_points_in_pieces(big_small_big, piece, monkeypatch):
    """BMF_PIECE_WINDOWS: every piece is a launch of its own with its own overflow list; big holds overflow items in
    every piece of 64 and of 97 windows."""
    rows, k2i, kw, big, small, want_big, want_small = big_small_big
    for cells in (2, 3):
        for W in coop.WAVES:
            flt = kl.new_filter(rows, k2i, env=env_of(cells, W), **kw)
            monkeypatch.setenv("BMF_PIECE_WINDOWS", piece)
            for windows, (c_ref, b_ref, _) in ((big, want_big), (small, want_small)):
                mask = np.arange(b_ref.shape[-1])[None, None, :] < c_ref[:, :, None]
                c, ids = flt.map_windows_compact(*windows)
                assert np.array_equal(c, c_ref) and np.array_equal(ids, b_ref[mask]), (cells, W, piece, len(windows[2]))
            monkeypatch.delenv("BMF_PIECE_WINDOWS")
            flt.close()


def test_rejected_windows_beside_accepted_ones():
    rng = np.random.default_rng(20900)
    rows, k2i, windows, kw, kind = inflight.cycle_case(rng, 100)
    assert (windows[3][kind == 1] < K).all() and (windows[3][kind != 1] == READ_LEN).all()
    c_ref, _, _ = every_form(rows, k2i, windows, {**kw, "num_fault": 6})
    assert not c_ref[kind == 1].any() and (c_ref[kind == 0, 0] == 1).all()


@pytest.mark.parametrize("S, F, served", [(1, 1, True), (15, 6, True), (16, 6, True), (31, 12, True), (32, 12, False), (64, 26, False)])
def test_samples(S, F, served):
    """S = 16: two batches of heads for one wave; S = 31: the most the byte fields of a cell of 8 hold (248).  S = 32 and
    64 run on the full-width kernel although the cells are forced."""
    rng = np.random.default_rng(21000 + S)
    rows, k2i = kl.mixed_index(rng, NB, Q, G, 1.0)
    windows = kl.random_windows(rng, 100, READ_LEN, K)
    c_ref, _, _ = every_form(rows, k2i, windows, coop.params(NB, S, F), served=served)
    assert (c_ref > 0).any()


def test_tails_in_both_phases():
    """NB = 65 535.  The window repeats ACG; one of its three k-mers holds 656 buckets, 82 units, the planted one beyond
    the 64th, the other two hold the planted bucket alone.  With F = 1 only the planted bucket's cell reaches t = S (the
    long list's other ids lie 100 apart and are met by fewer than S samples -- the oracle's answer says so): the cell
    phase and the exact phase both walk the tail."""
    rng = np.random.default_rng(21100)
    nb, S, F = kl.NB_MAX, 15, 1
    dense, p = list(range(50, nb - 100, 100)), 65001
    bits = ext.sparse_bits(rng, nb, density=0.001, clear=dense + [p])
    plant(bits, {"ACGA": dense + [p], "CGAC": dense + [p], "GACG": [p], "CGTC": [], "GTCG": [], "TCGT": []})
    rows, k2i = ext.pack(bits)
    long_list = list_of(rows, k2i, nb, "ACGAC")
    assert long_list == sorted(dense + [p]) and long_list.index(p) >= 8 * 64 and len(long_list) > 8 * 64
    assert list_of(rows, k2i, nb, "CGACG") == [p] and list_of(rows, k2i, nb, "GACGA") == [p]
    windows = ext.with_windows(rng, 20, ["ACG"])
    c_ref, b_ref, _ = every_form(rows, k2i, windows, coop.params(nb, S, F))
    assert c_ref[-1, 0] == 1 and b_ref[-1, 0, 0] == p
