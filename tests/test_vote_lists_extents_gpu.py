"""The list entries of the k-mer lists vote are list EXTENTS: the sample kernel reads offsets[x] and offsets[x + 1] of the
sampled k-mer x and hands bmf_vote_kernel_lists the first unit and the unit count of its list in one 64-bit entry, and the
vote kernel loads its item's entries together with list_n, before it knows whether the window was rejected.  What only
this form can get wrong: the two ends of the offsets table, the longest list there is (all NB ids) and the shortest (no
unit), the lane that holds the last of 64 entries, entries of a rejected window that were never written or that an
earlier, larger batch left behind, and the pieces of the host-buffer entry points.  Every case compares counts, ids below
the count and the number of rows the reference ANDs, bit for bit, three ways (test_vote_lists_coop_gpu.every_w): the
oracle, the index rows (BMF_FLAG_PLAIN_ROWS), forced lists under 1, 2 and 4 waves per item.  What a batch claims to hold is
asserted on the host before the GPU is asked.  q = 4, k = 5 throughout."""
import numpy as np
import pytest

import test_kmer_lists_gpu as kl
import test_vote_lists_coop_gpu as coop
import test_vote_lists_inflight_gpu as inflight

pytestmark = pytest.mark.gpu

Q, G, K, READ_LEN, NB = coop.Q, coop.G, coop.K, coop.READ_LEN, coop.NB
GOOD = inflight.GOOD
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def gram(text):
    """The two numbers a q-gram may have, its first base in the high or in the low bits: the indexes below treat both alike,
    so no case depends on which the library uses (as in inflight.cycle_case)."""
    hi = sum(CODE[c] << (2 * (len(text) - 1 - j)) for j, c in enumerate(text))
    lo = sum(CODE[c] << (2 * j) for j, c in enumerate(text))
    return hi, lo


def grams_of(repeat):
    """the q-grams of the endless repetition of `repeat`, each under both numberings"""
    text = repeat * (Q + len(repeat))
    return sorted({g for i in range(len(repeat)) for g in gram(text[i: i + Q])})


def with_windows(rng, n_random, repeats):
    """n_random windows of kl.random_windows, then one full-length, good-quality window per entry of `repeats`"""
    bases, quals, off, lens = kl.random_windows(rng, n_random, READ_LEN, K)
    extra = [np.frombuffer((r * READ_LEN)[:READ_LEN].encode(), np.uint8) for r in repeats]
    at = int(off[-1]) + int(lens[-1]) if len(off) else 0
    off = np.concatenate([off, at + READ_LEN * np.arange(len(extra), dtype=np.uint64)]).astype(np.uint64)
    lens = np.concatenate([lens, np.full(len(extra), READ_LEN, np.uint32)]).astype(np.uint32)
    return (np.concatenate([bases] + extra), np.concatenate([quals, np.full(READ_LEN * len(extra), GOOD, np.uint8)]), off, lens)


def sparse_bits(rng, nb, density=0.004, clear=()):
    bits = rng.random((4 ** Q, nb)) < density
    for b in clear:
        bits[:, b] = False
    return bits


def pack(bits, unindexed=()):
    """(rows, k2i): the q-grams of `unindexed` have no row"""
    kept = np.ones(len(bits), bool)
    kept[list(unindexed)] = False
    k2i = np.full(len(bits), -1, np.int32)
    k2i[kept] = np.arange(int(kept.sum()))
    return np.packbits(bits[kept], axis=1, bitorder="little"), k2i


@pytest.mark.parametrize("S", [1, 15, 16, 64])
def test_first_and_last_entry_of_the_offsets_table(S):
    """A window of A alone samples k-mer 0 S times, and its reverse complement is k-mer 4^k - 1: offsets[0], offsets[1] and
    offsets[4^k - 1], offsets[4^k].  A window of T alone does the same the other way round.  Both lists are planted: 24
    buckets of AAAA's row at the low end, 9 of TTTT's at the high end, NB - 1 among them.  S = 64: lane 63 of a one-wave item
    holds an entry, lane 15 of a four-wave one; S = 1: three of four waves hold none."""
    rng = np.random.default_rng(13100 + S)
    low, high = list(range(3, 27)), list(range(NB - 9, NB))
    bits = sparse_bits(rng, NB)
    for g in gram("AAAA"):
        bits[g] = False
        bits[g, low] = True
    for g in gram("TTTT"):
        bits[g] = False
        bits[g, high] = True
    rows, k2i = pack(bits)
    assert gram("A" * K) == (0, 0) and gram("T" * K) == (4 ** K - 1, 4 ** K - 1)
    for x, want in ((0, low), (4 ** K - 1, high)):
        assert np.flatnonzero(np.unpackbits(kl.kmer_and(rows, k2i, NB, Q, G, x), bitorder="little")[:NB]).tolist() == want
    windows = with_windows(rng, 60, ["A", "T"])
    F = 1 if S == 1 else (26 if S == 64 else 6)
    c_ref, b_ref = coop.every_w(rows, k2i, windows, coop.params(NB, S, F))
    assert c_ref[-2].tolist() == [24, 9] and c_ref[-1].tolist() == [9, 24]
    assert b_ref[-2, 0, :24].tolist() == low and b_ref[-2, 1, :9].tolist() == high


@pytest.mark.parametrize("nb", [NB, kl.NB_MAX])
def test_a_kmer_with_no_indexed_qgram_holds_every_bucket(nb):
    """The longest list: all NB ids, 257 units and, at NB = 65 535, 8 192 -- the largest unit count an entry must hold.
    The window repeats AAC; its reverse complement repeats GTT, whose q-grams are TGTT, TTGT and GTTG.  The first two are
    not indexed, so the k-mer TTGTT has no indexed q-gram and its list holds every bucket, while GTTGT and TGTTG have the
    planted row of GTTG, 24 buckets with 0 and NB - 1 among them.  With F = 1 a bucket needs all S hits: the planted ones
    have them only if every id of the all-buckets lists is counted, the last of the last unit included.
    That the S samples do meet TTGTT is the oracle's word: with an EMPTY row for TGTT and TTGT, instead of none, the item is
    empty."""
    rng = np.random.default_rng(13200 + nb % 97)
    S, F = 15, 1
    planted = [0, 1, 2, 3] + list(range(1000, 1016)) + [nb - 4, nb - 3, nb - 2, nb - 1]
    bits = sparse_bits(rng, nb, clear=planted)
    none = sorted(set(gram("TGTT") + gram("TTGT")))
    assert not set(none) & set(grams_of("AAC")) and not set(none) & set(gram("GTTG"))
    for g in gram("GTTG"):
        bits[g] = False
        bits[g, planted] = True
    rows, k2i = pack(bits, unindexed=none)
    windows = with_windows(rng, 40, ["AAC"])
    kw = coop.params(nb, S, F)
    # on the host: the k-mer has all NB buckets, the oracle keeps the planted ones, and not with an empty row in its place
    for x in gram("TTGTT"):
        assert int(np.unpackbits(kl.kmer_and(rows, k2i, nb, Q, G, x), bitorder="little")[:nb].sum()) == nb
    emptied = bits.copy()
    emptied[none] = False
    c_emptied, _, _ = kl.oracle_run(*pack(emptied), windows, **kw)
    assert c_emptied[-1, 1] == 0, "no sample of the window is the k-mer without an indexed q-gram"
    c_ref, b_ref = coop.every_w(rows, k2i, windows, kw)
    assert c_ref[-1, 1] == 24 and b_ref[-1, 1, :24].tolist() == planted


def test_a_kmer_whose_and_is_empty_has_no_unit():
    """The shortest list: offsets[x + 1] == offsets[x].  The window repeats AAC: its k-mers are AACAA (q-grams AACA and
    ACAA, both with the 24 planted buckets), ACAAC and CAACA (each holds CAAC, whose row shares no bucket with the other
    two).  Two of three lists are empty; with F = 13 the planted buckets need three hits of fifteen samples.  Units read
    for an empty list would be those of the next k-mer's."""
    rng = np.random.default_rng(13300)
    S, F = 15, 13
    planted, other = list(range(40, 64)), list(range(1500, 1520))
    bits = sparse_bits(rng, NB)
    for text, buckets in (("AACA", planted), ("ACAA", planted), ("CAAC", other)):
        for g in gram(text):
            bits[g] = False
            bits[g, buckets] = True
    rows, k2i = pack(bits)
    for text in ("ACAAC", "CAACA"):
        for x in gram(text):
            assert not kl.kmer_and(rows, k2i, NB, Q, G, x).any(), text
    windows = with_windows(rng, 40, ["AAC"])
    c_ref, b_ref = coop.every_w(rows, k2i, windows, coop.params(NB, S, F))
    assert c_ref[-1, 0] == 24 and b_ref[-1, 0, :24].tolist() == planted


@pytest.mark.parametrize("S", [15, 64])
def test_rejected_windows_beside_accepted_ones(S):
    """inflight.cycle_case: every fifth window is shorter than k, so its entries are never written (a fresh batch) while
    its neighbours' are; the vote kernel loads them all the same and must leave at list_n == 0."""
    rng = np.random.default_rng(13400 + S)
    rows, k2i, windows, kw, kind = inflight.cycle_case(rng, 100, S=S)
    assert (windows[3][kind == 1] < K).all() and (windows[3][kind != 1] == READ_LEN).all()
    c_ref, _ = coop.every_w(rows, k2i, windows, {**kw, "num_fault": 26 if S == 64 else 6})
    assert not c_ref[kind == 1].any() and (c_ref[kind == 0, 0] == 1).all()


@pytest.fixture(scope="module")
def big_then_small():
    """(rows, k2i, kw, big, small, the oracle's answers): big is 400 full-length windows that all vote; small is its first
    40 with every second one cut below k, so that in a buffer big has been through, the entries of a rejected window of
    small are those of an accepted window of big."""
    rng = np.random.default_rng(13500)
    rows, k2i = kl.mixed_index(rng, NB, Q, G, 1.0)
    n = 400
    lens = np.full(n, READ_LEN, np.uint32)
    off = (READ_LEN * np.arange(n)).astype(np.uint64)
    big = (kl.LETTERS[rng.integers(0, 4, n * READ_LEN)], np.full(n * READ_LEN, GOOD, np.uint8), off, lens)
    small_lens = lens[:40].copy()
    small_lens[::2] = K - 1
    small = (big[0], big[1], off[:40].copy(), small_lens)
    kw = coop.params(NB, 15, 6)
    want_big, want_small = kl.oracle_run(rows, k2i, big, **kw), kl.oracle_run(rows, k2i, small, **kw)
    assert (want_big[0][:40] > 0).any(axis=1).all(), "a window of big's first 40 does not vote"
    assert not want_small[0][::2].any() and np.array_equal(want_small[0][1::2], want_big[0][1:40:2])
    return rows, k2i, kw, big, small, want_big, want_small


@pytest.mark.parametrize("W", coop.WAVES)
def test_stale_extents_beside_list_n_zero(big_then_small, W):
    """One context, one batch object run on big and a smaller batch through the context's map slots after big."""
    from conftest import assert_same_candidates
    rows, k2i, kw, big, small, want_big, want_small = big_then_small
    flt = kl.new_filter(rows, k2i, env={**kl.FORCE, "BMF_LISTS_ITEM_WAVES": str(W)}, **kw)
    assert flt.info()["derived_form"] == "kmer_lists" and flt.info()["lists_item_waves"] == W
    for step, (windows, want) in enumerate(((big, want_big), (small, want_small), (big, want_big), (small, want_small))):
        c, b = flt.map_windows(*windows)
        assert_same_candidates(want[0], want[1], c, b, f"{W} waves per item, step {step}")
    flt.close()


@pytest.mark.parametrize("piece", ["64", "97", "100000"])
def test_host_buffer_entry_points_in_pieces(big_then_small, piece, monkeypatch):
    """BMF_PIECE_WINDOWS: every piece is a launch of its own on its own slot's entries; big, then small on the same slots."""
    rows, k2i, kw, big, small, want_big, want_small = big_then_small
    for W in coop.WAVES:
        flt = kl.new_filter(rows, k2i, env={**kl.FORCE, "BMF_LISTS_ITEM_WAVES": str(W)}, **kw)
        monkeypatch.setenv("BMF_PIECE_WINDOWS", piece)
        for windows, (c_ref, b_ref, _) in ((big, want_big), (small, want_small)):
            mask = np.arange(b_ref.shape[-1])[None, None, :] < c_ref[:, :, None]
            c, ids = flt.map_windows_compact(*windows)
            assert np.array_equal(c, c_ref) and np.array_equal(ids, b_ref[mask]), (W, piece, len(windows[2]))
        flt.close()
