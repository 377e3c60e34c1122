"""bmf_vote_kernel_lists with its lists split in two phases: the first S - F lists of an item are counted with plain LDS
adds (no return, no fold), a fence, then the other F lists with returning adds, whose returns alone make the item's
highest hit count.  That is exact as long as at most S - F lists are plain and no plain add lands after a returning one
(bmf_kmer_lists.hip.h), and it can only go wrong where the best count is S - F + 1 (its last increment must be a
returning one) or S - F (the item must stay empty), where the boundary falls inside, on or next to a 16-list batch, where
plain and returning lists both have tails beyond their first 64 units, where plain and returning adds meet in one counter
dword, and where the padding id of a plain list has its dword inside the counters.  Every case compares counts, bucket
ids and the number of rows the reference ANDs, bit for bit, three ways: forced lists, the index rows
(BMF_FLAG_PLAIN_ROWS) and the oracle.  q = 4, k = 5 throughout: a few MB of lists."""
import numpy as np
import pytest

import test_kmer_lists_gpu as kl
import test_vote_lists_inflight_gpu as inflight

pytestmark = pytest.mark.gpu

Q, G = 4, 2
K = Q + G - 1
READ_LEN = 80
NB = 2049


def params(nb, S, F):
    return {**kl.params(nb, Q, K, S), "num_fault": F}


def voting(rows, k2i, windows, kw, F):
    """Per (window, orientation): does the oracle keep a candidate with num_fault = F"""
    c, _, _ = kl.oracle_run(rows, k2i, windows, **{**kw, "num_fault": F})
    return c > 0


# S = 15 (4-bit counters): 14, 13, 9, 1, 0, 0 plain lists; S = 16 (8-bit): 15, 10, 1, 0; S = 64: the boundary at list
# 63, 49, 48, 47 and 33 -- inside a 16-list batch, on one, and next to one
F_SWEEP = [(15, F) for F in (1, 2, 6, 14, 15, 20)] + [(16, F) for F in (1, 6, 15, 16)] + [(64, F) for F in (1, 15, 16, 17, 31)]


@pytest.mark.parametrize("S, F", F_SWEEP)
def test_every_position_of_the_phase_boundary(S, F):
    rng = np.random.default_rng(9100 + 100 * S + F)
    rows, k2i = kl.mixed_index(rng, NB, Q, G, 1.0)
    windows = kl.random_windows(rng, 200, READ_LEN, K)
    inflight.three_ways(rows, k2i, windows, params(NB, S, F))


@pytest.mark.parametrize("S, F, density", [(15, 1, 0.6), (15, 2, 0.6), (15, 6, 0.4), (16, 1, 0.6), (16, 6, 0.4),
                                           (64, 1, 0.8), (64, 15, 0.6), (64, 16, 0.6), (64, 17, 0.6)])
def test_items_at_and_just_below_the_threshold(S, F, density):
    """An item votes at F and not at F - 1 iff its best count is exactly S - F + 1: its last increment is a returning
    add.  It votes at F + 1 and not at F iff its best count is exactly S - F: the returning adds report at most that,
    and it stays empty.  The oracle alone says the batch holds both kinds before the kernel is asked."""
    rng = np.random.default_rng(9200 + 100 * S + F)
    rows, k2i = kl.random_index(rng, NB, Q, 1.0, density)
    windows = kl.random_windows(rng, 200, READ_LEN, K)
    kw = params(NB, S, F)
    assert kw["max_candidates"] == 30
    at_f = voting(rows, k2i, windows, kw, F)
    at_threshold = at_f & ~voting(rows, k2i, windows, kw, F - 1) if F > 1 else at_f
    just_below = ~at_f & voting(rows, k2i, windows, kw, F + 1)
    print(f"S={S} F={F}: {int(at_threshold.sum())} items at the threshold, {int(just_below.sum())} just below it")
    assert at_threshold.sum() >= 5
    assert just_below.sum() >= 5
    inflight.three_ways(rows, k2i, windows, kw)


@pytest.mark.parametrize("nb", [NB, 128 * 64 + 5])
@pytest.mark.parametrize("S, F", [(15, 1), (15, 6), (15, 14), (64, 16), (64, 31)])
def test_long_lists_on_both_sides_of_the_fence(S, F, nb):
    """A quarter of the q-grams indexed: more than half of the k-mers have none and hold all NB ids, 257 and 1 025
    units, so tails beyond the first 64 units occur in the plain lists and in the returning ones (F = 1: nearly all of
    them plain, F = 14: nearly all returning)."""
    rng = np.random.default_rng(9300 + 100 * S + F + nb % 97)
    rows, k2i = kl.mixed_index(rng, nb, Q, G, 0.25)
    windows = kl.random_windows(rng, 120 if S < 64 else 60, READ_LEN, K)
    c_ref, _ = inflight.three_ways(rows, k2i, windows, params(nb, S, F))
    assert (c_ref > 0).any()


@pytest.mark.parametrize("F", [2, 6])
@pytest.mark.parametrize("S", [15, 16, 64])
def test_plain_and_returning_adds_on_shared_dwords(S, F):
    """Runs of 24 consecutive ids: one counter dword takes plain adds from one lane and returning adds from others."""
    rng = np.random.default_rng(9400 + 100 * S + F)
    rows, k2i = inflight.run_index(rng, NB, Q)
    windows = kl.random_windows(rng, 200, READ_LEN, K)
    c_ref, _ = inflight.three_ways(rows, k2i, windows, params(NB, S, F))
    assert (c_ref > 0).any()


@pytest.mark.parametrize("F", [1, 6])
@pytest.mark.parametrize("nb, S", [(100, 15), (100, 16), (kl.NB_MAX, 15), (kl.NB_MAX, 16)])
def test_edges_of_the_counter_array_under_the_split(nb, S, F):
    """NB = 100: fewer 16-byte groups of counters than lanes, the plain padding adds land in the staging area.
    NB = 65 535: the padding id's dword lies inside the counters, and plain padding adds carry out of its top field."""
    rng = np.random.default_rng(9500 + 100 * S + F + nb % 89)
    rows, k2i = kl.mixed_index(rng, nb, Q, G, 1.0)
    windows = kl.random_windows(rng, 60, READ_LEN, K)
    inflight.three_ways(rows, k2i, windows, params(nb, S, F))
