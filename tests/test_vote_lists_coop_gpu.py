"""bmf_vote_kernel_lists with W waves of one workgroup sharing the hit counters of one item (W = 1, 2 or 4, forced with
BMF_LISTS_ITEM_WAVES): wave w counts the lists s = w (mod W), the plain ones of every wave before a workgroup barrier and
the returning ones after it, the waves' maxima and match counts meet in LDS, and each wave scans and emits a contiguous
range of the counters.  Only this form can go wrong where a wave has no list or no plain or no returning list, where the
last increment of a counter comes from another wave than the plain ones, where plain adds of one wave and returning adds
of another meet in one dword, where tails are walked by several waves on both sides of the barrier, where ties at the
maximum lie in the ranges of several waves, and where whole waves have nothing to zero or scan.  Every case compares
counts, ids below the count and the number of rows the reference ANDs, bit for bit: the oracle, the index rows
(BMF_FLAG_PLAIN_ROWS), then forced lists under every W.  q = 4, k = 5 throughout: a few MB of lists."""
import numpy as np
import pytest

import test_kmer_lists_gpu as kl
import test_vote_lists_inflight_gpu as inflight
from conftest import assert_same_candidates

pytestmark = pytest.mark.gpu

Q, G = 4, 2
K = Q + G - 1
READ_LEN = 80
NB = 2049
WAVES = (1, 2, 4)


def params(nb, S, F, **more):
    return {**kl.params(nb, Q, K, S), "num_fault": F, **more}


def every_w(rows, k2i, windows, kw):
    """The oracle's (counts, buckets) after checking the index rows and, under every W, the forced lists against it."""
    import bucket_map_amd as bma
    what = f"NB={kw['num_buckets']} S={kw['num_samples']} F={kw['num_fault']} max_candidates={kw['max_candidates']}"
    c_ref, b_ref, n_ref = kl.oracle_run(rows, k2i, windows, **kw)
    plain = kl.new_filter(rows, k2i, **{**kw, "flags": bma.BMF_FLAG_PLAIN_ROWS})
    assert plain.info()["derived_form"] == "rows" and plain.info()["lists_item_waves"] == 0
    c_p, b_p, n_p = kl.run_batch(plain, windows)
    plain.close()
    assert_same_candidates(c_ref, b_ref, c_p, b_p, what + ", index rows")
    assert n_p == n_ref
    for W in WAVES:
        lists = kl.new_filter(rows, k2i, env={**kl.FORCE, "BMF_LISTS_ITEM_WAVES": str(W)}, **kw)
        assert lists.info()["derived_form"] == "kmer_lists"
        assert lists.info()["lists_item_waves"] == W
        c_l, b_l, n_l = kl.run_batch(lists, windows)
        lists.close()
        assert_same_candidates(c_ref, b_ref, c_l, b_l, f"{what}, lists, {W} waves per item")
        assert n_l == n_ref, (what, W)
    return c_ref, b_ref


def voting(rows, k2i, windows, kw, F):
    """Per (window, orientation): does the oracle keep a candidate with num_fault = F"""
    c, _, _ = kl.oracle_run(rows, k2i, windows, **{**kw, "num_fault": F})
    return c > 0


@pytest.mark.parametrize("S", [1, 2, 3, 5, 15, 16, 17, 64])
def test_samples_against_waves(S):
    """S < W: waves with no list; S = 3, 5, 15, 17: uneven shares; S = 64: a share needs further batches of heads.
    F = 1 for S = 1 (the one list is the returning one), else the default of the other files."""
    rng = np.random.default_rng(12100 + S)
    rows, k2i = kl.mixed_index(rng, NB, Q, G, 1.0)
    windows = kl.random_windows(rng, 120, READ_LEN, K)
    F = 26 if S == 64 else max(1, min(6, S - 1))
    c_ref, _ = every_w(rows, k2i, windows, params(NB, S, F))
    assert (c_ref > 0).any()


# the existing sweep, then: some waves with no plain list at all -- (15, 13): 2 plain lists, (15, 14) and (16, 15): 1 --
# and some with no returning list at all -- (15, 1), (15, 2), (64, 1): 1, 2 and 1 returning lists
BOUNDARY = sorted(set([(15, F) for F in (1, 2, 6, 14, 15, 20)] + [(16, F) for F in (1, 6, 15, 16)] +
                      [(64, F) for F in (1, 15, 16, 17, 31)] + [(15, 13), (15, 14), (16, 15), (15, 1), (15, 2), (64, 1)]))


@pytest.mark.parametrize("S, F", BOUNDARY)
def test_phase_boundary_inside_and_between_shares(S, F):
    rng = np.random.default_rng(12200 + 100 * S + F)
    rows, k2i = kl.mixed_index(rng, NB, Q, G, 1.0)
    windows = kl.random_windows(rng, 100, READ_LEN, K)
    every_w(rows, k2i, windows, params(NB, S, F))


@pytest.mark.parametrize("S, F, density", [(15, 1, 0.6), (15, 2, 0.6), (15, 6, 0.4), (16, 1, 0.6), (16, 6, 0.4),
                                           (64, 1, 0.8), (64, 15, 0.6), (64, 16, 0.6), (64, 17, 0.6)])
def test_items_at_and_just_below_the_threshold(S, F, density):
    """Best count exactly S - F + 1: the last increment is a returning add, now perhaps of another wave than the plain
    ones.  Best count exactly S - F: the item stays empty.  The oracle alone says the batch holds both kinds."""
    rng = np.random.default_rng(12300 + 100 * S + F)
    rows, k2i = kl.random_index(rng, NB, Q, 1.0, density)
    windows = kl.random_windows(rng, 200, READ_LEN, K)
    kw = params(NB, S, F)
    at_f = voting(rows, k2i, windows, kw, F)
    at_threshold = at_f & ~voting(rows, k2i, windows, kw, F - 1) if F > 1 else at_f
    just_below = ~at_f & voting(rows, k2i, windows, kw, F + 1)
    print(f"S={S} F={F}: {int(at_threshold.sum())} items at the threshold, {int(just_below.sum())} just below it")
    assert at_threshold.sum() >= 5
    assert just_below.sum() >= 5
    every_w(rows, k2i, windows, kw)


@pytest.mark.parametrize("F", [2, 6])
@pytest.mark.parametrize("S", [15, 16, 64])
def test_one_dword_several_waves(S, F):
    """Runs of 24 consecutive ids: plain adds from one wave and returning adds from another meet in one counter dword."""
    rng = np.random.default_rng(12400 + 100 * S + F)
    rows, k2i = inflight.run_index(rng, NB, Q)
    windows = kl.random_windows(rng, 150, READ_LEN, K)
    c_ref, _ = every_w(rows, k2i, windows, params(NB, S, F))
    assert (c_ref > 0).any()


@pytest.mark.parametrize("nb", [NB, 128 * 64 + 5])
@pytest.mark.parametrize("S, F", [(15, 1), (15, 6), (15, 14), (64, 16)])
def test_tails_in_different_waves_on_both_sides_of_the_barrier(S, F, nb):
    """A quarter of the q-grams indexed: more than half of the k-mers hold all NB ids (257 and 1 025 units), so every
    wave walks tails, of plain lists before the phase barrier and of returning ones after it."""
    rng = np.random.default_rng(12500 + 100 * S + F + nb % 97)
    rows, k2i = kl.mixed_index(rng, nb, Q, G, 0.25)
    windows = kl.random_windows(rng, 100 if S < 64 else 60, READ_LEN, K)
    c_ref, _ = every_w(rows, k2i, windows, params(nb, S, F))
    assert (c_ref > 0).any()


def tie_index(rng):
    """Bucket columns in classes of identical columns, so that the buckets of a class always tie: 250 pairs (b, b + 1 024),
    one id on either side of NB / 2; 30 classes of 32 buckets, 16 in either half, more ties than max_candidates = 30
    allows; the other buckets on their own.  Rows at 0.6: an item's best count is met by a few classes."""
    n = 4 ** Q
    bits = rng.random((n, NB)) < 0.6
    bits[:, 1024 + 10: 1024 + 260] = bits[:, 10: 260]
    for g in range(30):
        col = bits[:, 300 + 16 * g].copy()
        bits[:, 300 + 16 * g: 316 + 16 * g] = col[:, None]
        bits[:, 1324 + 16 * g: 1340 + 16 * g] = col[:, None]
    return np.packbits(bits, axis=1, bitorder="little"), np.arange(n, dtype=np.int32)


@pytest.fixture(scope="module")
def tie_case():
    """(rows, k2i, windows) of the first index drawn on which the oracle alone shows, for each max_candidates, at least 5
    cleared items and -- where a kept item can hold two ids at all, max_candidates >= 2 -- at least 5 kept with two or
    more ids and 5 kept with ids on both sides of NB / 2."""
    rng = np.random.default_rng(12600)
    for _ in range(8):
        rows, k2i = tie_index(rng)
        windows = kl.random_windows(rng, 200, READ_LEN, K)
        c_wide, _, _ = kl.oracle_run(rows, k2i, windows, **params(NB, 15, 6, max_candidates=100))
        kinds = {}
        for mc in (1, 2, 30):
            c, b, _ = kl.oracle_run(rows, k2i, windows, **params(NB, 15, 6, max_candidates=mc))
            live = np.arange(b.shape[-1])[None, None, :] < c[:, :, None]
            low = (live & (b < NB // 2)).any(axis=-1)
            high = (live & (b >= NB // 2)).any(axis=-1)
            kinds[mc] = (int(((c == 0) & (c_wide > mc)).sum()), int((c >= 2).sum()), int((low & high).sum()))
        print("cleared / kept with two ids or more / kept on both sides of NB/2, per max_candidates:", kinds)
        if all(kinds[mc][0] >= 5 for mc in kinds) and all(min(kinds[mc][1:]) >= 5 for mc in (2, 30)):
            return rows, k2i, windows, kinds
    pytest.fail(f"no index with 5 items of every kind in 8 draws: {kinds}")


@pytest.mark.parametrize("max_candidates", [1, 2, 30])
def test_ties_across_the_scan_split(tie_case, max_candidates):
    """Ties at the maximum in the counter ranges of several waves: the ids come out in ascending order whichever wave
    found them, and the item is cleared iff the waves' matches together exceed max_candidates.  (With max_candidates = 1
    a kept item holds one id: only the cleared kind exists there.)"""
    rows, k2i, windows, kinds = tie_case
    assert kinds[max_candidates][0] >= 5
    assert max_candidates == 1 or min(kinds[max_candidates][1:]) >= 5
    every_w(rows, k2i, windows, params(NB, 15, 6, max_candidates=max_candidates))


@pytest.mark.parametrize("nb, S", [(100, 15), (100, 16), (kl.NB_MAX, 15), (kl.NB_MAX, 16)])
def test_edges_of_the_counter_array(nb, S):
    """NB = 100: 4 (7 in the 8-bit form) 16-byte groups of counters: whole waves have nothing to zero or scan.
    NB = 65 535: the padding id's dword lies inside the counters, 32 KB and 64 KB of LDS per workgroup."""
    rng = np.random.default_rng(12700 + nb % 89 + S)
    rows, k2i = kl.mixed_index(rng, nb, Q, G, 1.0)
    windows = kl.random_windows(rng, 60, READ_LEN, K)
    c_ref, _ = every_w(rows, k2i, windows, params(nb, S, 6))
    assert (c_ref > 0).any()


def test_rejected_windows_next_to_voting_ones():
    """The five kinds of inflight.cycle_case in turn: the whole workgroup leaves at list_n == 0, at "empty" and at
    "cleared", or none of it does."""
    rng = np.random.default_rng(12800)
    rows, k2i, windows, kw, kind = inflight.cycle_case(rng, 200)
    c_ref, b_ref = every_w(rows, k2i, windows, kw)
    fwd = c_ref[:, 0]
    assert (fwd[kind == 0] == 1).all() and (b_ref[kind == 0, 0, 0] == 7).all()
    assert (c_ref[kind == 1] == 0).all() and (c_ref[kind == 2] == 0).all() and (fwd[kind == 3] == 0).all()
    assert (fwd[kind == 4] == 24).all()
