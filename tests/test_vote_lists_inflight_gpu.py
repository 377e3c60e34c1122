"""bmf_vote_kernel_lists with its LDS adds in flight (eight per unit issued back to back, folded one unit later, a padding
id adding 0 instead of branching): the shapes at which that can go wrong.  Every case compares counts, bucket ids and the
number of rows the reference ANDs, bit for bit, against the same filter on the index rows (BMF_FLAG_PLAIN_ROWS) and against
the oracle.

The cases also set BMF_LISTS_WAVES = n: the hook of the kernel form in which one resident round of waves walks several
items each (n caps its grid, so that with 1, 2 or 3 every wave meets what the item before left behind).  That form was
built, passed these cases and measured slower (profiles/r07/README.md), so the kernel that ships runs one item per
workgroup and does not read the variable: the capped runs then repeat the uncapped one.  They stay for the day the item
loop comes back.  Small q throughout: k = 5, a few MB of lists."""
import numpy as np
import pytest

import test_kmer_lists_gpu as kl
from conftest import assert_same_candidates

pytestmark = pytest.mark.gpu

Q, G = 4, 2
K = Q + G - 1
READ_LEN = 80
GOOD = 33 + 40


def three_ways(rows, k2i, windows, kw, caps=(None,)):
    """The oracle's (counts, buckets) after checking the index rows and, under every cap, the lists against it."""
    import bucket_map_amd as bma
    what = f"NB={kw['num_buckets']} S={kw['num_samples']}"
    c_ref, b_ref, n_ref = kl.oracle_run(rows, k2i, windows, **kw)
    plain = kl.new_filter(rows, k2i, **{**kw, "flags": bma.BMF_FLAG_PLAIN_ROWS})
    assert plain.info()["derived_form"] == "rows"
    c_p, b_p, n_p = kl.run_batch(plain, windows)
    plain.close()
    assert_same_candidates(c_ref, b_ref, c_p, b_p, what + ", index rows")
    assert n_p == n_ref
    for cap in caps:
        env = dict(kl.FORCE) if cap is None else {**kl.FORCE, "BMF_LISTS_WAVES": str(cap)}
        lists = kl.new_filter(rows, k2i, env=env, **kw)
        assert lists.info()["derived_form"] == "kmer_lists"
        c_l, b_l, n_l = kl.run_batch(lists, windows)
        lists.close()
        assert_same_candidates(c_ref, b_ref, c_l, b_l, f"{what}, lists, cap {cap}")
        assert n_l == n_ref, (what, cap)
    return c_ref, b_ref


def run_index(rng, nb, q):
    """Rows whose set buckets come in runs of 24 consecutive ids on one grid (3 + 24 j: no run starts on a counter dword),
    so the AND of two rows is made of whole runs: the eight ids of a unit lie in two neighbouring counter dwords (three in
    the 8-bit form) and the units of neighbouring lanes share them.  One row in four keeps few runs; the rows of the four
    one-base q-grams keep one run each, which a window of that base then hits S times."""
    n, n_runs = 4 ** q, (nb - 3) // 24
    p = np.where(np.arange(n) % 4 == 1, 0.04, 0.7)
    have = rng.random((n, n_runs)) < p[:, None]
    for j, gram in enumerate((0, (4 ** q - 1) // 3, 2 * (4 ** q - 1) // 3, 4 ** q - 1)):
        have[gram] = False
        have[gram, 5 + 11 * j] = True
    bits = np.zeros((n, nb), bool)
    bits[:, 3: 3 + 24 * n_runs] = np.repeat(have, 24, axis=1)
    return np.packbits(bits, axis=1, bitorder="little"), np.arange(n, dtype=np.int32)


@pytest.mark.parametrize("S", [15, 16, 64])
def test_adds_piling_on_one_dword(S):
    rng = np.random.default_rng(700 + S)
    nb = 2049
    rows, k2i = run_index(rng, nb, Q)
    windows = kl.random_windows(rng, 300, READ_LEN, K)          # the last eight: one repeated base, a 2-base repeat
    c_ref, _ = three_ways(rows, k2i, windows, kl.params(nb, Q, K, S), caps=(None, 2))
    assert (c_ref[:-8] > 0).any(), "no random window voted"
    assert (c_ref[-8:-4].max(axis=1) == 24).all(), "a one-base window keeps the one run of its row"


def cycle_case(rng, n_windows, S=15):
    """n_windows windows in a fixed cycle of five kinds, on an index built for them:
       0 voting          every q-gram of the read holds bucket 7
       1 rejected        shorter than k
       2 nothing near    random bases on sparse rows: the best count stays at or below S - F
       3 cleared         every q-gram of the read holds buckets 100 .. 160: 61 ties, more than max_candidates
       4 repeated base   all A: the one k-mer's list S times"""
    nb, n = 2049, 4 ** Q
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    reads = [kl.LETTERS[rng.integers(0, 4, READ_LEN)] for _ in range(3)]
    grams = [{sum(code[int(c)] << (2 * (Q - 1 - j)) for j, c in enumerate(r[i: i + Q])) for i in range(READ_LEN - Q + 1)} for r in reads]
    bits = rng.random((n, nb)) < 0.004
    bits[:, :200] = False
    # (either packing order of a q-gram: the rows of both are given the buckets, the test does not depend on which is used)
    rev = lambda g: sum(((g >> (2 * j)) & 3) << (2 * (Q - 1 - j)) for j in range(Q))
    for g in grams[0]:
        bits[g, 7] = bits[rev(g), 7] = True
    for g in grams[2]:
        bits[g, 100:161] = bits[rev(g), 100:161] = True
    bits[0] = False
    bits[0, 500:524] = True                                     # AAAA
    rows, k2i = np.packbits(bits, axis=1, bitorder="little"), np.arange(n, dtype=np.int32)
    kind = np.arange(n_windows) % 5
    body = {0: reads[0], 1: reads[1][:3], 2: reads[1], 3: reads[2], 4: np.full(READ_LEN, 65, np.uint8)}
    lens = np.array([len(body[int(t)]) for t in kind], np.uint32)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    bases = np.concatenate([body[int(t)] for t in kind])
    quals = np.full(len(bases), GOOD, np.uint8)
    return rows, k2i, (bases, quals, off[:-1].copy(), lens), kl.params(nb, Q, K, S), kind


def test_every_exit_followed_by_every_other():
    rng = np.random.default_rng(71)
    rows, k2i, windows, kw, kind = cycle_case(rng, 200)
    c_ref, b_ref = three_ways(rows, k2i, windows, kw, caps=(1, 2, 3, None))
    fwd = c_ref[:, 0]
    assert (fwd[kind == 0] == 1).all() and (b_ref[kind == 0, 0, 0] == 7).all()
    assert (c_ref[kind == 1] == 0).all() and (c_ref[kind == 2] == 0).all() and (fwd[kind == 3] == 0).all()
    assert (fwd[kind == 4] == 24).all()
    # ... and the cleared kind is cleared, not empty: with room for them the 61 ties come back
    c_wide, _, _ = kl.oracle_run(rows, k2i, windows, **{**kw, "max_candidates": 100})
    assert (c_wide[kind == 3, 0] == 61).all()
    # more waves than items, and a window count that no cap divides
    one = tuple(a[:1] for a in windows[2:])
    three_ways(rows, k2i, (windows[0], windows[1]) + one, kw, caps=(3,))
    rows, k2i, windows, kw, kind = cycle_case(rng, 203)
    three_ways(rows, k2i, windows, kw, caps=(2, 3))


@pytest.mark.parametrize("nb", [2049, 128 * 64 + 5])
def test_long_lists_under_the_prefetch(nb):
    """A quarter of the q-grams indexed: a k-mer with none holds all NB ids, 257 and 1 025 units, far into the tail path
    while the next item's units are in flight."""
    for S in (15, 16, 64):
        rng = np.random.default_rng(7200 + nb % 97 + S)
        rows, k2i = kl.mixed_index(rng, nb, Q, G, 0.25)
        windows = kl.random_windows(rng, 240 if S < 64 else 80, READ_LEN, K)
        c_ref, _ = three_ways(rows, k2i, windows, kl.params(nb, Q, K, S), caps=(2,))
        assert (c_ref > 0).any()


@pytest.mark.parametrize("nb, S", [(100, 15), (100, 16), (kl.NB_MAX, 15), (kl.NB_MAX, 16)])
def test_edges_of_the_counter_array(nb, S):
    """NB = 100: fewer 16-byte groups of counters than lanes; NB = 65 535: the raised dynamic LDS, a few waves per CU, and
    the padding id's own dword inside the counters.  120 items on 8 waves: 15 each."""
    rng = np.random.default_rng(7300 + nb % 89 + S)
    rows, k2i = kl.mixed_index(rng, nb, Q, G, 1.0)
    windows = kl.random_windows(rng, 60, READ_LEN, K)
    c_ref, _ = three_ways(rows, k2i, windows, kl.params(nb, Q, K, S), caps=(8,))
    assert (c_ref > 0).any()


def test_pieces_launch_with_their_own_window_counts(monkeypatch):
    rng = np.random.default_rng(74)
    nb, S = 2049, 15
    rows, k2i = kl.mixed_index(rng, nb, Q, G, 1.0)
    windows = kl.random_windows(rng, 300, READ_LEN, K)
    kw = kl.params(nb, Q, K, S)
    c_ref, b_ref = three_ways(rows, k2i, windows, kw, caps=(3,))
    mask = np.arange(b_ref.shape[-1])[None, None, :] < c_ref[:, :, None]
    for cap, piece in ((3, "64"), (None, "97"), (3, "100000")):
        env = dict(kl.FORCE) if cap is None else {**kl.FORCE, "BMF_LISTS_WAVES": str(cap)}
        flt = kl.new_filter(rows, k2i, env=env, **kw)
        monkeypatch.setenv("BMF_PIECE_WINDOWS", piece)
        c, ids = flt.map_windows_compact(*windows)
        flt.close()
        assert np.array_equal(c, c_ref) and np.array_equal(ids, b_ref[mask]), (cap, piece)
