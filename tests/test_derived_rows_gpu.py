"""The pair table of the plain vote: one row per (q+1)-gram, the AND of the rows of the two q-grams it holds, read by
the default kernel instead of the index rows (half the row bytes per read).  Row by row against the index it was
built from, and the filter's outputs with the table against the same filter on the index rows (BMF_FLAG_PLAIN_ROWS) and
against the oracle: counts, bucket ids and the number of rows the reference ANDs, bit for bit.  Small q throughout:
the tables stay at a few MB."""
import numpy as np
import pytest

from conftest import assert_same_candidates, oracle_map_windows

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTacgtN", np.uint8)


def random_index(rng, nb, q, kmer_frac, density):
    """(rows in the .qgram layout, kmer_to_index): each q-gram kept with probability kmer_frac, bits set with `density`."""
    kept = rng.random(4 ** q) < kmer_frac
    k2i = np.full(4 ** q, -1, np.int32)
    k2i[kept] = np.arange(kept.sum())
    rows = np.packbits(rng.random((int(kept.sum()), nb)) < density, axis=1, bitorder="little")
    return rows, k2i


def random_windows(rng, n, read_len):
    """n windows back to back: half of them read_len long, the others of any length from 0 (those shorter than k, and
    those whose qualities fail the filter, are the rejected ones)."""
    lens = rng.integers(0, read_len + 1, n)
    lens[: n // 2] = read_len
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    bases = LETTERS[rng.integers(0, len(LETTERS), int(off[-1]))]
    quals = rng.integers(33, 33 + 42, int(off[-1])).astype(np.uint8)
    return bases, quals, off[:-1].copy(), lens.astype(np.uint32)


def params(nb, q, k, S, flags=0):
    # threshold 0: every indexed q-gram is distinguishable; min_base_quality 18 per base: some k-mers fail it
    return dict(num_buckets=nb, q=q, k=k, num_samples=S, num_fault=6, threshold=0, min_base_quality=18 * k, max_candidates=30,
                read_len=80, flags=flags)


def new_filter(rows, k2i, env=None, **kw):
    """A context with the index loaded.  `env` holds while it is created and loaded (the table is decided at load);
    by default BMF_DERIVED=1: on its own the library keeps the index rows for NB <= 2 048, and the short rows are
    where CPL is 1."""
    import os
    import bucket_map_amd as bma
    env = {"BMF_DERIVED": "1"} if env is None else env
    saved = {name: os.environ.get(name) for name in env}
    os.environ.update(env)
    try:
        f = bma.Filter(bma.Params(**kw))
        f.load_index(rows, k2i)
    finally:
        for name, value in saved.items():
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value
    return f


def run_batch(flt, windows):
    b = flt.batch(*windows)
    b.run()
    counts, buckets = b.download()
    anded = b.rows_anded()
    b.close()
    return counts, buckets, anded


def oracle_run(rows, k2i, windows, **kw):
    from oracle import oracle_c as oc
    kw = {key: v for key, v in kw.items() if key != "flags"}
    ix = oc.Index(oc.make_params(kw.pop("num_buckets"), **kw), rows, k2i)
    return oracle_map_windows(ix, *windows)


def expected_pair_row(rows, k2i, nb, q, x):
    ones = np.packbits(np.ones(nb, bool), bitorder="little")
    lo, hi = x & (4 ** q - 1), x >> 2
    r_lo = rows[k2i[lo]] if k2i[lo] >= 0 else ones
    r_hi = rows[k2i[hi]] if k2i[hi] >= 0 else ones
    return r_lo & r_hi


def check_rows(flt, k2i, nb, q, rng):
    rows = flt.index_download()
    grams = np.unique(np.concatenate(([0, 4 ** (q + 1) - 1], rng.integers(0, 4 ** (q + 1), 200))))
    lo_missing = hi_missing = 0
    for x in grams:
        x = int(x)
        got = flt.derived_row(x)
        assert np.array_equal(got, expected_pair_row(rows, k2i, nb, q, x)), f"pair row {x}"
        if nb & 7:
            assert got[-1] >> (nb & 7) == 0, f"pair row {x}: bits >= NB set"
        lo_missing += k2i[x & (4 ** q - 1)] < 0
        hi_missing += k2i[x >> 2] < 0
    return lo_missing, hi_missing


def compare_three_ways(rng, nb, q, k, S, kmer_frac, n_windows, expect_span):
    """Derived context == BMF_FLAG_PLAIN_ROWS context == oracle on one random index and batch."""
    import bucket_map_amd as bma
    G = k - q + 1
    # a sample's G rows AND to a hit with probability ~ 0.45 whatever G is: lists of a few buckets, some empty, some cleared
    # (with q-grams that are not indexed, a sample ANDs fewer rows and some AND none: sparser rows keep the ties few)
    rows, k2i = random_index(rng, nb, q, kmer_frac, 0.45 ** (1.0 / G) if kmer_frac == 1.0 else 0.3)
    windows = random_windows(rng, n_windows, 80)
    kw = params(nb, q, k, S)
    derived = new_filter(rows, k2i, **kw)
    plain = new_filter(rows, k2i, **{**kw, "flags": bma.BMF_FLAG_PLAIN_ROWS})
    assert derived.info()["derived_span"] == expect_span and plain.info()["derived_span"] == 1
    assert (derived.info()["derived_bytes"] > 0) == (expect_span == 2) and plain.info()["derived_bytes"] == 0
    c_d, b_d, n_d = run_batch(derived, windows)
    c_p, b_p, n_p = run_batch(plain, windows)
    derived.close()
    plain.close()
    c_ref, b_ref, n_ref = oracle_run(rows, k2i, windows, **kw)
    what = f"NB={nb} q={q} k={k} S={S} kmer_frac={kmer_frac}"
    assert_same_candidates(c_ref, b_ref, c_p, b_p, what + ", index rows")
    assert_same_candidates(c_ref, b_ref, c_d, b_d, what + ", pair table")
    assert n_p == n_ref and n_d == n_ref, (what, n_d, n_p, n_ref)
    # the batch exercises what it is meant to: windows that vote, candidates in both orientations, rejected windows
    assert n_ref > 0 and (c_ref[:, 0] > 0).any() and (c_ref[:, 1] > 0).any()
    assert (windows[3] < k).any()


def test_pair_rows_are_the_and_of_their_two_index_rows():
    rng = np.random.default_rng(51)
    nb, q = 128 * 64 + 5, 5
    rows, k2i = random_index(rng, nb, q, 0.25, 0.5)
    flt = new_filter(rows, k2i, **params(nb, q, q + 1, 15))
    info = flt.info()
    assert info["derived_span"] == 2 and info["derived_bytes"] == (4 ** (q + 1) + 1) * info["row_pitch_bytes"]
    lo_missing, hi_missing = check_rows(flt, k2i, nb, q, rng)
    assert lo_missing > 20 and hi_missing > 20              # q-grams that are not indexed, on either side
    flt.close()


@pytest.mark.parametrize("nb", [100, 128 * 64 + 5, 3 * 8192 + 1])          # CPL 1, a partial last chunk, CPL > 1
@pytest.mark.parametrize("G", [1, 2, 3, 4, 5, 8])                           # 1: no table; 3, 5: overlapping last pair
def test_outputs_equal_plain_rows_and_oracle(G, nb):
    q = 5
    rng = np.random.default_rng(100 * G + nb % 97)
    # S * ceil(G/2) both off and on a multiple of the ring depth (8, 8 and 4 at these NB): S = 15 and S = 16
    for kmer_frac, S in ((1.0, 15), (0.25, 16)):
        compare_three_ways(rng, nb, q, q + G - 1, S, kmer_frac, 2000 if nb < 20000 else 1200, 2 if G >= 2 else 1)


def test_sliced_rows_and_merge():
    rng = np.random.default_rng(7)
    compare_three_ways(rng, 70_000, 4, 6, 15, 1.0, 600, 2)                  # NB > 65 536: two slices + merge, G = 3


def test_fallbacks():
    import bucket_map_amd as bma
    rng = np.random.default_rng(8)
    nb, q, k = 1000, 5, 8
    rows, k2i = random_index(rng, nb, q, 1.0, 0.45 ** 0.25)
    windows = random_windows(rng, 1000, 80)
    kw = params(nb, q, k, 15)
    derived = new_filter(rows, k2i, **kw)
    assert derived.info()["derived_span"] == 2
    want = run_batch(derived, windows)
    derived.close()
    for name, env in (("BMF_DERIVED_MAX_MB", {"BMF_DERIVED": "1", "BMF_DERIVED_MAX_MB": "0"}), ("BMF_DERIVED", {"BMF_DERIVED": "0"}),
                      ("short rows", {})):                 # NB = 1 000: no table unless asked for
        flt = new_filter(rows, k2i, env=env, **kw)
        assert flt.info()["derived_span"] == 1 and flt.info()["derived_bytes"] == 0
        with pytest.raises(bma.BmfError) as e:
            flt.derived_row(0)
        assert e.value.code == bma.BMF_ERR_STATE
        got = run_batch(flt, windows)
        flt.close()
        assert_same_candidates(want[0], want[1], got[0], got[1], name)
        assert got[2] == want[2]
    # a pruning context never builds the table, and reports its pruning form as it did
    off = new_filter(rows, k2i, env={"BMF_DERIVED": "0"}, **{**kw, "flags": bma.BMF_FLAG_EARLY_EXIT})
    on = new_filter(rows, k2i, **{**kw, "flags": bma.BMF_FLAG_EARLY_EXIT})
    assert on.info()["derived_span"] == 1 and on.info()["derived_bytes"] == 0
    assert on.info() == off.info()
    assert {"pass1_rows", "pass1_fold", "pass1_fold_rows", "rows_in_flight", "planes", "chunks_per_lane", "row_pitch_bytes"} <= set(on.info())
    got = run_batch(on, windows)
    assert_same_candidates(want[0], want[1], got[0], got[1], "BMF_FLAG_EARLY_EXIT")
    on.close()
    off.close()


def test_long_rows_get_the_table_unasked():
    rng = np.random.default_rng(10)
    for nb, span in ((2048, 1), (2049, 2)):                    # 16 and 17 chunks of 128 buckets
        rows, k2i = random_index(rng, nb, 5, 1.0, 0.5)
        flt = new_filter(rows, k2i, env={}, **params(nb, 5, 7, 15))
        assert flt.info()["derived_span"] == span, nb
        flt.close()


def test_reload_rebuilds_the_table():
    rng = np.random.default_rng(9)
    nb, q, k = 2500, 5, 7                                      # long enough for the table to be built unasked
    kw = params(nb, q, k, 15)
    windows = random_windows(rng, 1000, 80)
    first = random_index(rng, nb, q, 1.0, 0.45 ** (1 / 3))
    second = random_index(rng, nb, q, 0.25, 0.8)
    flt = new_filter(*first, env={}, **kw)
    check_rows(flt, first[1], nb, q, rng)
    flt.reset()
    flt.load_index(*second)
    assert flt.info()["derived_span"] == 2
    check_rows(flt, second[1], nb, q, rng)
    c, b, n = run_batch(flt, windows)
    flt.close()
    c_ref, b_ref, n_ref = oracle_run(*second, windows, **kw)
    assert_same_candidates(c_ref, b_ref, c, b, "after the reload")
    assert n == n_ref
    c1, _, _ = oracle_run(*first, windows, **kw)
    assert not np.array_equal(c1, c_ref)                       # the two indexes do give different answers
