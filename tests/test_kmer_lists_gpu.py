"""The per-k-mer bucket-id lists of the plain vote: for every k-mer the ascending ids of the buckets in the AND of the rows
of its G q-grams, read by bmf_vote_kernel_lists instead of rows.  The lists against the AND computed in numpy from the
index they were built from, and the filter's outputs with the lists against the same filter on the index rows
(BMF_FLAG_PLAIN_ROWS) and against the oracle: counts, bucket ids and the number of rows the reference ANDs, bit for bit.

Small q throughout.  The table holds 4^k lists of up to NB ids, so k stays at 5 or 6 for G = 2, 3, 4 (q = 4, 4, 3): a few
MB to a few hundred at the largest NB.  G = 8 needs k >= 9 (q = 2: 262 144 lists): half of its rows are sparse, so most
lists are short (mixed_index) -- but with a quarter of the q-grams indexed one k-mer in ten has none, a list of NB ids
each: gigabytes at the largest NB, which is what that case costs."""
import os

import numpy as np
import pytest

from conftest import assert_same_candidates, oracle_map_windows

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTacgtN", np.uint8)
FORCE = {"BMF_DERIVED": "1", "BMF_KMER_LISTS": "1"}     # random indexes are denser than the rule accepts
NB_MAX = 65535                                          # 0xFFFF pads the lists: it must be no bucket


def random_index(rng, nb, q, kmer_frac, density):
    """(rows in the .qgram layout, kmer_to_index): each q-gram kept with probability kmer_frac; `density` is one number
    or one per kept row."""
    kept = rng.random(4 ** q) < kmer_frac
    if not kept.any():
        kept[rng.integers(0, 4 ** q)] = True
    k2i = np.full(4 ** q, -1, np.int32)
    k2i[kept] = np.arange(kept.sum())
    dens = np.broadcast_to(np.asarray(density, float), (int(kept.sum()),))
    rows = np.packbits(rng.random((int(kept.sum()), nb)) < dens[:, None], axis=1, bitorder="little")
    return rows, k2i


def mixed_index(rng, nb, q, G, kmer_frac):
    """One row in 20 (at least one) is sparse (1 %): a k-mer that holds its q-gram has an empty or nearly empty list.
    The others are dense enough that their AND keeps about half the buckets (lists longer than 512 ids from NB = 2 049 on,
    hit counts that reach S - F, and ties above max_candidates at the larger NB).  With kmer_frac 0.25 some k-mers have no
    indexed q-gram at all: lists of NB ids.
    G = 8 (q = 2, 16 rows): half of the rows hold about 16 buckets, AA among them and always indexed, the others nine
    buckets in ten -- most k-mers have short or empty lists, the few made of dense q-grams only have long ones, and the
    windows of one repeated A keep the candidates of row AA."""
    n = 4 ** q
    kept = rng.random(n) < kmer_frac
    if G < 8:
        dens = np.full(n, 0.5 ** (1.0 / G) if kmer_frac == 1.0 else 0.3)
        dens[rng.permutation(n)[: max(1, n // 20)]] = 0.01
    else:
        dens = np.full(n, 0.9)
        dens[rng.permutation(n)[: n // 2]] = min(0.5, 16.0 / nb)
        dens[0] = min(0.5, 16.0 / nb)
        kept[0] = True
    if not kept.any():
        kept[0] = True
    k2i = np.full(n, -1, np.int32)
    k2i[kept] = np.arange(kept.sum())
    rows = np.packbits(rng.random((int(kept.sum()), nb)) < dens[kept][:, None], axis=1, bitorder="little")
    return rows, k2i


def random_windows(rng, n, read_len, k):
    """n windows back to back: half of them read_len long, the others of any length from 0 (those shorter than k, and
    those whose qualities fail the filter, are the rejected ones); then windows of one repeated base and of a 2-base
    repeat, whose S samples are the same one or two k-mers."""
    lens = rng.integers(0, read_len + 1, n)
    lens[: n // 2] = read_len
    lens[-8:] = read_len
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    bases = LETTERS[rng.integers(0, len(LETTERS), int(off[-1]))]
    quals = rng.integers(33, 33 + 42, int(off[-1])).astype(np.uint8)
    for i, unit in enumerate((b"A", b"C", b"G", b"T", b"AC", b"GT", b"CG", b"TA")):
        w = n - 8 + i
        rep = np.frombuffer(unit * read_len, np.uint8)[:read_len]
        bases[int(off[w]): int(off[w]) + read_len] = rep
        quals[int(off[w]): int(off[w]) + read_len] = 33 + 40
    return bases, quals, off[:-1].copy(), lens.astype(np.uint32)


def params(nb, q, k, S, flags=0):
    # threshold 0: every indexed q-gram is distinguishable; min_base_quality 18 per base: some k-mers fail it
    return dict(num_buckets=nb, q=q, k=k, num_samples=S, num_fault=6 if S < 64 else 26, threshold=0, min_base_quality=18 * k,
                max_candidates=30, read_len=80, flags=flags)


def new_filter(rows, k2i, env=FORCE, **kw):
    """A context with the index loaded; `env` holds while it is created and loaded (the table is decided at load)."""
    import bucket_map_amd as bma
    names = set(env) | {"BMF_DERIVED", "BMF_KMER_LISTS", "BMF_DERIVED_MAX_MB"}
    saved = {name: os.environ.get(name) for name in names}
    for name in names:
        os.environ.pop(name, None)
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


def kmer_and(rows, k2i, nb, q, G, x):
    out = np.packbits(np.ones(nb, bool), bitorder="little")
    for g in range(G):
        i = k2i[(x >> (2 * g)) & (4 ** q - 1)]
        if i >= 0:
            out = out & rows[i]
    return out


def check_lists(flt, k2i, nb, q, G, rng):
    """derived_row of the first, the last and 200 random k-mers against numpy; returns how many had no indexed q-gram."""
    rows = flt.index_download()
    k = q + G - 1
    none_indexed = 0
    for x in np.unique(np.concatenate(([0, 4 ** k - 1], rng.integers(0, 4 ** k, 200)))):
        x = int(x)
        got = flt.derived_row(x)
        assert np.array_equal(got, kmer_and(rows, k2i, nb, q, G, x)), f"k-mer {x}"
        if nb & 7:
            assert got[-1] >> (nb & 7) == 0, f"k-mer {x}: bits >= NB set"
        if all(k2i[(x >> (2 * g)) & (4 ** q - 1)] < 0 for g in range(G)):
            none_indexed += 1
            assert int(np.unpackbits(got).sum()) == nb
    return none_indexed


def test_lists_are_the_and_of_the_index_rows():
    rng = np.random.default_rng(61)
    nb, q, G = 128 * 64 + 5, 4, 3
    rows, k2i = random_index(rng, nb, q, 0.25, 0.5)
    flt = new_filter(rows, k2i, **params(nb, q, q + G - 1, 15))
    info = flt.info()
    assert info["derived_span"] == G and info["derived_form"] == "kmer_lists"
    assert check_lists(flt, k2i, nb, q, G, rng) > 20
    # offsets (4^k + 1, 64-bit, in 16-byte units) plus every list padded to whole units of 8 ids
    n_k = 4 ** (q + G - 1)
    bits = np.unpackbits(np.vstack([rows, np.packbits(np.ones(nb, bool), bitorder="little")[None]]), axis=1, bitorder="little")[:, :nb]
    x = np.arange(n_k)
    acc = np.ones((n_k, nb), bool)
    for g in range(G):
        acc &= bits[k2i[(x >> (2 * g)) & (4 ** q - 1)]].astype(bool)          # -1: the all-ones row appended above
    units = (acc.sum(axis=1) + 7) // 8
    assert info["derived_bytes"] == 8 * (n_k + 1) + 16 * int(units.sum())
    flt.close()


def compare_three_ways(rng, nb, q, G, S, kmer_frac, n_windows, expect_form):
    import bucket_map_amd as bma
    k = q + G - 1
    rows, k2i = mixed_index(rng, nb, q, G, kmer_frac)
    windows = random_windows(rng, n_windows, 80, k)
    kw = params(nb, q, k, S)
    lists = new_filter(rows, k2i, **kw)
    plain = new_filter(rows, k2i, **{**kw, "flags": bma.BMF_FLAG_PLAIN_ROWS})
    assert lists.info()["derived_form"] == expect_form and plain.info()["derived_form"] == "rows"
    assert lists.info()["derived_span"] == (G if expect_form == "kmer_lists" else 2)
    if G == 8 and S == 15 and expect_form == "kmer_lists":
        check_lists(lists, k2i, nb, q, G, rng)                 # seven shared rows per prefix in the build kernels
    c_l, b_l, n_l = run_batch(lists, windows)
    c_p, b_p, n_p = run_batch(plain, windows)
    lists.close()
    plain.close()
    c_ref, b_ref, n_ref = oracle_run(rows, k2i, windows, **kw)
    what = f"NB={nb} q={q} k={k} S={S} kmer_frac={kmer_frac}"
    assert_same_candidates(c_ref, b_ref, c_p, b_p, what + ", index rows")
    assert_same_candidates(c_ref, b_ref, c_l, b_l, what + ", " + expect_form)
    assert n_p == n_ref and n_l == n_ref, (what, n_l, n_p, n_ref)
    # the batch exercises what it is meant to: windows that vote, rejected windows, and the repeats at the end
    assert n_ref > 0 and (c_ref > 0).any() and (windows[3] < k).any()
    return c_ref


Q_OF_G = {2: 4, 3: 4, 4: 3, 8: 2}


@pytest.mark.parametrize("nb", [100, 2049, 128 * 64 + 5, 3 * 8192 + 1, NB_MAX, NB_MAX + 1])
@pytest.mark.parametrize("G", [2, 3, 4, 8])
def test_outputs_equal_plain_rows_and_oracle(G, nb):
    rng = np.random.default_rng(1000 * G + nb % 991)
    n_windows = 1500 if nb < 20000 else 500
    # NB_MAX + 1 is not eligible (the padding id would be a bucket): it falls back to the pair table and is still right
    form = "kmer_lists" if nb <= NB_MAX else "pairs"
    # S = 15: 4-bit counters, 16: the first 8-bit S, 64: the most samples; each with all and with a quarter of the q-grams
    for S, kmer_frac in ((15, 1.0), (15, 0.25), (16, 0.25), (16, 1.0), (64, 1.0), (64, 0.25)):
        compare_three_ways(rng, nb, Q_OF_G[G], G, S, kmer_frac, n_windows if S < 64 else n_windows // 3, form)


def test_repeated_kmers_reach_s_hits():
    """Windows of one base and of a 2-base repeat: all S samples are the same one or two k-mers, so a bucket of their
    list is hit S times -- the counters' highest value, in the 4-bit and in the 8-bit form."""
    rng = np.random.default_rng(62)
    nb, q, G = 2049, 4, 2
    for S in (15, 16, 64):
        kw = params(nb, q, q + G - 1, S)
        # sparse rows: a one-base window ANDs one row with itself, about 16 buckets -- fewer than max_candidates
        rows, k2i = random_index(rng, nb, q, 1.0, 0.008)
        windows = random_windows(rng, 400, 80, q + G - 1)
        flt = new_filter(rows, k2i, **kw)
        assert flt.info()["derived_form"] == "kmer_lists"
        c, b, n = run_batch(flt, windows)
        flt.close()
        c_ref, b_ref, n_ref = oracle_run(rows, k2i, windows, **kw)
        assert_same_candidates(c_ref, b_ref, c, b, f"S={S}")
        assert n == n_ref
        assert (c_ref[-8:-4] > 0).any(), "no one-base window kept a candidate"


def test_fallbacks_and_the_rule():
    import bucket_map_amd as bma
    rng = np.random.default_rng(63)
    nb, q, k = 2049, 4, 6
    rows, k2i = random_index(rng, nb, q, 1.0, 0.45 ** (1 / 3))
    windows = random_windows(rng, 800, 80, k)
    kw = params(nb, q, k, 15)
    lists = new_filter(rows, k2i, **kw)
    info = lists.info()
    assert info["derived_form"] == "kmer_lists"
    want = run_batch(lists, windows)
    lists.close()
    pair_mb = (4 ** (q + 1) + 1) * info["row_pitch_bytes"] / 2 ** 20
    assert pair_mb < 1 < info["derived_bytes"] / 2 ** 20
    for name, env, form, span in (
            ("BMF_KMER_LISTS=0", {"BMF_DERIVED": "1", "BMF_KMER_LISTS": "0"}, "pairs", 2),
            ("BMF_DERIVED_MAX_MB", {**FORCE, "BMF_DERIVED_MAX_MB": "1"}, "pairs", 2),     # room for the pair table only
            ("the rule", {}, "pairs", 2),                                               # dense: the lists do not pay
            ("BMF_DERIVED=0", {"BMF_DERIVED": "0", "BMF_KMER_LISTS": "1"}, "rows", 1)):
        flt = new_filter(rows, k2i, env=env, **kw)
        assert flt.info()["derived_form"] == form and flt.info()["derived_span"] == span, name
        got = run_batch(flt, windows)
        flt.close()
        assert_same_candidates(want[0], want[1], got[0], got[1], name)
        assert got[2] == want[2]
    plain = new_filter(rows, k2i, **{**kw, "flags": bma.BMF_FLAG_PLAIN_ROWS})
    assert plain.info()["derived_form"] == "rows" and plain.info()["derived_bytes"] == 0
    plain.close()
    # a pruning context builds nothing derived, and reports itself as it did
    off = new_filter(rows, k2i, env={"BMF_DERIVED": "0"}, **{**kw, "flags": bma.BMF_FLAG_EARLY_EXIT})
    on = new_filter(rows, k2i, **{**kw, "flags": bma.BMF_FLAG_EARLY_EXIT})
    assert on.info()["derived_form"] == "rows" and on.info()["derived_span"] == 1 and on.info()["derived_bytes"] == 0
    assert on.info() == off.info()
    got = run_batch(on, windows)
    assert_same_candidates(want[0], want[1], got[0], got[1], "BMF_FLAG_EARLY_EXIT")
    on.close()
    off.close()


def test_sparse_index_gets_the_lists_unasked():
    rng = np.random.default_rng(64)
    nb, q, k = 2049, 4, 5
    for density, form in ((0.1, "kmer_lists"), (0.45, "pairs")):           # AND of two rows: 1 % and 20 %
        rows, k2i = random_index(rng, nb, q, 1.0, density)
        flt = new_filter(rows, k2i, env={}, **params(nb, q, k, 15))
        assert flt.info()["derived_form"] == form, density
        flt.close()


def test_reload_rebuilds_the_lists():
    rng = np.random.default_rng(65)
    nb, q, G = 2500, 4, 3
    k = q + G - 1
    kw = params(nb, q, k, 15)
    windows = random_windows(rng, 800, 80, k)
    first = random_index(rng, nb, q, 1.0, 0.45 ** (1 / 3))
    second = random_index(rng, nb, q, 0.25, 0.8)
    env = dict(FORCE)
    os.environ.update(env)
    try:
        flt = new_filter(*first, **kw)
        check_lists(flt, first[1], nb, q, G, rng)
        flt.reset()
        flt.load_index(*second)
    finally:
        for name in env:
            os.environ.pop(name, None)
    assert flt.info()["derived_form"] == "kmer_lists"
    check_lists(flt, second[1], nb, q, G, rng)
    c, b, n = run_batch(flt, windows)
    flt.close()
    c_ref, b_ref, n_ref = oracle_run(*second, windows, **kw)
    assert_same_candidates(c_ref, b_ref, c, b, "after the reload")
    assert n == n_ref
    c1, _, _ = oracle_run(*first, windows, **kw)
    assert not np.array_equal(c1, c_ref)                       # the two indexes do give different answers
