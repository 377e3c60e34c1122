"""The filter on a REUSED context, after a larger batch: every form of the vote through every way in (include/bmf.h).

A context and a batch keep their device buffers and clear little between runs (the queue counters of the two-pass forms).
So, per form, ONE context serves big (3 000 windows of 80 bases: dense enough that most windows vote and some lists are
cleared for holding more than max_candidates), small (5 windows: two shorter than k, one whose qualities fail the filter, one
that votes, one whose best count is exactly S - F and must stay empty), n = 0, small, big -- through bmf_map_windows,
bmf_map_windows_compact, bmf_map_text_windows_compact, a batch run twice, and two live batches of different sizes run and
downloaded crosswise.  A leftover of big lies where the rejected windows of small sit: counts, ids below the count and
rows_anded are the oracle's, bit for bit (oracle.oracle_c; the claims about the five windows are made by
oracle.bm_oracle_np's integer formulation before the GPU is asked).

q = 4, k = 6, NB = 2 049, S = 15, F = 3: with about half the buckets in the AND of most k-mers (and next to none in that of
one k-mer in seven) the best bucket of a window collects 11 to 15 of 15 hits, so S - F = 12 is reached exactly by some
windows and exceeded by seven in ten."""
import numpy as np
import pytest

import test_kmer_lists_gpu as kl
from oracle import bm_oracle_np as onp

pytestmark = pytest.mark.gpu

Q, K, NB, S, F, READ_LEN, N_BIG = 4, 6, 2049, 15, 3, 80, 3000
G = K - Q + 1
STEPS = ("big", "small", "empty", "small", "big")


def _forms():
    import bucket_map_amd as bma
    prune = bma.BMF_FLAG_EARLY_EXIT
    two = {(live, fold): (prune, {"BMF_PASS1_ROWS": "1", "BMF_MAX_LIVE": str(live), "BMF_FOLD": str(fold), "BMF_FOLD_ROWS": "2"})
           for live in (16, 32) for fold in (0, 2, 4)}
    return {
        "index rows": (bma.BMF_FLAG_PLAIN_ROWS, {}),
        "pair table": (0, {"BMF_DERIVED": "1", "BMF_KMER_LISTS": "0"}),
        **{f"k-mer lists, {w} waves an item": (0, {**kl.FORCE, "BMF_LISTS_ITEM_WAVES": str(w)}) for w in (1, 2, 4)},
        "single-pass pruning": (prune, {"BMF_PASS1_ROWS": "0"}),
        **{f"two-pass pruning, {live} live, fold {fold}": v for (live, fold), v in two.items()},
        "two-pass pruning in 3 slices": (prune, {"BMF_PASS1_ROWS": "1", "BMF_MAX_LIVE": "16", "BMF_FOLD": "0", "BMF_SLICES": "3"}),
    }


FORMS = ["index rows", "pair table", "k-mer lists, 1 waves an item", "k-mer lists, 2 waves an item", "k-mer lists, 4 waves an item",
         "single-pass pruning"] + [f"two-pass pruning, {live} live, fold {fold}" for live in (16, 32) for fold in (0, 2, 4)] + \
        ["two-pass pruning in 3 slices"]


def _kw(nb=NB, flags=0):
    return {**kl.params(nb, Q, K, S, flags), "num_fault": F}


def _levels(bits, k2i, bases, quals, kw):
    """query_sequence of oracle/bm_oracle_np.py up to the vote: None for a rejected window, else per orientation (the fewest
    misses of any bucket, how many buckets have them)."""
    hs, qs = onp.kmer_hashes(bases, K), onp.kmer_qualities(quals, K)
    good = [int(h) for h, s in zip(hs, qs)
            if s >= kw["min_base_quality"] and any(k2i[(int(h) >> (2 * i)) & (4 ** Q - 1)] >= 0 for i in range(G))]
    if len(good) < 0.2 * S:
        return None
    smp = [good[p] for p in onp.sample_positions(S, len(good) - 1)]
    out = []
    for hashes in (smp, [onp.hash_reverse_complement(h, K) for h in smp]):
        _, misses = onp.query_miss_counts(bits, k2i, hashes, k=K, q=Q, num_fault=F)
        out.append((int(misses.min()), int((misses == misses.min()).sum())))
    return out


@pytest.fixture(scope="module")
def world():
    """The index, the three batches and the oracle's answers, made once; what each batch claims to hold is asserted here."""
    rng = np.random.default_rng(20260201)
    rows, k2i = kl.mixed_index(rng, NB, Q, G, 1.0)
    bits, kw = onp.unpack_rows(rows, NB), _kw()
    big = kl.random_windows(rng, N_BIG, READ_LEN, K)
    c_big, b_big, n_big = kl.oracle_run(rows, k2i, big, **kw)
    voting = (c_big > 0).any(axis=1)
    assert voting.mean() > 0.5, f"only {voting.mean():.2f} of big vote"
    cleared = 0
    for w in range(N_BIG - 8, N_BIG):                           # the windows of one repeated base: S hits in a whole list
        at = int(big[2][w])
        lv = _levels(bits, k2i, big[0][at: at + READ_LEN], big[1][at: at + READ_LEN], kw)
        for o in range(2):
            if lv and lv[o][0] <= F - 1 and lv[o][1] > kw["max_candidates"]:
                assert c_big[w, o] == 0
                cleared += 1
    assert cleared > 0, "no list of big is cleared"
    # small: two windows shorter than k, one that fails the quality filter, one that votes, one at exactly S - F
    parts, quals = [], []
    voter = int(np.flatnonzero(voting & (big[3] == READ_LEN))[0])
    at = int(big[2][voter])
    for tries in range(4000):
        cand = kl.LETTERS[rng.integers(0, 8, READ_LEN)]
        cq = np.full(READ_LEN, 33 + 40, np.uint8)
        lv = _levels(bits, k2i, cand, cq, kw)
        if lv and lv[0][0] == F and lv[1][0] >= F:
            break
    else:
        raise AssertionError("no window whose best count is exactly S - F")
    for bases, q in ((kl.LETTERS[rng.integers(0, 4, K - 1)], None), (np.zeros(0, np.uint8), None),
                     (kl.LETTERS[rng.integers(0, 4, READ_LEN)], 33), (big[0][at: at + READ_LEN], big[1][at: at + READ_LEN]), (cand, cq)):
        parts.append(bases)
        quals.append(np.full(len(bases), 33 + 40 if q is None else q, np.uint8) if not isinstance(q, np.ndarray) else q)
    lens = np.array([len(p) for p in parts], np.uint32)
    small = (np.concatenate(parts), np.concatenate(quals), np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64), lens)
    c_small, b_small, n_small = kl.oracle_run(rows, k2i, small, **kw)
    assert (lens[:2] < K).all() and not c_small[:3].any() and c_small[3].any() and not c_small[4].any()
    assert _levels(bits, k2i, parts[2], quals[2], kw) is None and _levels(bits, k2i, parts[3], quals[3], kw) is not None
    assert np.array_equal(c_small[3], c_big[voter]) and n_small > 0
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    mc = kw["max_candidates"]
    return {"rows": rows, "k2i": k2i, "batch": {"big": big, "small": small, "empty": empty},
            "want": {"big": (c_big, b_big, n_big), "small": (c_small, b_small, n_small),
                     "empty": (np.zeros((0, 2), np.uint32), np.zeros((0, 2, mc), np.uint32), 0)}}


@pytest.fixture
def flt(world, request, monkeypatch):
    """a context of the form request.param with the index loaded; the form's environment holds for the whole test (some of it
    is read when the index is loaded, BMF_SLICES when a batch runs)"""
    flags, env = _forms()[request.param]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    f = kl.new_filter(world["rows"], world["k2i"], env=env, **_kw(flags=flags))
    info = f.info()
    if request.param == "index rows":
        assert info["derived_form"] == "rows" and info["pass1_rows"] == 0
    elif request.param == "pair table":
        assert info["derived_form"] == "pairs"
    elif request.param.startswith("k-mer lists"):
        assert info["derived_form"] == "kmer_lists" and info["lists_item_waves"] == int(env["BMF_LISTS_ITEM_WAVES"])
    elif request.param == "single-pass pruning":
        assert info["pass1_rows"] == 0 and info["derived_form"] == "rows"
    else:
        assert info["pass1_rows"] == 1 and info["pass1_fold"] == max(1, int(env["BMF_FOLD"]))
    yield f
    f.close()


def _same_dense(want, got, what):
    from conftest import assert_same_candidates
    assert_same_candidates(want[0], want[1], got[0], got[1], what)


def _same_compact(want, got, what):
    c_ref, b_ref, _ = want
    counts, ids = got
    assert np.array_equal(counts, c_ref), f"{what}: counts differ at windows {np.flatnonzero((counts != c_ref).any(axis=1))[:10]}"
    mask = np.arange(b_ref.shape[-1])[None, None, :] < c_ref[:, :, None]
    assert np.array_equal(ids, b_ref[mask]), f"{what}: ids differ"


def _two_pass(form):
    return form.startswith("two-pass")


@pytest.mark.parametrize("flt", FORMS, indirect=True)
def test_map_windows_calls(world, flt, request):
    """bmf_map_windows, bmf_map_windows_compact and bmf_map_text_windows_compact share the context's two map slots: the five
    steps through each of them, and then the five steps with the way in changing from step to step.  Stale: the slots' window
    views, row-id lists, counters, counts, dense ids, offsets and compacted ids (a rejected window writes count 0 for both
    orientations and no ids; a window at exactly S - F writes 0 where big's window 4 left a count), the two-pass forms' queue,
    live chunks and fold scratch."""
    def text(w):
        return (np.concatenate([w[0], w[1]]), w[2], w[2] + np.uint64(len(w[0])), w[3])

    def run(way, step, what):
        w, want = world["batch"][step], world["want"][step]
        if way == 0:
            _same_dense(want, flt.map_windows(*w), what)
        elif way == 1:
            _same_compact(want, flt.map_windows_compact(*w), what)
        else:
            _same_compact(want, flt.map_text_windows_compact(*text(w)), what)
    form = request.node.callspec.params["flt"]
    for way in range(3):
        for k, step in enumerate(STEPS):
            run(way, step, f"{form}, way {way}, step {k} ({step})")
    for k, step in enumerate(STEPS):
        run((k + 1) % 3, step, f"{form}, ways in turn, step {k} ({step})")


@pytest.mark.parametrize("flt", FORMS, indirect=True)
def test_batches(world, flt, request):
    """Device-resident batches on one context: each of the five steps a batch of its own, run twice (the second run finds the
    first one's counts, ids and queue in the batch's buffers); then two live batches, big and small, run b1, run b2, download
    b1, download b2, and the same with small first -- what a run keeps in the CONTEXT (row order, fold and queue scratch) must
    not leak into the other batch.  The two-pass forms: pass2_counts() after the small run counts the small run only."""
    form = request.node.callspec.params["flt"]
    for k, step in enumerate(STEPS):
        b = flt.batch(*world["batch"][step])
        for again in range(2):
            b.run()
            _same_dense(world["want"][step], b.download(), f"{form}, step {k} ({step}), run {again}")
            assert b.rows_anded() == world["want"][step][2], f"{form}, step {k} ({step}), run {again}: rows_anded"
            if _two_pass(form) and step == "small":
                recounted, slow = b.pass2_counts()
                assert recounted + slow <= 2 * 5, (form, k, recounted, slow)
        b.close()
    for first, second in (("big", "small"), ("small", "big"), ("big", "empty")):
        b1, b2 = flt.batch(*world["batch"][first]), flt.batch(*world["batch"][second])
        for again in range(2):
            b1.run()
            b2.run()
            if _two_pass(form) and second == "small":
                recounted, slow = b2.pass2_counts()
                assert recounted + slow <= 2 * 5, (form, first, second, recounted, slow)
            _same_dense(world["want"][first], b1.download(), f"{form}, {first} beside {second}, run {again}: the first")
            _same_dense(world["want"][second], b2.download(), f"{form}, {first} beside {second}, run {again}: the second")
            assert b1.rows_anded() == world["want"][first][2] and b2.rows_anded() == world["want"][second][2], (form, first, second)
        b1.close()
        b2.close()


@pytest.mark.parametrize("nb", [100, NB])
def test_a_smaller_index_after_the_fold_table(nb, monkeypatch):
    """reset() and load_index of an index with fewer rows (a quarter of the q-grams) on a context that held the two-pass fold
    table of a full one: the folded rows, the row order and the pass-1 choice are the new index's -- the oracle's answers,
    and a fresh context's.  (NB belongs to the context, so the smaller NB is a context of its own: NB = 100 and 2 049.)"""
    import bucket_map_amd as bma
    rng = np.random.default_rng(20260202 + nb)
    env = {"BMF_PASS1_ROWS": "1", "BMF_MAX_LIVE": "16", "BMF_FOLD": "2", "BMF_FOLD_ROWS": "2"}
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    kw = _kw(nb, bma.BMF_FLAG_EARLY_EXIT)
    first, second = kl.mixed_index(rng, nb, Q, G, 1.0), kl.mixed_index(rng, nb, Q, G, 0.25)
    assert len(second[0]) < len(first[0]) // 2
    windows = kl.random_windows(rng, 1500, READ_LEN, K)
    want_first, want = kl.oracle_run(*first, windows, **kw), kl.oracle_run(*second, windows, **kw)
    assert not np.array_equal(want_first[0], want[0]) and (want[0] > 0).any()
    flt = kl.new_filter(*first, env=env, **kw)
    assert flt.info()["pass1_fold"] == 2
    got = kl.run_batch(flt, windows)
    _same_dense(want_first, got, f"NB = {nb}, the first index")
    flt.reset()
    flt.load_index(*second)
    assert flt.info()["pass1_fold"] == 2 and flt.info()["pass1_rows"] == 1
    fresh = kl.new_filter(*second, env=env, **kw)
    for name, f in (("reloaded", flt), ("fresh", fresh)):
        got = kl.run_batch(f, windows)
        _same_dense(want, got, f"NB = {nb}, the second index, {name}")
        assert got[2] == want[2], f"NB = {nb}, {name}: rows_anded"
        _same_dense(want, f.map_windows(*windows), f"NB = {nb}, the second index through map_windows, {name}")
    flt.close()
    fresh.close()
