"""The locator on a REUSED context, after a larger batch (include/bml.h): bml_locate, bml_sample_windows and
bml_sample_text_windows each run big, small, n = 0, small, big on one context, every answer held against the oracle
(oracle.oracle_c, bit for bit) and the statistics against the same call on a fresh context.

The context keeps its buffers and clears only occ_count and n_heavy between calls.  After a big call in repeats -- heavy
candidates, occurrences far beyond the budget, so the scan goes in groups -- the candidate counts, the segment ends, the
heavy queue and the occurrence buffer hold plausible leftovers exactly where the three candidates of small sit, one of which
has no occurrence at all and must write offset -1 and 0 votes itself.  The sample kernel after 2 000 windows of 300 bases
meets a window of exactly k bases, one with exactly one good k-mer, one with none and one shorter than k (rejected: it
writes has = 0 and nothing else)."""
import numpy as np
import pytest

from oracle import oracle_c as oc
from test_locator import LETTERS, _sample_case, make_case, oracle

pytestmark = pytest.mark.gpu

STEPS = ("big", "small", "empty", "small", "big")
BUDGET = 20_000


def _joined(rng):
    """Three buckets of a 97-base motif (every sampled k-mer occurs some eighty times a bucket) beside three random ones: the
    cases "tandem repeats" and "random genome" of test_locator.py in one genome, 2 100 candidates in all."""
    a = make_case(rng, n_buckets=3, bucket_len=8192, read_len=150, n_reads=400, motif=97)
    b = make_case(rng, n_buckets=3, bucket_len=8192, read_len=150, n_reads=300)
    cat = lambda key, shift=0: np.concatenate([a[key], b[key] + b[key].dtype.type(shift)])             # noqa: E731
    return dict(genome=cat("genome"), bstart=cat("bstart", len(a["genome"])), blen=cat("blen"), sh=cat("sh"), sp=cat("sp"), sl=cat("sl"),
                pb=cat("pb", 3), pw=cat("pw", len(a["sl"])), pr=cat("pr"), k=a["k"], p=a["p"]), len(a["pb"])


def _only(case, idx):
    """the candidates idx of a case with the windows they name, renumbered"""
    windows, pw = np.unique(case["pw"][idx], return_inverse=True)
    return {**case, "sh": case["sh"][windows], "sp": case["sp"][windows], "sl": case["sl"][windows], "pb": case["pb"][idx],
            "pw": pw.astype(np.uint32), "pr": case["pr"][idx]}


@pytest.fixture(scope="module")
def world():
    big, n_repeats = _joined(np.random.default_rng(20260301))
    assert len(big["pb"]) == 2100 and (np.diff(big["pb"].astype(np.int64)) >= 0).all()
    o_big, v_big = oracle(big)
    # small: two candidates the oracle places and one without any occurrence, all in the random buckets
    rest = np.arange(n_repeats, len(big["pb"]))
    placed, none = rest[o_big[rest] >= 0][[0, -1]], rest[v_big[rest] == 0][:1]
    assert len(none) == 1 and o_big[none[0]] == -1
    small = _only(big, np.sort(np.concatenate([placed, none])))
    o_small, v_small = oracle(small)
    assert sorted(v_small.tolist())[0] == 0 and (o_small >= 0).sum() == 2 and len(o_small) == 3
    empty = _only(big, np.zeros(0, np.int64))
    return {"case": {"big": big, "small": small, "empty": empty},
            "want": {"big": (o_big, v_big), "small": (o_small, v_small), "empty": (np.zeros(0, np.int32), np.zeros(0, np.uint32))}}


def _scanner(case):
    from bucket_map_amd import locate
    s = locate.LocatorScan(case["k"], case["p"], 4, 6, int(case["blen"].max()))
    s.load_genome(case["genome"], case["bstart"], case["blen"])
    return s


def _locate(s, case):
    """(offsets, votes, the count fields of stats(), count_histogram()) of one call"""
    off, votes = s.locate(case["sh"], case["sp"], case["sl"], case["pb"], case["pw"], case["pr"])
    st = {k: x for k, x in s.stats().items() if not k.startswith("ms")}
    return off, votes, st, s.count_histogram(len(case["pb"]))


def test_locate(world, monkeypatch):
    """bml_locate.  Stale: cand_count, samp_end and cand_start (the counts and segment ends of 2 100 candidates: the candidate
    without occurrences must count 0 and own an empty segment), heavy and its queue (n_heavy is cleared, the queue's entries are
    not), the occurrence buffer and its groups, out_offset and out_votes (-1 and 0 are written by the replay, not left from a
    memset), chunks.  stats() and count_histogram() are those of the LAST call -- of a call without candidates too: zeros."""
    monkeypatch.setenv("BML_MAX_OCC", str(BUDGET))
    fresh = {}
    for step in ("big", "small", "empty"):
        s = _scanner(world["case"]["big"])
        fresh[step] = _locate(s, world["case"][step])
        s.close()
    st, (cand, occ) = fresh["big"][2], fresh["big"][3]
    assert st["heavy_candidates"] > 0 and st["occurrences"] > 4 * BUDGET, st          # repeats, and the scan goes in groups
    assert int(cand.sum()) == 2100 and cand[0] > 0
    st, (cand, occ) = fresh["small"][2], fresh["small"][3]
    assert st["heavy_candidates"] == 0 and int(cand.sum()) == 3 and cand[0] == 1 and int(occ.sum()) == st["occurrences"], (st, cand)
    st, (cand, occ) = fresh["empty"][2], fresh["empty"][3]
    assert st == {"occurrences": 0, "heavy_candidates": 0} and not cand.any() and not occ.any()
    s = _scanner(world["case"]["big"])
    for k, step in enumerate(STEPS):
        off, votes, st, (cand, occ) = _locate(s, world["case"][step])
        o_ref, v_ref = world["want"][step]
        bad = np.flatnonzero((off != o_ref) | (votes != v_ref))
        assert bad.size == 0, f"step {k} ({step}): candidates {bad[:5]}: ref {o_ref[bad[:5]]}/{v_ref[bad[:5]]}, got {off[bad[:5]]}/{votes[bad[:5]]}"
        assert st == fresh[step][2], f"step {k} ({step}): stats {st}, on a fresh context {fresh[step][2]}"
        assert np.array_equal(cand, fresh[step][3][0]) and np.array_equal(occ, fresh[step][3][1]), f"step {k} ({step}): count_histogram"
        for x, y in zip((off, votes), fresh[step][:2]):
            assert np.array_equal(x, y), f"step {k} ({step}): differs from a fresh context"
    s.close()


K, P, MINQ = 12, 10, 25 * 12


@pytest.fixture(scope="module")
def windows():
    rng = np.random.default_rng(20260302)
    big = _sample_case(rng, 2000, 300, K)
    texts = [LETTERS[rng.integers(0, 4, n)] for n in (K, 150, 150, K - 1)]
    quals = [np.full(K, 33 + 40, np.uint8), np.full(150, 33, np.uint8), np.full(150, 33, np.uint8), np.full(K - 1, 33 + 40, np.uint8)]
    quals[1][71: 71 + K] = 33 + 25                              # exactly one k-mer sums to MINQ, its neighbours to less
    lens = np.array([len(t) for t in texts], np.uint32)
    small = (np.concatenate(texts), np.concatenate(quals), np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64), lens)
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    batch = {"big": big, "small": small, "empty": empty}
    want = {step: oc.sample_windows(K, P, MINQ, *w) for step, w in batch.items()}
    h, pos, has = want["small"]
    assert has.tolist() == [1, 1, 1, 0] and pos[0].tolist() == [0] * P and pos[1].tolist() == [71] * P
    assert pos[2, 0] == 0 and pos[2, -1] == 150 - K and len(set(pos[2].tolist())) == P          # none good: all are candidates
    assert not h[3].any() and not pos[3].any()
    h, pos, has = want["big"]
    assert has.sum() > 1500 and (has == 0).any() and len(set(pos[:, -1].tolist())) > 50
    return batch, want


def test_sampling(windows):
    """bml_sample_windows and bml_sample_text_windows on one context: the five steps through each, then through both in turn.
    Stale: the sampled hashes and positions of 2 000 windows (a rejected window writes has = 0 and zeros; a window with one good
    k-mer writes that k-mer p times over whatever lay there), the has flags, the window views and the uploaded text."""
    from bucket_map_amd import locate
    batch, want = windows
    scan = locate.LocatorScan(K, P, 4, 6, 70000)

    def run(way, step, what):
        bases, quals, ws, wl = batch[step]
        if way == 0:
            got = scan.sample_windows(bases, quals, ws, wl, MINQ)
        else:
            got = scan.sample_text_windows(np.concatenate([bases, quals]), ws, ws + np.uint64(len(bases)), wl, MINQ)
        for a, b, name in zip(want[step], got, ("hash", "position", "has-samples")):
            assert np.array_equal(a, b), f"{what}: {name} differs at windows {np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8]}"
    for way in (0, 1):
        for k, step in enumerate(STEPS):
            run(way, step, f"way {way}, step {k} ({step})")
    for k, step in enumerate(STEPS):
        run(k % 2, step, f"ways in turn, step {k} ({step})")
    scan.close()
    for step in ("small", "empty"):                            # the same calls on a context of their own
        fresh = locate.LocatorScan(K, P, 4, 6, 70000)
        bases, quals, ws, wl = batch[step]
        for a, b in zip(want[step], fresh.sample_windows(bases, quals, ws, wl, MINQ)):
            assert np.array_equal(a, b), f"{step} on a fresh context"
        fresh.close()
