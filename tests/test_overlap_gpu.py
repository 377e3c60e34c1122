"""The overlap pass on the GPU (bmv_overlap, include/bmv.h): every output array against overlap_rule.overlap, the plain-Python
rule pinned on hand-worked cases in test_overlap.py, for hand-planted pairs at the shapes where the walks can go wrong -- the
cut at lane 0, at lane 63, on a 64-column step boundary, in the last partial step, inside a run carried across steps, beside
and inside I and D entries, CIGARs of more than 64 entries, one M entry of 100 000 columns -- in all four strand combinations,
with the mates far apart in a permuted batch, unpaired alignments and empty CIGARs between them, under the scores (0, 0),
(1, 2) and (1024, 1); the two identities, the invariants, the refusals and the reused context."""
import ctypes as C

import numpy as np
import pytest

import overlap_rule
from overlap_rule import NO_MATE
from test_annotate import D, EQ, I, X, pack
from test_annotate_gpu import _Batch, _plant, _unpack, _verifier, genome  # noqa: F401  (the last is a fixture)
from test_clip import S

SCORES = ((0, 0), (1, 2), (1024, 1))
STRANDS = ((0, 0), (0, 1), (1, 0), (1, 1))
MANY = [(EQ, 3), (I, 1), (EQ, 2), (X, 1), (D, 1)] * 40 + [(EQ, 4)]      # 201 entries, 401 columns, 361 reference bases


class _Recorder:
    """Takes _plant's b.add and keeps the arguments: the batch is put together after the alignments are permuted."""
    def __init__(self):
        self.last = None

    def add(self, q, start, width, rc):
        self.last = (np.asarray(q, np.uint8), start, width, rc)


def _place(rng, genome, fwd_spec, rc, at, exact=False):
    """One alignment whose FORWARD-strand columns are fwd_spec and whose first column lies at genome position `at`.
    Returns (q, start, width, rc, begin, cigar)."""
    lead, tail = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    lead = min(lead, at)
    rec = _Recorder()
    if rc:
        begin, cigar = _plant(rng, genome, rec, fwd_spec[::-1], 1, begin=tail, end_slack=lead, start=at - lead, exact=exact)
    else:
        begin, cigar = _plant(rng, genome, rec, fwd_spec, 0, begin=lead, end_slack=tail, start=at - lead, exact=exact)
    return (*rec.last, begin, cigar)


def _ref(spec):
    return sum(n for op, n in spec if op != I)


def _pair_cases():
    """(first's forward columns, second's, o): the second's first column lies o reference bases before the first's end
    (o <= 0: a gap).  Which of the two the rule calls `first` follows from the base ranges, not from this order."""
    cases = []
    for n1 in (64, 100, 128, 191):
        for o in (1, 2, 3, 63, 64, 65):
            if o <= n1:
                cases.append(([(EQ, n1)], [(EQ, 150)], o))
    cases += [([(EQ, 128)], [(EQ, 150)], o) for o in (126, 127, 128)]              # r' = l' = 64: on the step boundary
    cases += [([(EQ, 200)], [(EQ, 130)], o) for o in (8, 9, 10, 127, 129)]         # the cut in the first's last partial step
    for o in (5, 40, 64, 100, 130):                                                # runs carried across steps, X at the cut
        cases.append(([(EQ, 60), (X, 10), (EQ, 120)], [(X, 3), (EQ, 50), (X, 30), (EQ, 100)], o))
        cases.append(([(EQ, 30), (X, 100), (EQ, 60)], [(EQ, 10), (X, 70), (EQ, 90)], o))
    for o in range(88, 118, 1):                                                    # the cut beside and inside the first's D / I
        cases.append(([(EQ, 50), (D, 6), (EQ, 50)], [(EQ, 120)], o))
    for o in range(92, 108, 1):
        cases.append(([(EQ, 50), (I, 6), (EQ, 50)], [(EQ, 120)], o))
    for o in range(30, 62, 1):                                                     # ... and the second's
        cases.append(([(EQ, 100)], [(EQ, 20), (D, 5), (EQ, 100)], o))
        cases.append(([(EQ, 100)], [(EQ, 20), (I, 5), (EQ, 100)], o))
    for o in (1, 2, 7, 100, 180, 181, 182, 183, 300, 361):                         # more than 64 entries on either side
        cases.append((MANY, MANY, o))
        cases.append((MANY, [(EQ, 400)], o))
        cases.append(([(EQ, 380)], MANY, o))
    cases += [
        ([(EQ, 200)], [(EQ, 50)], 120),                                            # containment
        ([(EQ, 100)], [(EQ, 100)], 0), ([(EQ, 100)], [(EQ, 100)], -7),             # adjacent, disjoint
        ([(EQ, 100)], [(EQ, 120)], 100),                                           # equal G0: the index decides
        ([(EQ, 100)], [(EQ, 100)], 100),                                           # the same span
        ([(X, 30)], [(EQ, 100)], 10), ([(EQ, 100)], [(X, 30)], 10),                # an empty base range under scores
        ([(X, 5), (EQ, 1), (X, 5)], [(X, 5), (EQ, 40)], 11),                       # scores: both begin at one G0, o = 1: no column
        ([(I, 3), (D, 10), (EQ, 5)], [(EQ, 50)], 13),                              # no scores: nothing of the first lies below m
        ([(EQ, 50)], [(EQ, 5), (D, 30), (I, 2)], 20),                              # ... nothing of the second from m on
        ([(EQ, 40), (D, 5)], [(EQ, 60)], 4), ([(EQ, 40), (I, 5)], [(I, 4), (EQ, 60)], 6),   # I / D at the ends, no scores
        ([(X, 3), (I, 2), (EQ, 90), (D, 3), (X, 2)], [(X, 2), (D, 2), (EQ, 80), (I, 3)], 30),
    ]
    return cases


def _build(genome, seed=71, big=True):
    """The batch: (batch args, begins, cigar_offset, cigars, mate, contig) and the rule's alignments, permuted."""
    rng = np.random.default_rng(seed)
    alns, mate, contig = [], [], []                              # in planting order

    def pair(first, second, o, strands, at, contigs=(0, 0), exact=False):
        a = len(alns)
        alns.append(_place(rng, genome, first, strands[0], at, exact))
        alns.append(_place(rng, genome, second, strands[1], at + _ref(first) - o, exact))
        mate.extend([a + 1, a])
        contig.extend(contigs)

    def single(spec, rc, at):
        alns.append(_place(rng, genome, spec, rc, at))
        mate.append(NO_MATE)
        contig.append(0)

    def empty(qlen):
        alns.append((rng.choice(list(b"ACGT"), qlen).astype(np.uint8), int(rng.integers(0, 100_000)), 40, int(rng.integers(0, 2)), 0, []))
        mate.append(NO_MATE)
        contig.append(0)

    at = 50
    for k, (first, second, o) in enumerate(_pair_cases()):
        for strands in STRANDS if (first is not MANY and second is not MANY) or o in (7, 181) else STRANDS[1:3]:
            pair(first, second, o, strands, at)
            at = 50 + (at + 137) % 190_000
        if k % 5 == 0:
            single([(X, 2), (EQ, 70), (I, 2), (EQ, 30), (X, 1)], k & 1, at)        # unpaired alignments between the pairs
        if k % 17 == 0:
            empty(30 if k % 34 else 0)
    pair([(EQ, 100)], [(EQ, 100)], 50, (0, 1), 1000, contigs=(0, 1))               # on two contigs
    pair([(EQ, 100)], [(EQ, 100)], 50, (0, 1), 1000, contigs=(3, 3))               # the same on one, not contig 0
    a = len(alns)                                                                  # a pair of two empty CIGARs
    empty(20)
    empty(0)
    mate[a], mate[a + 1] = a + 1, a
    if big:                                                                        # one M entry of 100 000 columns each
        pair([(EQ, 60_000), (X, 1), (EQ, 39_999)], [(EQ, 100_000)], 70_001, (0, 1), 10, exact=True)
    n = len(alns)
    order = rng.permutation(n)                                   # new index k holds planted alignment order[k]
    where = np.empty(n, np.int64)
    where[order] = np.arange(n)
    b, begins, cigars = _Batch(), [], []
    for k in order:
        q, start, width, rc, begin, cigar = alns[k]
        b.add(q, start, width, rc)
        begins.append(begin)
        cigars.append(cigar)
    mt = np.array([NO_MATE if mate[k] == NO_MATE else where[mate[k]] for k in order], np.uint32)
    ct = np.array([contig[k] for k in order], np.uint32)
    off = np.concatenate([[0], np.cumsum([len(c) for c in cigars])]).astype(np.uint64)
    cg = np.concatenate([pack(c) for c in cigars] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    batch = b.args()
    rule_alns = [(bytes(genome[int(batch[1][a]): int(batch[1][a]) + int(batch[2][a])]), int(batch[3][a]),
                  bytes(batch[0][int(batch[4][a]): int(batch[4][a]) + int(batch[5][a])]), begins[a], cigars[a], int(batch[1][a]))
                 for a in range(n)]
    return batch, begins, off, cg, mt, ct, rule_alns


_CACHE = {}


def _case(genome, big=True):
    """The planted batch and the rule's answer per pair of scores, computed once and shared."""
    if big not in _CACHE:
        built = _build(genome, big=big)
        want = {s: overlap_rule.overlap(built[6], [int(x) for x in built[4]], [int(x) for x in built[5]], *s) for s in SCORES}
        _CACHE[big] = (built, want)
    return _CACHE[big]


def _entries(got, a):
    xo, ro = got["xcigar_offset"], got["ref_offset"]
    return _unpack(got["xcigar"][int(xo[a]): int(xo[a + 1])]), bytes(got["ref_bases"][int(ro[a]): int(ro[a + 1])])


def _assert_overlapped(got, want, info, batch, what):
    """Every array, every element, and the totals."""
    from bucket_map_amd import verify
    n = len(want)
    xo, ro = got["xcigar_offset"], got["ref_offset"]
    assert all(len(got[k]) == n for k in ("score", "clip_left", "clip_right", "nm", "pos", "ref_len", "cut")) and len(xo) == len(ro) == n + 1
    assert got["score"].dtype == np.int64
    assert xo[0] == 0 and ro[0] == 0 and xo[n] == len(got["xcigar"]) and ro[n] == len(got["ref_bases"]), what
    for a, w in enumerate(want):
        g_xc, g_ref = _entries(got, a)
        g = dict(score=int(got["score"][a]), clip_left=int(got["clip_left"][a]), clip_right=int(got["clip_right"][a]),
                 pos=int(got["pos"][a]), ref_len=int(got["ref_len"][a]), nm=int(got["nm"][a]), xcigar=g_xc, ref_bases=g_ref,
                 cut=int(got["cut"][a]))
        assert g == {k: w[k] for k in g}, f"{what}: alignment {a} differs from the rule ({info['role'][a]}, m = {info['m'][a]})"
        assert all(p[0] != q[0] for p, q in zip(g_xc, g_xc[1:])), f"{what}: alignment {a} has adjacent entries of one op"
        assert verify.md_string(got["xcigar"][int(xo[a]): int(xo[a + 1])], g_ref) == w["md"], f"{what}: MD of alignment {a}"
        if g_xc:
            assert sum(n_ for op, n_ in g_xc if op in (S, EQ, X, I)) == int(batch[5][a]), f"{what}: alignment {a} loses query bases"
        assert g["pos"] + g["ref_len"] <= int(batch[2][a]), f"{what}: alignment {a} leaves its window"
    assert (got["pairs_cut"], got["bases_cut"]) == (info["pairs_cut"], info["bases_cut"]), what


@pytest.mark.gpu
@pytest.mark.parametrize("scores", SCORES, ids=[f"{m}-{p}" for m, p in SCORES])
def test_planted_pairs(genome, scores):
    """Some thousand planted alignments, the mates far apart: every output array is the rule's, and the rule's invariants
    hold on the device's numbers."""
    (batch, begins, off, cg, mt, ct, _), want = _case(genome)
    recs, info = want[scores]
    assert info["pairs_cut"] > 300 and sum(r is None for r in info["role"]) > 50, "the planted batch shows little"
    v = _verifier()
    v.load_genome(genome)
    got = v.overlap(*batch, begins, off, cg, mt, ct, match=scores[0], penalty=scores[1])
    st = v.overlap_stats()
    v.close()
    assert st["columns"] == int((cg >> 4).sum()) and st["ms_kernels"] > 0
    _assert_overlapped(got, recs, info, batch, f"planted, scores {scores}")
    # the invariants, on what the device returned
    g_lo = batch[1].astype(np.int64) + got["pos"].astype(np.int64)
    g_hi = g_lo + got["ref_len"].astype(np.int64)
    cut_pairs = 0
    for a in range(len(mt)):
        xc, _ = _entries(got, a)
        if xc:
            assert int(got["clip_left"][a]) + sum(n for op, n in xc if op in (EQ, X, I)) + int(got["clip_right"][a]) == int(batch[5][a])
        if info["role"][a] != "first":
            assert info["role"][a] is not None or got["cut"][a] == 0
            continue
        b, m = int(mt[a]), info["m"][a]
        cut_pairs += 1
        assert g_hi[a] <= m <= g_lo[b], f"pair ({a}, {b}): the kept intervals [{g_lo[a]}, {g_hi[a]}) and [{g_lo[b]}, {g_hi[b]}) and m = {m}"
        assert g_lo[a] == info["G0"][a] and g_hi[b] == info["G1"][b], f"pair ({a}, {b}): an outer end moved"
        kept_a, kept_b = [e for e in _entries(got, a)[0] if e[0] != S], [e for e in _entries(got, b)[0] if e[0] != S]
        assert kept_a[-1][0] in (EQ, X) and kept_b[0][0] in (EQ, X), f"pair ({a}, {b}): a kept range meets the cut on I or D"
    assert cut_pairs == got["pairs_cut"]


@pytest.mark.gpu
def test_identities(genome):
    """Without mates and with scores: Verifier.clip's arrays exactly.  Without mates and without scores: Verifier.annotate's."""
    (batch, begins, off, cg, mt, ct, _), _ = _case(genome)
    none = np.full(len(mt), NO_MATE, np.uint32)
    v = _verifier()
    v.load_genome(genome)
    for match, penalty in ((1, 2), (1024, 1), (3, 1024)):
        clip = v.clip(*batch, begins, off, cg, match=match, penalty=penalty)
        got = v.overlap(*batch, begins, off, cg, none, ct, match=match, penalty=penalty)
        for k, x in clip.items():
            assert got[k].dtype == x.dtype and np.array_equal(got[k], x), (k, match, penalty)
        assert not got["cut"].any() and got["pairs_cut"] == got["bases_cut"] == 0
    nm, pos, ref_len, xo, xc, ro, rb = v.annotate(*batch, begins, off, cg)
    got = v.overlap(*batch, begins, off, cg, none, None, match=0, penalty=0)
    v.close()
    for k, x in dict(nm=nm, pos=pos, ref_len=ref_len, xcigar_offset=xo, xcigar=xc, ref_offset=ro, ref_bases=rb).items():
        assert got[k].dtype == x.dtype and np.array_equal(got[k], x), k
    assert not got["score"].any() and not got["clip_left"].any() and not got["clip_right"].any() and not got["cut"].any()
    assert not ((got["xcigar"] & 15) == S).any()


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(genome):
    from bucket_map_amd import verify
    (batch, begins, off, cg, mt, ct, _), want = _case(genome, big=False)
    recs, info = want[(1, 2)]
    n = len(mt)
    v = _verifier()
    v.load_genome(genome)
    _assert_overlapped(v.overlap(*batch, begins, off, cg, mt, ct), recs, info, batch, "before the refusals")
    paired = np.flatnonzero(mt != NO_MATE)
    a, single = int(paired[0]), int(np.flatnonzero(mt == NO_MATE)[0])

    def refused(what, names, **kw):
        args = dict(batch=batch, begins=begins, off=off, cg=cg, mate=mt, contig=ct, match=1, penalty=2)
        args.update(kw)
        with pytest.raises(verify.BmvError) as e:
            v.overlap(*args["batch"], args["begins"], args["off"], args["cg"], args["mate"], args["contig"], match=args["match"],
                      penalty=args["penalty"])
        assert e.value.code == 1 and names in str(e.value), (what, str(e.value))

    for match, penalty in ((0, 1), (1, 0), (1025, 1), (1, 1025)):
        refused("scores", "1..1024", match=match, penalty=penalty)
    bad = mt.copy(); bad[a] = n
    refused("a mate beyond the batch", f"alignment {a}", mate=bad)
    bad = mt.copy(); bad[a] = a
    refused("its own mate", f"alignment {a}", mate=bad)
    bad = mt.copy(); bad[single] = a                              # a's mate names another
    refused("a mate that names another", f"alignment {single}", mate=bad)
    ts = batch[1].copy(); ts[5] = 2 ** 62
    refused("text_start at 2^62", "alignment 5", batch=(batch[0], ts, *batch[2:]))
    k = next(i for i in range(n) if off[i + 1] > off[i])          # bmv_clip's checks: an entry of length 0
    c2 = cg.copy(); c2[int(off[k])] &= 15
    refused("a zero-length entry", f"alignment {k}", cg=c2)
    b2 = np.array(begins, np.uint32); b2[k] = batch[2][k]
    refused("past the window", f"alignment {k}", begins=b2)
    _assert_overlapped(v.overlap(*batch, begins, off, cg, mt, ct), recs, info, batch, "after the refusals")
    got = v.overlap(np.zeros(0, np.uint8), [], [], [], [], [], [], [0], [], [])                             # n == 0 is fine
    assert got["xcigar_offset"].tolist() == [0] and len(got["score"]) == 0 and got["pairs_cut"] == 0
    v.close()


@pytest.mark.gpu
def test_a_reused_context_and_the_other_rows(genome):
    """After a larger batch the call gives a smaller one's results unchanged, and it leaves untouched what results, clipped,
    annotations and pairs return."""
    from bucket_map_amd import verify
    (big, big_begins, big_off, big_cg, big_mt, big_ct, _), _ = _case(genome)
    (batch, begins, off, cg, mt, ct, _), want = _case(genome, big=False)
    assert len(big_mt) > len(mt) and len(big_cg) > len(cg)
    v = _verifier()
    v.load_genome(genome)
    some = np.flatnonzero(batch[5] > 0)[:40]
    few = tuple(x[some] for x in batch[1:])
    results = v.align(batch[0], *few)
    annotations = v.annotate(batch[0], *few, *results[1:])
    clipped = v.clip(batch[0], *few, *results[1:])
    pairs = v.pair(few[0], few[1], few[2], few[4], np.zeros(40, np.uint32), few[1], np.arange(0, 41, 10, dtype=np.uint32), 0, 1000)
    stats = (v.stats(), v.annotate_stats(), v.clip_stats())
    v.overlap(*big, big_begins, big_off, big_cg, big_mt, big_ct)
    for scores in SCORES:
        recs, info = want[scores]
        got = v.overlap(*batch, begins, off, cg, mt, ct, match=scores[0], penalty=scores[1])
        _assert_overlapped(got, recs, info, batch, f"after a larger batch, scores {scores}")
    L = verify.lib()
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    s2, b2, o2, c2 = np.zeros(40, np.int32), np.zeros(40, np.uint32), np.zeros(41, np.uint64), np.zeros(max(len(results[3]), 1), np.uint32)
    assert L.bmv_results(v._h, p(s2, C.c_int32), p(b2, C.c_uint32), p(o2, C.c_uint64), p(c2, C.c_uint32)) == 0
    assert all(np.array_equal(x, y) for x, y in zip((s2, b2, o2, c2[: len(results[3])]), results)), "overlap changed bmv_results"
    again = [np.zeros(max(len(x), 1), x.dtype) for x in annotations]
    assert L.bmv_annotations(v._h, p(again[0], C.c_uint32), p(again[1], C.c_uint32), p(again[2], C.c_uint32), p(again[3], C.c_uint64),
                             p(again[4], C.c_uint32), p(again[5], C.c_uint64), p(again[6], C.c_uint8)) == 0
    assert all(np.array_equal(x[: len(y)], y) for x, y in zip(again, annotations)), "overlap changed bmv_annotations"
    sc, le, ri, nm, po, rl = np.zeros(40, np.int64), *(np.zeros(40, np.uint32) for _ in range(5))
    xo, ro = np.zeros(41, np.uint64), np.zeros(41, np.uint64)
    xc, rb = np.zeros(max(len(clipped["xcigar"]), 1), np.uint32), np.zeros(max(len(clipped["ref_bases"]), 1), np.uint8)
    assert L.bmv_clipped(v._h, p(sc, C.c_int64), p(le, C.c_uint32), p(ri, C.c_uint32), p(nm, C.c_uint32), p(po, C.c_uint32),
                         p(rl, C.c_uint32), p(xo, C.c_uint64), p(xc, C.c_uint32), p(ro, C.c_uint64), p(rb, C.c_uint8)) == 0
    again = dict(score=sc, clip_left=le, clip_right=ri, nm=nm, pos=po, ref_len=rl, xcigar_offset=xo, xcigar=xc[: len(clipped["xcigar"])],
                 ref_offset=ro, ref_bases=rb[: len(clipped["ref_bases"])])
    assert all(np.array_equal(again[k], clipped[k]) for k in clipped), "overlap changed bmv_clipped"
    assert all(np.array_equal(x, y) for x, y in zip(v._pairs(4).values(), pairs.values())), "overlap changed bmv_pairs"
    assert (v.stats(), v.annotate_stats(), v.clip_stats()) == stats
    v.close()
