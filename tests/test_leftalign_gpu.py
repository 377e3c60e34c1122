"""The indel normalisation pass on the GPU (bmv_leftalign, include/bmv.h): begin, entries, changed and dropped of every
alignment, and the four counts of the stats, against test_leftalign.restate_leftalign -- the plain-Python restatement held
there against a second formulation and the hand-worked cases -- for planted CIGARs on windows built so that gaps move far
(the ballot-step borders, merges, gaps that meet, gaps that reach either end, odd letters, both strands), for a 20 000-column
alignment in a satellite whose batch is taken in pieces, after bmv_align and bmv_realign on reads from a low-complexity
genome; idempotence; what the call leaves untouched; that bmv_annotate and bmv_clip take its output; the refusals; and
`bucketmap_align --left-align` against the oracle-backed tool, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from test_annotate import D, I, M, pack
from test_annotate_gpu import LETTERS, _Batch, _revcomp, _unpack, _verifier
from test_leftalign import ARGS, HAND, TOOLS, check_invariants, make_site_job, parse, restate_leftalign
from test_realign_gpu import LENGTHS, _edited, _packed, _snapshot, _views

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GAPS = (1, 2, 3, 7, 63, 64, 65, 200)
BEFORE = (0, 1, 63, 64, 65, 129, 300)
RUNS = (63, 64, 65, 128)                                         # the ballot-step borders


def _assert_leftaligned(v, genome, batch, begins, cigars, what, thorough=False):
    """Verifier.leftalign on the batch: every output of every alignment is the restatement's, the stats are its sums, the
    structural invariants hold, and the output fed back comes out unchanged.  Returns (the device's dict, the restatement's
    dicts)."""
    n = len(cigars)
    off, cg = _packed(cigars)
    got = v.leftalign(*batch, begins, off, cg)
    st = v.leftalign_stats()
    o = got["cigar_offset"]
    assert len(got["begin"]) == len(got["changed"]) == len(got["dropped"]) == n and len(o) == n + 1
    assert o[0] == 0 and o[n] == len(got["cigar"]), f"{what}: the total is not the offsets' end"
    want = []
    for a in range(n):
        window, rc, query = _views(genome, batch, a)
        w = restate_leftalign(window, rc, query, int(begins[a]), cigars[a])
        ops = _unpack(got["cigar"][int(o[a]): int(o[a + 1])])
        g = dict(begin=int(got["begin"][a]), cigar=ops, changed=int(got["changed"][a]), dropped=int(got["dropped"][a]))
        assert g == {k: w[k] for k in g}, f"{what}: alignment {a} (rc = {rc}, begin {begins[a]}, given {cigars[a]}) differs from the restatement"
        assert sum(k for op, k in ops if op != D) == (len(query) if cigars[a] else 0), f"{what}: alignment {a} loses query bases"
        assert g["begin"] + sum(k for op, k in ops if op != I) <= len(window), f"{what}: alignment {a} leaves its window"
        assert all(x[0] != y[0] for x, y in zip(ops, ops[1:])) and not (ops and D in (ops[0][0], ops[-1][0])), f"{what}: alignment {a}"
        assert len(ops) <= len(cigars[a]) + sum(op != M for op, _ in cigars[a]), f"{what}: alignment {a} has too many entries"
        if thorough and cigars[a]:
            check_invariants(window, rc, query, int(begins[a]), cigars[a], w, f"{what}: alignment {a}")
        want.append(w)
    assert st["ms_kernels"] > 0 or n == 0
    assert (st["compared"], st["n_changed"], st["merges"], st["dropped"]) == tuple(
        sum(w[k] for w in want) for k in ("compared", "changed", "merges", "dropped")), f"{what}: the stats are not the restatement's sums"
    again = v.leftalign(*batch, got["begin"], got["cigar_offset"], got["cigar"])
    assert all(np.array_equal(again[k], got[k]) for k in ("begin", "cigar_offset", "cigar")) and not again["changed"].any() \
        and not again["dropped"].any(), f"{what}: the pass is not idempotent"
    assert v.leftalign_stats()["merges"] == 0
    return got, want


class _Planted:
    """Alignments built in the forward view -- ranks of the reference under the path, of the query along the forward strand,
    and forward entries --, laid into a genome of their own with 0..8 bases of slack either side and handed to the batch as
    the aligner would have seen them."""

    def __init__(self, rng):
        self.rng, self.parts, self.at, self.batch, self.begins, self.cigars = rng, [np.zeros(0, np.uint8)], 0, _Batch(), [], []

    def spell(self, ranks, odd):
        if not odd:
            return np.frombuffer(b"ACGT", np.uint8)[np.asarray(ranks, np.int64)]
        return np.array([LETTERS[r][int(self.rng.integers(0, len(LETTERS[r])))] for r in ranks], np.uint8)

    def add(self, ref, query, cigar, rc, odd=False):
        rng = self.rng
        assert sum(k for op, k in cigar if op != I) == len(ref) and sum(k for op, k in cigar if op != D) == len(query)
        left, right = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        window = list(rng.integers(0, 4, left)) + list(ref) + list(rng.integers(0, 4, right))
        self.parts.append(self.spell(window, odd))
        read = [3 - r for r in reversed(query)] if rc else list(query)
        self.batch.add(self.spell(read, odd), self.at, len(window), rc)
        self.at += len(window)
        self.begins.append(right if rc else left)
        self.cigars.append([tuple(e) for e in (reversed(cigar) if rc else cigar)])

    def empty(self):
        self.batch.add(self.spell(self.rng.integers(0, 4, 12), False), max(self.at - 30, 0), min(self.at, 30), int(self.rng.integers(0, 2)))
        self.begins.append(int(self.rng.integers(0, 5)))
        self.cigars.append([])

    def genome(self):
        return np.concatenate(self.parts + [np.frombuffer(b"ACGTACGT", np.uint8)])


def _from_ref(rng, ref, cigar):
    """The query a path reads off a reference: M copies, D skips, I inserts random bases."""
    q, at = [], 0
    for op, k in cigar:
        if op == I:
            q += list(rng.integers(0, 4, k))
        else:
            if op == M:
                q += list(ref[at: at + k])
            at += k
    return q


def _from_query(rng, query, cigar):
    """The reference under a path whose query is given: M copies, I skips, D inserts random bases."""
    r, at = [], 0
    for op, k in cigar:
        if op == D:
            r += list(rng.integers(0, 4, k))
        else:
            if op == M:
                r += list(query[at: at + k])
            at += k
    return r


def _periodic_case(rng, op, L, before, run, period):
    """A gap of L after `before` M columns, the last `run` of them (and the gap) inside a stretch of the given period in the
    sequence the gap compares -- the reference for a D, the query for an I --, the column before the stretch breaking it, so
    that with a period that divides L the gap moves exactly `run` columns."""
    unit = list(rng.integers(0, 4, period))
    if period > 1 and len(set(unit)) == 1:
        unit[0] = (unit[0] + 1) % 4
    seq = list(rng.integers(0, 4, before - run)) + [unit[x % period] for x in range(run + L)] + list(rng.integers(0, 4, 20))
    if before > run:
        seq[before - run - 1] = (seq[before - run - 1 + L] + 1) % 4
    cigar = ([(M, before)] if before else []) + [(op, L), (M, 20)]
    if op == D:
        ref, query = seq, seq[:before] + seq[before + L:]
    else:
        query, ref = seq, seq[:before] + seq[before + L:]
    return ref, query, cigar


def _period_for(rng, L, kind):
    if kind == "equal" or L == 1:
        return L
    if kind == "divides":
        return {2: 1, 3: 1, 7: 1, 63: 9, 64: 16, 65: 13, 200: 25}[L]
    return {2: 3, 3: 2, 7: 4, 63: 10, 64: 3, 65: 4, 200: 7}[L]


@pytest.mark.gpu
def test_planted_gaps_at_the_ballot_borders():
    """Every gap length x every preceding M run x runs of exactly 63, 64, 65 and 128 free columns and the whole M run x a
    period equal to L, dividing L and not dividing L, I and D, strands alternating, a third of the cases spelled with lower
    case, N and IUPAC letters, one query base inside the passed run changed."""
    rng = np.random.default_rng(601)
    P = _Planted(rng)
    exact = []
    for op in (D, I):
        for L in GAPS:
            for before in BEFORE:
                for run in sorted({min(r, before) for r in RUNS} | {before}):
                    for kind in ("equal", "divides", "other"):
                        if L == 1 and kind != "equal":
                            continue
                        period = _period_for(rng, L, kind)
                        ref, query, cigar = _periodic_case(rng, op, L, before, run, period)
                        k = len(P.cigars)
                        if run >= 2 and k % 4 == 0:                  # a mismatch inside the passed run: the gap passes it
                            at = before - 1 - run // 2
                            if op == D:
                                query[at] = (query[at] + 1) % 4
                            else:
                                ref[at] = (ref[at] + 1) % 4
                        P.add(ref, query, cigar, k % 2, odd=k % 3 == 0)
                        if L % period == 0:
                            exact.append((k, op, L, before, run))
    genome, batch = P.genome(), P.batch.args()
    v = _verifier()
    v.load_genome(genome)
    got, want = _assert_leftaligned(v, genome, batch, P.begins, P.cigars, "planted")
    v.close()
    # the cases are what they were built to be: with a period that divides L the gap moved exactly `run` columns
    for k, op, L, before, run in exact:
        rc, w = int(batch[3][k]), want[k]
        ops = w["cigar"][::-1] if rc else w["cigar"]
        if run == before:
            assert ops == ([(M, before + 20)] if op == D else [(I, L), (M, before + 20)]) and w["dropped"] == (L if op == D else 0), (k, ops)
        else:
            assert ops == [(M, before - run), (op, L), (M, run + 20)], (k, op, L, before, run, ops)
    assert len(want) > 700 and sum(w["changed"] for w in want) > 500


def _special_cases(rng, P):
    A, C, G, T = 0, 1, 2, 3
    hom = lambda n: [C] + [A] * (n - 1)                          # a homopolymer behind a C
    for rc in (0, 1):
        for odd in (False, True):
            for mk, other in ((_from_ref, D), (_from_query, I)):
                swap = (lambda c: c) if other == D else (lambda c: [(({D: I, I: D}).get(op, op), k) for op, k in c])

                def add(seq, cigar):
                    cigar = swap(cigar)
                    derived = mk(rng, seq, cigar)
                    P.add(*((seq, derived) if other == D else (derived, seq)), cigar, rc, odd)
                # three gaps that merge in turn, and the merged one moves on to the C
                add(hom(47), [(M, 11), (D, 2), (M, 5), (D, 1), (M, 5), (D, 3), (M, 20)])
                # a stuck 1-gap, a 2-gap that reaches it through (CG)n, and the merged 3-gap moves on through (ACG)n
                add([T] + [A, C, G] * 30 + [A] + [C, G] * 20 + [T] * 5, [(M, 91), (D, 1), (M, 20), (D, 2), (M, 23)])
                # a gap that meets one of the other op, from either side
                add(hom(63), [(M, 20), (I, 2), (M, 10), (D, 3), (M, 30)])
                add(hom(63), [(M, 20), (D, 3), (M, 10), (I, 2), (M, 30)])
                add(hom(40), [(M, 20), (I, 2), (D, 3), (M, 17)])
                # a gap that reaches the start, a leading one, a trailing one, both; with 64 and 65 columns to the start
                add([A] * 37, [(M, 5), (D, 2), (M, 30)])
                add([A] * 96, [(M, 64), (D, 2), (M, 30)])
                add([A] * 97, [(M, 65), (D, 2), (M, 30)])
                add(hom(33), [(D, 3), (M, 30)])
                add(list(rng.integers(0, 4, 34)), [(M, 30), (D, 4)])
                add([A] * 34, [(M, 30), (D, 4)])
                add([A] * 14, [(D, 2), (M, 10), (D, 2)])
                add([A] * 20, [(D, 2), (M, 5), (I, 2), (M, 5), (D, 2), (M, 6)])
                add([A, C] * 40, [(M, 31), (D, 4), (M, 10), (I, 3), (M, 20), (D, 2), (M, 13)])
                # one entry
                add([A], [(M, 1)])
                add([A] * 5, [(D, 5)])
            P.add([], [2], [(I, 1)], rc, odd)
            P.empty()
            for window, query, given, *_ in HAND:
                r = lambda s: ["ACGT".index(chr(c)) for c in s]
                P.add(r(window), r(query), parse(given), rc, odd)


@pytest.mark.gpu
def test_merges_meetings_ends_and_a_mixed_batch():
    """Same-op merges (three gaps in turn; a merge after which the longer gap moves on), I meeting D, gaps that arrive at the
    start, leading and trailing D, one-entry CIGARs, the hand-worked cases and empty CIGARs in one batch, both strands, plain
    and odd letters; then a share of the batch with offsets that do not start at 0."""
    rng = np.random.default_rng(602)
    P = _Planted(rng)
    _special_cases(rng, P)
    genome, batch = P.genome(), P.batch.args()
    v = _verifier()
    v.load_genome(genome)
    got, want = _assert_leftaligned(v, genome, batch, P.begins, P.cigars, "specials", thorough=True)
    assert sum(w["merges"] for w in want) >= 24 and sum(w["dropped"] > 0 for w in want) >= 24
    assert 0 < sum(w["changed"] for w in want) < len(want) - 8 and sum(1 for c in P.cigars if not c) == 4
    first = want[1]                                              # forward strand, plain letters: the merged 3-gap behind the T
    assert first["cigar"] == [(M, 1), (D, 3), (M, 134 - 1)] and first["merges"] == 1
    part = slice(7, 61)
    share = tuple(x[part] for x in batch)[1:]
    off, cg = _packed(P.cigars)
    again = v.leftalign(batch[0], *share, P.begins[part], off[7:62], cg)
    v.close()
    o = again["cigar_offset"]
    for k, a in enumerate(range(7, 61)):
        assert (int(again["begin"][k]), _unpack(again["cigar"][int(o[k]): int(o[k + 1])])) == (want[a]["begin"], want[a]["cigar"]), a


@pytest.mark.gpu
def test_a_satellite_alignment_in_pieces(monkeypatch, capfd):
    """A 20 000-column alignment inside 171-base monomers whose one deleted monomer moves 19 000 columns to the array's start,
    then ten alignments of 20 000 one-column entries each (15 000 reference bases): 30 000 stack words apiece, so that under a scratch of 1 MB the
    batch is taken in two pieces."""
    rng = np.random.default_rng(603)
    P = _Planted(rng)
    monomer = list(rng.integers(0, 4, 171))
    array = [(monomer[170] + 1) % 4] + monomer * 120
    for rc in (0, 1):
        cigar = [(M, 1 + 171 * 111 + 20), (D, 171), (M, 20_000 - (1 + 171 * 111 + 20))]
        ref = array[: 20_000 + 171]
        P.add(ref, _from_ref(rng, ref, cigar), cigar, rc)
    for k in range(10):
        cigar = [(M, 1), (D, 1), (M, 1), (I, 1)] * 5000
        ref = array[100 + k: 100 + k + 15_000]
        P.add(ref, _from_ref(rng, ref, cigar), cigar, k % 2)
    genome, batch = P.genome(), P.batch.args()
    monkeypatch.setenv("BMV_SCRATCH_MB", "1")
    monkeypatch.setenv("BMV_LOG_CLASSES", "1")
    v = _verifier()
    v.load_genome(genome)
    capfd.readouterr()
    got, want = _assert_leftaligned(v, genome, batch, P.begins, P.cigars, "satellite")
    log = capfd.readouterr().err
    v.close()
    assert f"[bmv] leftalign: 12 alignments ({sum(w['changed'] for w in want)} changed) in 2 pieces" in log, log
    assert want[0]["cigar"] == [(M, 1), (D, 171), (M, 19_999)] and want[0]["compared"] == 171 * 111 + 20 + 1
    assert want[1]["cigar"] == [(M, 19_999), (D, 171), (M, 1)]


@pytest.fixture(scope="module")
def repeats():
    """300 000 bases of low complexity: microsatellites of unit 1..6, 5..30 copies, 10..30 random bases between them."""
    rng = np.random.default_rng(20251001)
    bases, parts, size = np.frombuffer(b"ACGT", np.uint8), [], 0
    while size < 300_000:
        unit = bases[rng.integers(0, 4, int(rng.integers(1, 7)))]
        parts += [np.tile(unit, int(rng.integers(5, 31))), bases[rng.integers(0, 4, int(rng.integers(10, 31)))]]
        size += len(parts[-1]) + len(parts[-2])
    return np.concatenate(parts)[:300_000]


def _read_batch(rng, genome):
    b = _Batch()
    for m in LENGTHS:
        for rc in (0, 1):
            for _ in range(3):
                start = int(rng.integers(0, len(genome) - 2 * m - 64))
                q = _edited(rng, genome[start + 6: start + 6 + m + m // 8 + 8], 8)[:m]
                b.add(_revcomp(q) if rc else q, start, m + m // 8 + 20, rc)
    return b


@pytest.mark.gpu
def test_after_the_aligner_and_after_realign(repeats):
    """Edited reads of every length on either strand from the low-complexity genome: bmv_align's paths normalised, and
    bmv_realign's; the output goes into bmv_annotate and bmv_clip, NM is nm_in - dropped, and what bmv_results,
    bmv_realigned, bmv_annotations and bmv_clipped return is the same before and after the call."""
    from bucket_map_amd import verify
    from test_annotate_gpu import _assert_annotations
    from test_annotate_gpu import _expected as expected_annotations
    from test_clip_gpu import _assert_clipped
    from test_clip_gpu import _expected as expected_clipped
    rng = np.random.default_rng(604)
    batch = _read_batch(rng, repeats).args()
    n = len(batch[1])
    v = _verifier()
    v.load_genome(repeats)
    score, begin, off, cg = v.align(*batch)
    ra = v.realign(*batch, begin, off, cg)
    ann = v.annotate(*batch, begin, off, cg)
    cl = v.clip(*batch, begin, off, cg)
    L = verify.lib()

    def realigned():
        arrs = [np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n + 1, np.uint64),
                np.zeros(max(len(ra["cigar"]), 1), np.uint32)]
        assert L.bmv_realigned(v._h, *(x.ctypes.data_as(t) for x, t in zip(arrs, verify.SYMBOLS["bmv_realigned"][1][1:]))) == 0
        return arrs + [v.realign_stats()]
    sizes = (n, len(cg), len(ann[4]), len(ann[6]), len(cl["xcigar"]), len(cl["ref_bases"]))
    before = _snapshot(v, *sizes) + realigned()
    cigars = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in range(n)]
    got, want = _assert_leftaligned(v, repeats, batch, [int(x) for x in begin], cigars, "after bmv_align")
    after = _snapshot(v, *sizes) + realigned()
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(before, after)), \
        "bmv_leftalign changed what another result or stats call returns"
    assert sum(w["changed"] for w in want) >= 8, "hardly any path changed: the batch shows little"
    ann2 = v.annotate(*batch, got["begin"], got["cigar_offset"], got["cigar"])
    _assert_annotations(ann2, expected_annotations(repeats, batch, got["begin"], got["cigar_offset"], got["cigar"]), "annotate after leftalign")
    assert np.array_equal(ann2[0].astype(np.int64), ann[0].astype(np.int64) - got["dropped"]), "NM is not nm_in - dropped"
    cl2 = v.clip(*batch, got["begin"], got["cigar_offset"], got["cigar"])
    _assert_clipped(cl2, expected_clipped(repeats, batch, got["begin"], got["cigar_offset"], got["cigar"], 1, 2), batch, "clip after leftalign")
    # ... and on top of the realignment
    cigars = [_unpack(ra["cigar"][int(ra["cigar_offset"][a]): int(ra["cigar_offset"][a + 1])]) for a in range(n)]
    got, want = _assert_leftaligned(v, repeats, batch, [int(x) for x in ra["begin"]], cigars, "after bmv_realign")
    assert sum(w["changed"] for w in want) >= 4
    ann_ra = v.annotate(*batch, ra["begin"], ra["cigar_offset"], ra["cigar"])
    ann3 = v.annotate(*batch, got["begin"], got["cigar_offset"], got["cigar"])
    v.close()
    assert np.array_equal(ann3[0].astype(np.int64), ann_ra[0].astype(np.int64) - got["dropped"])


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(repeats):
    from bucket_map_amd import verify
    rng = np.random.default_rng(605)
    b = _Batch()
    for _ in range(3):
        start = int(rng.integers(0, 100_000))
        b.add(_edited(rng, repeats[start + 6: start + 400], 8)[:300], start, 320, 0)
    batch = b.args()
    with pytest.raises(verify.BmvError) as e:
        verify.Verifier().leftalign(*batch, np.zeros(3, np.uint32), np.zeros(4, np.uint64), np.zeros(0, np.uint32))
    assert e.value.code == 3                                     # BMV_ERR_STATE: no genome yet
    v = _verifier()
    v.load_genome(repeats)
    score, begin, off, cg = v.align(*batch)
    cigars = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in range(3)]
    good = v.leftalign(*batch, begin, off, cg)
    bad_cigars = {
        "consumes query_len - 1": [(M, 299)],
        "runs past the window": [(M, 300), (D, 21)],
        "a zero-length entry": [(M, 150), (I, 0), (M, 150)],
        "adjacent equal ops": [(M, 150), (M, 150)],
        "an op code of 3": [(M, 150), (3, 2), (M, 150)],
    }
    for what, bad in bad_cigars.items():
        o, c = _packed(cigars[:2] + [bad])
        with pytest.raises(verify.BmvError) as e:
            v.leftalign(*batch, [begin[0], begin[1], 0], o, c)
        assert e.value.code == 1 and "alignment 2" in str(e.value), (what, str(e.value))
    with pytest.raises(verify.BmvError) as e:
        v.leftalign(batch[0], batch[1], batch[2], batch[3], batch[4] + np.uint64(10 ** 9), batch[5], begin, off, cg)
    assert e.value.code == 1 and "alignment 0" in str(e.value)
    again = v.leftalign(*batch, begin, off, cg)
    assert all(np.array_equal(good[k], again[k]) for k in good), "a refusal changed what the next call returns"
    empty = v.leftalign(np.zeros(0, np.uint8), [], [], [], [], [], [], [0], [])                # n == 0 is fine
    assert empty["cigar_offset"].tolist() == [0] and len(empty["begin"]) == 0
    v.close()
    # D lengths, then I lengths, that sum to 2^28: a merged entry would not fit
    half, size = 1 << 27, (1 << 28) + 10
    big = np.full(size + 64, ord("A"), np.uint8)
    v = _verifier()
    v.load_genome(big)
    small = np.full(20, ord("A"), np.uint8)
    o, c = _packed([[(M, 10)], [(M, 3), (D, half), (M, 4), (D, half), (M, 3)]])
    with pytest.raises(verify.BmvError) as e:
        v.leftalign(small, [0, 0], [64, size], [0, 0], [0, 10], [10, 10], [0, 0], o, c)
    assert e.value.code == 5 and "alignment 1" in str(e.value) and "D entries" in str(e.value)
    o, c = _packed([[(M, 10)], [(M, 3), (I, half), (M, 4), (I, half), (M, 3)]])
    with pytest.raises(verify.BmvError) as e:
        v.leftalign(big[:size + 10], [0, 0], [64, 64], [0, 1], [0, 10], [10, size], [0, 0], o, c)
    assert e.value.code == 5 and "alignment 1" in str(e.value) and "I entries" in str(e.value)
    o, c = _packed([[(M, 10)], [(M, 3), (D, 6), (M, 4), (D, 6), (M, 3)]])
    ok = v.leftalign(small, [0, 0], [64, 64], [0, 0], [0, 10], [10, 10], [0, 0], o, c)           # the context stays usable
    v.close()
    assert _unpack(ok["cigar"]) == [(M, 10), (M, 10)] and ok["dropped"].tolist() == [0, 12] and ok["begin"].tolist() == [0, 12]


def _run(exe, d, args, out, *extra, block="17"):
    env = dict(os.environ, BM_VERIFY_BLOCK_READS=block)
    r = subprocess.run([exe, *args, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return (d / out).read_bytes(), r.stderr


@pytest.mark.gpu
def test_the_tool_against_the_oracle_backed_tool(tmp_path):
    """bucketmap_align --left-align writes, byte for byte, what the oracle-backed tool writes through the host restatement
    (host/left_align.h) -- alone, after --affine, under --best with other scores, with --clip, and from two contexts; without
    the option the pass does not run."""
    make_site_job(tmp_path)
    gpu = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    for k, extra in enumerate((["--left-align"], ["--affine", "--left-align"], ["--best", "--affine-scores", "2,3,5,2", "--left-align"])):
        cpu, _ = _run(TOOLS["bucketmap_align"], tmp_path, ARGS, f"cpu{k}.sam", *extra)
        got, err = _run(gpu, tmp_path, ARGS, f"gpu{k}.sam", *extra)
        assert "GPU indel normalisation" in err and got == cpu and got.count(b"3D") >= 14, extra
    two, _ = _run(gpu, tmp_path, ARGS, "gpu_two.sam", "--affine", "--left-align", "--gpus", "0,0")
    assert two == (tmp_path / "gpu1.sam").read_bytes()
    clipped, err = _run(gpu, tmp_path, ARGS, "gpu_clip.sam", "--affine", "--left-align", "--clip")
    assert "GPU indel normalisation" in err and clipped.count(b"AS:i:") == clipped.count(b"NM:i:") > 0
    plain, err = _run(gpu, tmp_path, ARGS, "gpu_plain.sam", "--affine")
    assert "GPU indel normalisation" not in err and plain != two


@pytest.mark.gpu
def test_the_tool_on_top_of_rescue_and_affine(tmp_path):
    """--rescue --affine --left-align: the picks and the rescued mates normalised on the device, byte for byte the
    oracle-backed tool's records."""
    from test_pair import ARGS as PAIR_ARGS
    from test_rescue import N_LOST, make_rescue_fixture
    make_rescue_fixture(tmp_path)
    gpu = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    args = [*PAIR_ARGS, "-q", "lost.fastq", "--rescue", "--affine", "--left-align"]
    cpu, _ = _run(TOOLS["bucketmap_align"], tmp_path, args, "cpu.sam", block="6")
    got, err = _run(gpu, tmp_path, args, "gpu.sam", block="6")
    assert "GPU indel normalisation" in err and "GPU affine realignment" in err and "GPU mate rescue" in err
    assert got == cpu and got.count(b"XR:i:1") >= N_LOST and got.count(b"AS:i:") == got.count(b"NM:i:") > 0
