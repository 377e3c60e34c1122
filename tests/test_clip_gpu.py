"""The clipping pass on the GPU (bmv_clip, include/bmv.h): score, clips, pos, ref_len, nm, entries with S and the reference
bases of the kept part, for hand-planted CIGARs at the shapes where the wave-wide range search can go wrong, for one long M
entry, for prefix sums beyond 2^31, and for what align / align_long / align_bounded return; its relation to bmv_annotate;
the refusals; and `bucketmap_align --clip`, whose records are derived again in Python from the --annotate run's.

Expected values come from test_clip.restate_clip, the plain-Python restatement pinned on hand-worked cases there."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from test_annotate import D, EQ, I, M, X, pack
from test_annotate_gpu import (_Batch, _check_annotated, _fasta, _fastq, _mutate, _plant, _records, _revcomp, _simulated, _tool,
                               _unpack, _verifier, genome, plain_genome)  # noqa: F401  (the last two are fixtures)
from test_clip import S, range_scan, restate_clip

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SCORES = ((1, 1), (1, 2), (1024, 1), (1, 1024))


def _expected(genome, batch, begin, off, cg, match, penalty):
    reads, ts, tl, trc, qs, ql = batch
    return [restate_clip(bytes(genome[int(ts[a]): int(ts[a]) + int(tl[a])]), int(trc[a]),
                         bytes(reads[int(qs[a]): int(qs[a]) + int(ql[a])]), int(begin[a]),
                         _unpack(cg[int(off[a]): int(off[a + 1])]), match, penalty) for a in range(len(ts))]


def _entries(got, a):
    xo, ro = got["xcigar_offset"], got["ref_offset"]
    return _unpack(got["xcigar"][int(xo[a]): int(xo[a + 1])]), bytes(got["ref_bases"][int(ro[a]): int(ro[a + 1])])


def _assert_clipped(got, want, batch, what):
    """got: Verifier.clip's dict; want: restate_clip's dict per alignment.  Every array, every element, and the contract's
    two invariants."""
    from bucket_map_amd import verify
    n = len(want)
    xo, ro = got["xcigar_offset"], got["ref_offset"]
    assert all(len(got[k]) == n for k in ("score", "clip_left", "clip_right", "nm", "pos", "ref_len")) and len(xo) == len(ro) == n + 1
    assert got["score"].dtype == np.int64
    assert xo[0] == 0 and ro[0] == 0 and xo[n] == len(got["xcigar"]) and ro[n] == len(got["ref_bases"]), \
        f"{what}: the totals are not the offsets' ends"
    for a, w in enumerate(want):
        g_xc, g_ref = _entries(got, a)
        g = dict(score=int(got["score"][a]), clip_left=int(got["clip_left"][a]), clip_right=int(got["clip_right"][a]),
                 pos=int(got["pos"][a]), ref_len=int(got["ref_len"][a]), nm=int(got["nm"][a]), xcigar=g_xc, ref_bases=g_ref)
        assert g == {k: w[k] for k in g}, f"{what}: alignment {a} differs from the restatement"
        assert all(p[0] != q[0] for p, q in zip(g_xc, g_xc[1:])), f"{what}: alignment {a} has adjacent entries of one op"
        assert verify.md_string(got["xcigar"][int(xo[a]): int(xo[a + 1])], g_ref) == w["md"], f"{what}: MD of alignment {a}"
        if g_xc:
            assert sum(n_ for op, n_ in g_xc if op in (S, EQ, X, I)) == int(batch[5][a]), f"{what}: alignment {a} loses query bases"
        assert g["pos"] + g["ref_len"] <= int(batch[2][a]), f"{what}: alignment {a} leaves its window"


def _packed(cigars):
    off = np.concatenate([[0], np.cumsum([len(c) for c in cigars])]).astype(np.uint64)
    cg = np.concatenate([pack(c) for c in cigars] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return off, cg


# ------------------------------------------------------------------------------------------------ 1. planted CIGARs

# (op, length) runs in the aligner's frame; every one is planted on both strands, so a border at the first lane of a step on
# one strand is a border at the other end on the other.  Comments give the kept range under match 1 / penalty 2.
PLANTED = [
    [(EQ, 64)],                                               # borders at lane 0 and behind lane 63
    [(X, 1), (EQ, 62), (X, 1)],                               # at lanes 1 and 62
    [(X, 63), (EQ, 1)], [(EQ, 1), (X, 63)],                   # one column, in lane 63 / lane 0
    [(X, 64), (EQ, 64), (X, 64)],                             # borders exactly at the 64-column step boundaries
    [(EQ, 64), (X, 64)], [(X, 64), (EQ, 100)], [(X, 128), (EQ, 64), (X, 10)],
    [(X, 10), (EQ, 100), (X, 10)],                            # one M entry cut by the range on both sides
    [(X, 50), (EQ, 30), (X, 50)],                             # borders inside a run carried across steps
    [(EQ, 60), (X, 3), (EQ, 120), (X, 70), (EQ, 3)],
    [(X, 3), (EQ, 200), (X, 1), (EQ, 200), (X, 3)],
    [(EQ, 64), (X, 3), (EQ, 5), (X, 2)],                      # borders in the last partial step
    [(X, 70), (EQ, 5)], [(X, 130), (EQ, 1)], [(EQ, 129), (X, 2)],
    [(X, 3), (I, 2), (EQ, 30), (D, 3), (X, 2)],               # borders directly beside an I or D entry
    [(EQ, 30), (I, 5)], [(I, 5), (EQ, 30)], [(D, 4), (EQ, 30), (D, 4)], [(I, 2), (D, 2), (EQ, 70), (D, 1), (I, 3)],
    [(EQ, 10), (I, 1), (EQ, 10)], [(EQ, 3), (D, 1), (EQ, 70), (I, 1), (EQ, 3)],    # I and D inside the range
    [(EQ, 40), (I, 5), (EQ, 25)], [(EQ, 40), (D, 5), (X, 1), (EQ, 25)],
    [(EQ, 20), (I, 15), (EQ, 25)],                            # an entry heavier than all before it: the minimum moves behind it
    [(EQ, 20), (D, 15), (EQ, 25)], [(EQ, 70), (D, 40), (EQ, 80), (X, 5)], [(EQ, 70), (I, 35), (EQ, 70)],
    [(EQ, 60), (X, 60), (EQ, 60)],                            # two equal maxima, r = 60 and r = 180: across step boundaries
    [(EQ, 70), (X, 70), (EQ, 70)], [(EQ, 64), (X, 64), (EQ, 64)], [(EQ, 2), (X, 2), (EQ, 2)],
    [(EQ, 64), (X, 32), (EQ, 100)],                           # two equal minima, l = 0 and l = 96
    [(EQ, 2), (X, 1), (EQ, 70)], [(EQ, 66), (X, 33), (EQ, 70)], [(EQ, 128), (X, 64), (EQ, 130)],
    [(EQ, 2), (I, 1), (EQ, 70)], [(EQ, 4), (D, 2), (EQ, 70)],
    [(X, 70)], [(X, 1)], [(I, 5)], [(X, 3), (I, 2), (X, 1)], [(D, 5), (I, 1)], [(D, 130)],     # the empty range
    [(EQ, 1)], [(EQ, 200)],
]


def _planted_batch(genome):
    rng = np.random.default_rng(61)
    b, begins, cigars = _Batch(), [], []

    def plant(spec, rc, **kw):
        bg, cg = _plant(rng, genome, b, spec, rc, **kw)
        begins.append(bg)
        cigars.append(cg)

    def empty(qlen):
        b.add(rng.choice(list(b"ACGT"), qlen).astype(np.uint8), int(rng.integers(0, 100_000)), 40, int(rng.integers(0, 2)))
        begins.append(0)
        cigars.append([])

    for spec in PLANTED:
        for rc in (0, 1):
            plant(spec, rc)
    empty(30)                                                  # an empty CIGAR between two non-empty ones (a rejected alignment)
    for rc in (0, 1):
        plant([(X, 2), (EQ, 90), (X, 2)], rc, begin=0, end_slack=0)
        plant([(EQ, 100), (X, 1)], rc, start=len(genome) - 120, begin=19, end_slack=0)       # the genome's last base
        empty(0)                                               # a zero-length query
    while len(begins) < 220:                                   # random ones on top: short runs, many borders to choose from
        spec, last = [], None
        for _ in range(int(rng.integers(1, 12))):
            op = int(rng.choice([o for o in (EQ, X, I, D) if o != last]))
            spec.append((op, int(rng.integers(1, 90 if op == EQ else 40 if op == X else 6))))
            last = op
        if not any(op != D for op, _ in spec):
            continue
        plant(spec, int(rng.integers(0, 2)))
    off, cg = _packed(cigars)
    return b.args(), begins, off, cg


@pytest.mark.gpu
def test_planted_cigars(genome):
    """About two hundred valid, deliberately non-optimal alignments on both strands under four pairs of scores: every output
    array is the restatement's."""
    from bucket_map_amd import verify
    batch, begins, off, cg = _planted_batch(genome)
    v = _verifier()
    v.load_genome(genome)
    for match, penalty in SCORES:
        want = _expected(genome, batch, begins, off, cg, match, penalty)
        if (match, penalty) == (1, 2):                         # the planted properties are really there
            at = lambda spec, rc: want[2 * PLANTED.index(spec) + rc]
            assert at([(EQ, 60), (X, 60), (EQ, 60)], 0)["xcigar"] == [(EQ, 60), (S, 120)]
            assert at([(EQ, 60), (X, 60), (EQ, 60)], 1)["xcigar"] == [(EQ, 60), (S, 120)]
            assert at([(EQ, 64), (X, 32), (EQ, 100)], 0)["xcigar"] == [(S, 96), (EQ, 100)]
            assert at([(EQ, 64), (X, 32), (EQ, 100)], 1)["xcigar"] == [(EQ, 100), (S, 96)]
            assert at([(EQ, 20), (I, 15), (EQ, 25)], 0)["xcigar"] == [(S, 35), (EQ, 25)]
            assert at([(X, 10), (EQ, 100), (X, 10)], 1)["xcigar"] == [(S, 10), (EQ, 100), (S, 10)]
            assert at([(X, 70)], 0)["xcigar"] == [(S, 70)] and at([(D, 130)], 0)["xcigar"] == []
            assert at([(D, 4), (EQ, 30), (D, 4)], 0)["clip_left"] == 0 and at([(D, 4), (EQ, 30), (D, 4)], 0)["pos"] >= 4
        got = v.clip(*batch, begins, off, cg, match=match, penalty=penalty)
        st = v.clip_stats()
        assert st["columns"] == int((cg >> 4).sum()) and st["ms_kernels"] > 0
        _assert_clipped(got, want, batch, f"planted, scores {match}/{penalty}")
    # the defaults are 1 / 2, and the call takes offsets that do not start at 0, as a share of a larger batch has them
    want = _expected(genome, batch, begins, off, cg, 1, 2)
    part = slice(60, 160)
    share = tuple(x[part] for x in batch)[1:]
    got = v.clip(batch[0], *share, begins[part], off[60:161], cg)
    v.close()
    _assert_clipped(got, want[part], (batch[0], *share), "a share of the batch")
    assert verify.xcigar_string(got["xcigar"][: int(got["xcigar_offset"][1])]) == "".join(f"{n}{'MIDNSHP=X'[op]}" for op, n in want[60]["xcigar"])


@pytest.mark.gpu
def test_one_long_entry(genome):
    """A single M entry of 70 000 columns on either strand (more than 65 536: the column index leaves 16 bits, a thousand
    steps carry the minimum and the best) with a planted bad tail of two mismatches in three columns."""
    rng = np.random.default_rng(62)
    b, begins, cigars = _Batch(), [], []
    for rc in (0, 1):
        spec = [(EQ, 30_000), (X, 1), (EQ, 34_989)] + [(X, 2), (EQ, 1)] * 1670
        bg, cg = _plant(rng, genome, b, spec, rc, exact=True)
        assert cg == [(M, 70_000)]
        begins.append(bg)
        cigars.append(cg)
    batch = b.args()
    off, cg = _packed(cigars)
    want = _expected(genome, batch, begins, off, cg, 1, 2)
    assert want[0]["xcigar"] == [(EQ, 30_000), (X, 1), (EQ, 34_989), (S, 5010)] and want[0]["score"] == 64_987
    assert want[1]["xcigar"] == [(S, 5010), (EQ, 34_989), (X, 1), (EQ, 30_000)]
    v = _verifier()
    v.load_genome(genome)
    got = v.clip(*batch, begins, off, cg)
    v.close()
    _assert_clipped(got, want, batch, "one long entry")


@pytest.mark.gpu
def test_prefix_sums_beyond_32_bits():
    """One alignment of 2 200 000 columns at match 1024: the prefix sums pass 2^31 (and 2^32 x 1/2), the score does too.
    300 leading and 500 trailing mismatches are clipped, a thousand scattered ones stay."""
    rng = np.random.default_rng(63)
    n = 2_200_000
    g = rng.choice(list(b"ACGT"), n + 64).astype(np.uint8)
    src = g[7: 7 + n]
    fwd = src.copy()                                           # the read along the forward strand
    other = np.frombuffer(b"CGTA", np.uint8)                   # a letter of another rank
    bad = np.concatenate([np.arange(300), np.arange(n - 500, n), rng.choice(np.arange(400, n - 600), 1000, replace=False)])
    fwd[bad] = other[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), src[bad])]
    b = _Batch()
    b.add(_revcomp(fwd), 0, n + 64, 1)
    batch = b.args()
    begins, (off, cg) = [n + 64 - 7 - n], _packed([[(M, n)]])
    want = _expected(g, batch, begins, off, cg, 1024, 1)
    assert want[0]["score"] == (n - 800 - 1000) * 1024 - 1000 > 2 ** 31 and want[0]["clip_left"] == 300 and want[0]["clip_right"] == 500
    assert want[0]["pos"] == 307 and want[0]["nm"] == 1000
    v = _verifier()
    v.load_genome(g)
    got = v.clip(*batch, begins, off, cg, match=1024, penalty=1)
    v.close()
    _assert_clipped(got, want, batch, "2.2 M columns")


# ------------------------------------------------------------------------------------------------ 2. after the aligner

TAIL = 40


def _tailed(rng, genome, count):
    """300-base reads with 2 % edits; every third carries TAIL random bases behind its 3' end (an adapter).  The window
    leaves room for the tail on the side where it lies along the forward strand.  Returns the batch, and per read whether it
    is tailed and where its genome bases begin in the window."""
    b, tailed, true_pos = _Batch(), [], []
    for k in range(count):
        rc, t = int(rng.integers(0, 2)), k % 3 == 0
        start = int(rng.integers(0, len(genome) - 400))
        lead = 1 + (TAIL if t and rc else 0)
        src = genome[start + lead: start + lead + 300]
        q = _mutate(rng, _revcomp(src) if rc else src, 0.01, 0.005, 0.005)
        if t:
            q = np.concatenate([q, rng.choice(list(b"ACGT"), TAIL).astype(np.uint8)])
        b.add(q, start, 307 + (TAIL if t else 0), rc)
        tailed.append(t)
        true_pos.append(lead)
    return b.args(), np.array(tailed), np.array(true_pos)


@pytest.mark.gpu
def test_after_the_aligner(plain_genome):
    """2 001 simulated 300-base reads through align, then clip with the default scores: the restatement's arrays; the tailed
    reads lose about TAIL bases at the tailed end and begin where their genome bases begin.

    The slack around TAIL.  The clip is shorter than TAIL by k when the first k columns of the tail keep a positive score:
    more than two = columns in three, where a random base matches with probability 1/4 (somewhat more after the aligner chose
    the tail's gaps); k = 1 alone happens to a quarter of the reads.  It is longer by k when the read's last k genome columns
    score at most 0, which takes an edit among the last two or three (2 % edits per base).  Both tails fall off geometrically:
    at least 90 % of the tailed reads are asked to be within 5 of TAIL, and every one within 20 (fourteen = columns in twenty
    random ones: below 1e-5 a read).  POS inherits the same slack on the reverse strand, where the tail lies on the left."""
    rng = np.random.default_rng(64)
    batch, tailed, true_pos = _tailed(rng, plain_genome, 2001)
    v = _verifier()
    v.load_genome(plain_genome)
    score, begin, off, cg = v.align(*batch)
    got = v.clip(*batch, begin, off, cg)
    v.close()
    _assert_clipped(got, _expected(plain_genome, batch, begin, off, cg, 1, 2), batch, "after align")
    rc = batch[3].astype(bool)
    at_tail = np.where(rc, got["clip_left"], got["clip_right"]).astype(np.int64)
    elsewhere = np.where(rc, got["clip_right"], got["clip_left"]).astype(np.int64)
    off_by = np.abs(at_tail[tailed] - TAIL)
    assert tailed.sum() == 667 and off_by.max() <= 20 and (off_by <= 5).mean() >= 0.9, np.bincount(off_by)
    assert (at_tail[~tailed] <= 20).all() and (at_tail[~tailed] == 0).mean() >= 0.9 and (elsewhere == 0).mean() >= 0.9
    pos_off = np.abs(got["pos"].astype(np.int64) - true_pos)
    assert pos_off.max() <= 20 and (pos_off[tailed] <= 5).mean() >= 0.9 and (pos_off[~tailed] == 0).mean() >= 0.9
    assert (got["score"] > 200).all()


@pytest.mark.gpu
def test_after_align_long(plain_genome):
    """One 70 000-base read with substitutions and a tail of 500 random bases through align_long, on the reverse strand."""
    rng = np.random.default_rng(65)
    b = _Batch()
    src = plain_genome[1600: 71_600]
    q = np.concatenate([_mutate(rng, _revcomp(src), 0.02, 0, 0), rng.choice(list(b"ACGT"), 500).astype(np.uint8)])
    b.add(q, 1000, 70_620, 1)
    batch = b.args()
    v = _verifier()
    v.load_genome(plain_genome)
    score, begin, off, cg = v.align_long(*batch)
    got = v.clip(*batch, begin, off, cg)
    v.close()
    _assert_clipped(got, _expected(plain_genome, batch, begin, off, cg, 1, 2), batch, "after align_long")
    assert abs(int(got["clip_left"][0]) - 500) <= 20 and abs(int(got["pos"][0]) - 600) <= 20 and int(got["clip_right"][0]) <= 20
    assert int(got["score"][0]) > 60_000


@pytest.mark.gpu
def test_after_align_bounded(plain_genome):
    """Half the alignments at unrelated places under a bound of 10 %: the rejected come back with zeros and no entries."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(66)
    b = _Batch()
    _simulated(rng, plain_genome, b, 600, 300, 307, (0.02, 0.01, 0.01))
    batch = list(b.args())
    batch[1] = np.where(np.arange(600) % 2 == 1, (batch[1] + 150_000) % 390_000, batch[1]).astype(np.uint64)
    v = _verifier()
    v.load_genome(plain_genome)
    score, begin, off, cg = v.align_bounded(*batch, np.full(600, 30, np.uint32))
    rejected = score == verify.REJECTED
    assert 250 < rejected.sum() < 350
    got = v.clip(*batch, begin, off, cg)
    v.close()
    _assert_clipped(got, _expected(plain_genome, batch, begin, off, cg, 1, 2), batch, "after align_bounded")
    for k in ("score", "clip_left", "clip_right", "nm", "pos", "ref_len"):
        assert not got[k][rejected].any(), k
    assert (np.diff(got["xcigar_offset"].astype(np.int64))[rejected] == 0).all()
    assert (np.diff(got["ref_offset"].astype(np.int64))[rejected] == 0).all()
    assert (got["score"][~rejected] > 200).all()


@pytest.mark.gpu
def test_the_truncated_window(plain_genome):
    """The query is 300 genome bases, its text window only the 200 of them at one end -- what a read that overhangs a
    bucket's border gets.  align has to insert the other 100; clip reports them as S.  The window's last base (as the
    aligner sees it) is made a letter the overhang does not hold, so that no chance match lets the aligner split the run."""
    rng = np.random.default_rng(67)
    g = plain_genome.copy()
    g[5200: 5300] = rng.choice(list(b"ACG"), 100)             # forward: window g[5000, 5200), the overhang behind it
    g[5199] = ord("T")
    g[9000: 9100] = rng.choice(list(b"ACG"), 100)             # reverse: window g[9100, 9300), the overhang before it
    g[9100] = ord("T")
    b = _Batch()
    b.add(g[5000: 5300], 5000, 200, 0)
    b.add(_revcomp(g[9000: 9300]), 9100, 200, 1)
    batch = b.args()
    v = _verifier()
    v.load_genome(g)
    score, begin, off, cg = v.align(*batch)
    assert score.tolist() == [-100, -100] and _unpack(cg) == [(M, 200), (I, 100)] * 2 and begin.tolist() == [0, 0]
    got = v.clip(*batch, begin, off, cg)
    v.close()
    _assert_clipped(got, _expected(g, batch, begin, off, cg, 1, 2), batch, "the truncated window")
    assert _entries(got, 0)[0] == [(EQ, 200), (S, 100)] and _entries(got, 1)[0] == [(S, 100), (EQ, 200)]
    assert got["pos"].tolist() == [0, 0] and got["nm"].tolist() == [0, 0] and got["score"].tolist() == [200, 200]


# ------------------------------------------------------------------------------------------------ 3. relation to bmv_annotate

@pytest.mark.gpu
def test_relation_to_annotate(plain_genome):
    """match 1024 / penalty 1 on reads with fewer than 1024 edits: no stretch of edits outweighs one match, so the kept part
    is annotate's output with only the leading and trailing non-= columns removed."""
    rng = np.random.default_rng(68)
    b = _Batch()
    _simulated(rng, plain_genome, b, 500, 300, 307, (0.04, 0.02, 0.02))
    batch = b.args()
    v = _verifier()
    v.load_genome(plain_genome)
    score, begin, off, cg = v.align(*batch)
    nm, pos, ref_len, xo, xc, ro, rb = v.annotate(*batch, begin, off, cg)
    got = v.clip(*batch, begin, off, cg, match=1024, penalty=1)
    v.close()
    assert nm.max() < 1024
    trimmed = 0
    for a in range(500):
        ent = _unpack(xc[int(xo[a]): int(xo[a + 1])])
        ref = bytes(rb[int(ro[a]): int(ro[a + 1])])
        head = next(k for k, e in enumerate(ent) if e[0] == EQ)
        tail = len(ent) - next(k for k, e in enumerate(reversed(ent)) if e[0] == EQ)
        cut_q = lambda es: sum(n for op, n in es if op != D)
        cut_t = lambda es: sum(n for op, n in es if op != I)
        cut_r = lambda es: sum(n for op, n in es if op in (X, D))
        left, right = cut_q(ent[:head]), cut_q(ent[tail:])
        want = ([(S, left)] if left else []) + ent[head:tail] + ([(S, right)] if right else [])
        g_xc, g_ref = _entries(got, a)
        assert g_xc == want and g_ref == ref[cut_r(ent[:head]): len(ref) - cut_r(ent[tail:])], a
        assert int(got["pos"][a]) == int(pos[a]) + cut_t(ent[:head]) and int(got["ref_len"][a]) == cut_t(ent[head:tail])
        assert int(got["nm"][a]) == int(nm[a]) - sum(n for _, n in ent[:head] + ent[tail:])
        assert int(got["score"][a]) == 1024 * sum(n for op, n in ent if op == EQ) - int(got["nm"][a])
        trimmed += head > 0 or tail < len(ent)
    assert trimmed > 20, "no alignment began or ended on an edit: the comparison shows little"


# ------------------------------------------------------------------------------------------------ 4. refusals

@pytest.mark.gpu
def test_refusals_leave_the_context_usable(plain_genome):
    from bucket_map_amd import verify
    rng = np.random.default_rng(69)
    b = _Batch()
    _simulated(rng, plain_genome, b, 50, 300, 307, (0.02, 0.01, 0.01))
    batch = b.args()
    with pytest.raises(verify.BmvError) as e:
        verify.Verifier().clip(*batch, np.zeros(50, np.uint32), np.zeros(51, np.uint64), np.zeros(0, np.uint32))
    assert e.value.code == 3                                     # BMV_ERR_STATE: no genome yet
    v = _verifier()
    v.load_genome(plain_genome)
    results = v.align(*batch)
    score, begin, off, cg = results
    annotations = v.annotate(*batch, begin, off, cg)
    a_stats, stats = v.annotate_stats(), v.stats()
    want = _expected(plain_genome, batch, begin, off, cg, 1, 2)
    _assert_clipped(v.clip(*batch, begin, off, cg), want, batch, "before the refusals")
    one = tuple(x[7:8] for x in batch[1:])                       # alignment 7 alone, as alignment 2 of three
    three = (batch[0], *(np.concatenate([x[:2], y]) for x, y in zip(batch[1:], one)))
    head = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in (0, 1)]
    bad_cigars = {
        "consumes query_len - 1": [(M, 299)],
        "runs past the window": [(M, 300), (D, 8)],
        "a zero-length entry": [(M, 150), (I, 0), (M, 150)],
        "adjacent equal ops": [(M, 150), (M, 150)],
        "an op code of 4": [(M, 150), (S, 2), (M, 150)],
    }
    for what, bad in bad_cigars.items():
        cigs = head + [bad]
        o, c = _packed(cigs)
        with pytest.raises(verify.BmvError) as e:
            v.clip(*three, np.array([begin[0], begin[1], 0], np.uint32), o, c)
        assert e.value.code == 1 and "alignment 2" in str(e.value), (what, str(e.value))
    for match, penalty in ((0, 1), (1, 0), (1025, 1), (1, 1025)):
        with pytest.raises(verify.BmvError) as e:
            v.clip(*batch, begin, off, cg, match=match, penalty=penalty)
        assert e.value.code == 1 and "1..1024" in str(e.value), str(e.value)
    _assert_clipped(v.clip(*batch, begin, off, cg), want, batch, "after the refusals")
    # neither the clips nor the refusals touched what the other calls return
    L = verify.lib()
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    s2, b2, o2, c2 = np.zeros(50, np.int32), np.zeros(50, np.uint32), np.zeros(51, np.uint64), np.zeros(len(cg), np.uint32)
    assert L.bmv_results(v._h, p(s2, C.c_int32), p(b2, C.c_uint32), p(o2, C.c_uint64), p(c2, C.c_uint32)) == 0
    assert all(np.array_equal(x, y) for x, y in zip((s2, b2, o2, c2), results)), "clip changed bmv_results"
    again = [np.zeros_like(x) for x in annotations]
    assert L.bmv_annotations(v._h, p(again[0], C.c_uint32), p(again[1], C.c_uint32), p(again[2], C.c_uint32), p(again[3], C.c_uint64),
                             p(again[4], C.c_uint32), p(again[5], C.c_uint64), p(again[6], C.c_uint8)) == 0
    assert all(np.array_equal(x, y) for x, y in zip(again, annotations)), "clip changed bmv_annotations"
    assert v.annotate_stats() == a_stats and v.stats() == stats and v.bounded_stats()["n_rejected"] == 0
    got = v.clip(np.zeros(0, np.uint8), [], [], [], [], [], [], [0], [])                                   # n == 0 is fine
    assert got["xcigar_offset"].tolist() == [0] and len(got["score"]) == 0
    v.close()


# ------------------------------------------------------------------------------------------------ 5. the tool

ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAG"                        # 30 bases, the start of a common sequencing adapter


def _clip_record(f, match, penalty):
    """What --clip makes of one --annotate record: (POS, CIGAR, NM, MD, AS), or None when nothing is kept."""
    ops = [(int(n), "MIDNSHP=X".index(op)) for n, op in re.findall(r"(\d+)([=XID])", f[5])]
    cols = [op for n, op in ops for _ in range(n)]
    score, l, r = range_scan([match if op == EQ else -penalty for op in cols])
    if l == r:
        return None
    before, kept, after = cols[:l], cols[l:r], cols[r:]
    left, right = sum(1 for op in before if op != D), sum(1 for op in after if op != D)
    runs = []
    for op in kept:
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    cigar = (f"{left}S" if left else "") + "".join(f"{n}{'MIDNSHP=X'[op]}" for op, n in runs) + (f"{right}S" if right else "")
    # MD of the kept part: the whole record's MD items, an item per X or D column or = run, cut the same way
    tags = dict(t.split(":", 2)[::2] for t in f[11:])
    ref = re.sub(r"[\d^]", "", tags["MD"])                       # the reference letters under X and D, in order
    at = sum(1 for op in before if op in (X, D))
    md, run = "", 0
    for op, n in runs:
        if op == EQ:
            run += n
        elif op == X:
            for k in range(n):
                md += f"{run}{ref[at + k]}"
                run = 0
            at += n
        elif op == D:
            md += f"{run}^{ref[at: at + n]}"
            run = 0
            at += n
    return (int(f[3]) + sum(1 for op in before if op != I), cigar, sum(1 for op in kept if op != EQ), md + str(run), score)


@pytest.mark.gpu
def test_bucketmap_align_with_clip(tmp_path):
    """3 000 reads of 120 bases, every third with 30 adapter bases behind it: --annotate (whose records are the parent's,
    byte for byte, and true against the FASTA) and --clip, whose records are the --annotate records cut by the restatement's
    range finder; two contexts write the same bytes; other scores through --clip-scores."""
    from bucket_map_amd import host
    g = host.Genome.synth(43, [700_000, 250_000])
    g.write_fasta(str(tmp_path / "g.fa"))
    host.Reads(g, 8192, 150, 120, 3000, sub=0.02, ins=0.004, dele=0.004, seed=11).write_fastq(str(tmp_path / "plain"))
    lines = open(tmp_path / "plain.fastq").read().split("\n")
    for k in range(0, len(lines) - 3, 12):                       # every third record
        lines[k + 1] += ADAPTER
        lines[k + 3] += lines[k + 3][:30]
    open(tmp_path / "r.fastq", "w").write("\n".join(lines))
    common = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "8192", "-r", "150", "-f", "1", "-u", "0", "-q", "r.fastq"]
    err_ann = _tool([*common, "-o", "ann.sam", "--annotate"], tmp_path)
    err = _tool([*common, "-o", "clip.sam", "--clip"], tmp_path)
    assert "GPU alignment clipping" in err and "GPU alignment clipping" not in err_ann and "GPU alignment annotation" not in err
    _tool([*common, "-o", "clip2.sam", "--clip", "--gpus", "0,0"], tmp_path)
    _tool([*common, "-o", "clip3.sam", "--clip-scores", "1,2", "--annotate"], tmp_path)
    _tool([*common, "-o", "clip4.sam", "--clip-scores=2,3"], tmp_path)
    assert (tmp_path / "clip2.sam").read_bytes() == (tmp_path / "clip.sam").read_bytes()
    assert (tmp_path / "clip3.sam").read_bytes() == (tmp_path / "clip.sam").read_bytes()
    # without --clip: the parent's --annotate output on these inputs (tests/golden/clip_tool_annotate.sha256 was taken from the
    # parent's build), and true against the FASTA by the parent's own check
    ref, reads = _fasta(tmp_path / "g.fa"), _fastq(tmp_path / "r.fastq")
    ann = _records(tmp_path / "ann.sam")
    _check_annotated(ann, ref, reads)
    golden = open(os.path.join(ROOT, "tests", "golden", "clip_tool_annotate.sha256")).read().split()[0]
    assert hashlib.sha256((tmp_path / "ann.sam").read_bytes()).hexdigest() == golden, "--annotate no longer writes the parent's bytes"
    head = lambda p: [l for l in open(tmp_path / p).read().split("\n") if l.startswith("@")]
    assert head("ann.sam") == head("clip.sam")
    fold_len = lambda name: len(reads[name][0])
    for path, (match, penalty) in (("clip.sam", (1, 2)), ("clip4.sam", (2, 3))):
        clip = _records(tmp_path / path)
        want = [(f, _clip_record(f, match, penalty)) for f in ann]
        want = [(f, w) for f, w in want if w is not None]
        assert len(clip) == len(want) > 1000 and all(len(f) == 14 for f in clip)
        n_s = n16_s = 0
        for c, (f, (pos, cigar, nm, md, score)) in zip(clip, want):
            assert c[:3] == f[:3] and c[4] == f[4] and c[6:11] == f[6:11], (c[0], "QNAME, FLAG, RNAME, MAPQ, SEQ or QUAL changed")
            assert (int(c[3]), c[5], c[11], c[12], c[13]) == (pos, cigar, f"NM:i:{nm}", f"MD:Z:{md}", f"AS:i:{score}"), (c[0], f[5])
            parts = [(int(n), op) for n, op in re.findall(r"(\d+)([=XIDS])", c[5])]
            assert sum(n for n, op in parts if op in "S=XI") == len(c[9]) == fold_len(c[0]), c[0]
            assert all(op != "S" for _, op in parts[1:-1]) and parts[0][1] in "S=" and parts[-1][1] in "S="
            n_s += "S" in c[5]
            n16_s += "S" in c[5] and c[1] == "16"
        # about a third of the reads carry an adapter, on either strand
        assert n_s > len(clip) // 5 and n16_s > len(clip) // 20, (n_s, n16_s, len(clip))
