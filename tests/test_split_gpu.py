"""Split alignments on the GPU (bmv_split, bmv_split_pick, include/bmv.h): the range pass on planted CIGARs at the shapes
where a wave-wide search that carries cursors can go wrong, the pick alone at every lane-chunk border, the whole call on
planted chimeric reads behind the aligner, what the call leaves alone, its refusals, and `bucketmap_align --split`.

Expected values come from verify.clip_range and verify.select_segments, the plain-Python restatements tests/test_split.py
holds against brute force, and from Verifier.clip on the same inputs."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from test_annotate import D, EQ, I, M, X
from test_annotate_gpu import _Batch, _mutate, _plant, _revcomp, _unpack, _verifier, genome, plain_genome  # noqa: F401  (fixtures)
from test_clip_gpu import PLANTED, SCORES, _packed

from bucket_map_amd import verify

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NONE, BEYOND = verify.SPLIT_NONE, verify.BEYOND
PER_ALIGNMENT = ("score", "q_lo", "q_hi", "g_lo", "g_hi")


def _ranges(genome, batch, begin, off, cg, match, penalty):
    """verify.clip_range per alignment, as the five arrays bmv_segments returns."""
    reads, ts, tl, trc, qs, ql = batch
    out = {k: [] for k in PER_ALIGNMENT}
    for a in range(len(ts)):
        r = verify.clip_range(genome[int(ts[a]): int(ts[a]) + int(tl[a])], reads[int(qs[a]): int(qs[a]) + int(ql[a])], int(trc[a]),
                              int(begin[a]), cg[int(off[a]): int(off[a + 1])], match, penalty)
        out["score"].append(r["score"]); out["q_lo"].append(r["q_lo"]); out["q_hi"].append(r["q_hi"])
        out["g_lo"].append(int(ts[a]) + r["g_off_lo"]); out["g_hi"].append(int(ts[a]) + r["g_off_hi"])
    return out


def _assert_split(got, want, groups, min_score, permille, max_segments, what, contig=None, clipped=None, batch=None):
    """got: Verifier.split's dict; want: _ranges' lists.  Every per-alignment array, then the pick over them; clipped:
    Verifier.clip's dict for the same inputs, whose score, clips, pos and ref_len give the same five arrays."""
    for k in PER_ALIGNMENT:
        assert got[k].tolist() == want[k], f"{what}: {k} differs from clip_range at {np.nonzero(got[k] != np.array(want[k]))[0][:5]}"
    assert got["score"].dtype == np.int64 and got["g_lo"].dtype == np.int64 and got["q_lo"].dtype == np.uint32
    if clipped is not None:
        ts, trc, ql = batch[1].astype(np.int64), batch[3].astype(bool), batch[5].astype(np.int64)
        cl, cr = clipped["clip_left"].astype(np.int64), clipped["clip_right"].astype(np.int64)
        assert np.array_equal(got["score"], clipped["score"]), f"{what}: the score is not bmv_clip's"
        assert np.array_equal(got["q_lo"], np.where(trc, cr, cl)) and np.array_equal(got["q_hi"], ql - np.where(trc, cl, cr)), what
        assert np.array_equal(got["g_lo"], ts + clipped["pos"]) and np.array_equal(got["g_hi"], ts + clipped["pos"] + clipped["ref_len"]), what
    pick = verify.select_segments(want["score"], want["q_lo"], want["q_hi"], want["g_lo"], want["g_hi"], batch[3] if batch else got["rc"],
                                  groups, min_score, permille, max_segments, contig)
    for k in ("n_seg", "seg", "s2"):
        assert np.array_equal(got[k], pick[k]), f"{what}: {k} differs from select_segments in groups {np.nonzero((got[k] != pick[k]).reshape(len(groups) - 1, -1).any(1))[0][:5]}"
    return pick


# ------------------------------------------------------------------------------------------------ 1. the range pass

# beyond test_clip_gpu's PLANTED (borders at lanes 0, 1, 62, 63, at the step boundaries, in carried steps, beside I and D,
# equal maxima and minima): borders at columns 63, 64, 65 and 128 of ONE M entry, from either side, and the minimum and the
# best in one step or steps apart
MORE = [[(X, k), (EQ, 200 - k)] for k in (63, 64, 65, 128)] + [[(EQ, k), (X, 200 - k)] for k in (63, 64, 65, 128)] + [
    [(EQ, 5), (X, 58), (EQ, 1), (X, 1), (EQ, 70)],            # the minimum at column 63 / 65 of the entry, the best steps later
    [(EQ, 5), (X, 59), (EQ, 70)], [(EQ, 5), (X, 60), (EQ, 70)], [(EQ, 5), (X, 123), (EQ, 70)],
    [(X, 10), (EQ, 20), (X, 3), (EQ, 20), (X, 11)],           # the minimum and the best in the same step
    [(EQ, 2), (X, 5), (EQ, 3), (X, 9), (EQ, 4), (X, 20), (EQ, 19)],
    [(X, 64), (EQ, 1), (X, 63), (EQ, 2), (X, 62)],            # one and two columns, right behind a step boundary
    [(EQ, 30), (X, 40), (I, 3), (EQ, 31)], [(EQ, 31), (D, 3), (X, 40), (EQ, 30)],      # the minimum behind an I / in front of a D
    [(I, 7), (EQ, 64), (I, 7)], [(D, 7), (EQ, 65), (D, 7)], [(X, 2), (D, 70), (EQ, 63), (I, 70), (X, 2)],
    [(EQ, 50), (X, 25), (EQ, 50), (X, 25), (EQ, 50)],         # three equal maxima end at r = 50, the whole range ties too
    [(EQ, 63), (X, 63), (EQ, 63), (X, 63), (EQ, 63)], [(EQ, 64), (X, 32), (EQ, 64), (X, 32), (EQ, 64)],
]


def _range_batch(genome, seed=71):
    rng = np.random.default_rng(seed)
    b, begins, cigars = _Batch(), [], []

    def plant(spec, rc, **kw):
        bg, cg = _plant(rng, genome, b, spec, rc, **kw)
        begins.append(bg)
        cigars.append(cg)

    for spec in PLANTED + MORE:
        for rc in (0, 1):
            plant(spec, rc)
    b.add(rng.choice(list(b"ACGT"), 30).astype(np.uint8), 1234, 40, 1)          # an empty CIGAR, a zero-length query
    begins.append(0); cigars.append([])
    b.add(np.zeros(0, np.uint8), 99, 40, 0)
    begins.append(0); cigars.append([])
    plant([(EQ, 100), (X, 1)], 0, start=len(genome) - 120, begin=19, end_slack=0)            # the genome's last base
    while len(begins) < 300:                                   # random ones on top: short runs, many borders to choose from
        spec, last = [], None
        for _ in range(int(rng.integers(1, 12))):
            op = int(rng.choice([o for o in (EQ, X, I, D) if o != last]))
            spec.append((op, int(rng.integers(1, 90 if op == EQ else 40 if op == X else 6))))
            last = op
        if any(op != D for op, _ in spec):
            plant(spec, int(rng.integers(0, 2)))
    off, cg = _packed(cigars)
    return b.args(), np.array(begins, np.uint32), off, cg


@pytest.mark.gpu
def test_range_pass_on_planted_cigars(genome):
    """300 planted alignments on both strands, odd letters included, under four pairs of scores: the five per-alignment arrays
    are clip_range's and Verifier.clip's, and the pick over groups of 0 .. 7 of them is select_segments'."""
    batch, begins, off, cg = _range_batch(genome)
    n = len(begins)
    rng = np.random.default_rng(72)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(0, 8)), n - sum(sizes)))
    groups = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    v = _verifier()
    v.load_genome(genome)
    for match, penalty in SCORES:
        want = _ranges(genome, batch, begins, off, cg, match, penalty)
        if (match, penalty) == (1, 2):                         # the planted properties are really there
            at = lambda spec, rc: 2 * (PLANTED + MORE).index(spec) + rc
            a = at([(X, 64), (EQ, 136)], 0)
            assert (want["q_lo"][a], want["q_hi"][a], want["score"][a]) == (64, 200, 136)
            a = at([(X, 65), (EQ, 135)], 1)                    # read orientation, whatever the strand
            assert (want["q_lo"][a], want["q_hi"][a], want["g_hi"][a] - want["g_lo"][a]) == (65, 200, 135)
            a = at([(EQ, 50), (X, 25), (EQ, 50), (X, 25), (EQ, 50)], 0)
            assert (want["q_lo"][a], want["q_hi"][a], want["score"][a]) == (0, 50, 50)
            a = at([(X, 2), (D, 70), (EQ, 63), (I, 70), (X, 2)], 0)
            assert (want["q_lo"][a], want["q_hi"][a], want["g_hi"][a] - want["g_lo"][a]) == (2, 65, 63)
        clipped = v.clip(*batch, begins, off, cg, match=match, penalty=penalty)
        got = v.split(*batch, begins, off, cg, groups, match=match, penalty=penalty, min_score=3 * match, max_overlap_permille=300, max_segments=3)
        st = v.split_stats()
        assert st["columns"] == int((cg >> 4).sum()) and st["ms_range"] > 0 and st["ms_pick"] > 0
        pick = _assert_split(got, want, groups, 3 * match, 300, 3, f"planted, scores {match}/{penalty}", clipped=clipped, batch=batch)
        assert st["n_segments"] == int(pick["n_seg"].sum()) > 60
    # offsets that do not start at 0, as a share of a larger batch has them
    want = _ranges(genome, batch, begins, off, cg, 1, 2)
    part = slice(60, 160)
    share = tuple(x[part] for x in batch)[1:]
    got = v.split(batch[0], *share, begins[part], off[60:161], cg, [0, 40, 40, 100], min_score=1, max_segments=16)
    v.close()
    _assert_split(got, {k: x[part] for k, x in want.items()}, [0, 40, 40, 100], 1, 500, 16, "a share of the batch", batch=(batch[0], *share))


@pytest.mark.gpu
def test_range_pass_on_one_long_entry(genome):
    """A single M entry of 70 000 columns on either strand: a thousand steps carry the minimum's and the best's cursors."""
    rng = np.random.default_rng(73)
    b, begins, cigars = _Batch(), [], []
    for rc in (0, 1):
        spec = [(X, 2), (EQ, 1)] * 700 + [(EQ, 30_000), (X, 1), (EQ, 32_889)] + [(X, 2), (EQ, 1)] * 1670
        bg, cg = _plant(rng, genome, b, spec, rc, exact=True)
        assert cg == [(M, 70_000)]
        begins.append(bg); cigars.append(cg)
    batch = b.args()
    off, cg = _packed(cigars)
    want = _ranges(genome, batch, begins, off, cg, 1, 2)
    # (the = that ends the leading pattern belongs to the range: 62 891 columns, two of them X)
    assert want["score"] == [62_888, 62_888] and (want["q_lo"][0], want["q_hi"][0]) == (2099, 64_990) == (want["q_lo"][1], want["q_hi"][1])
    v = _verifier()
    v.load_genome(genome)
    got = v.split(*batch, begins, off, cg, [0, 2])
    clipped = v.clip(*batch, begins, off, cg)
    v.close()
    _assert_split(got, want, [0, 2], 40, 500, 8, "one long entry", clipped=clipped, batch=batch)
    assert got["n_seg"].tolist() == [1] and got["seg"][0, 0] == 0      # the second is a conflict: it claims the same bases


# ------------------------------------------------------------------------------------------------ 2. the pick alone

def _check_pick(v, f, groups, min_score, permille, max_segments, what, contig=None):
    got = v.split_pick(f["score"], f["q_lo"], f["q_hi"], f["g_lo"], f["g_hi"], f["rc"], groups, min_score, permille, max_segments, contig)
    for k in PER_ALIGNMENT:
        assert got[k].tolist() == list(f[k]), f"{what}: bmv_segments does not return {k} as given"
    want = verify.select_segments(f["score"], f["q_lo"], f["q_hi"], f["g_lo"], f["g_hi"], f["rc"], groups, min_score, permille, max_segments, contig)
    for k in ("n_seg", "seg", "s2"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs in groups {np.nonzero((got[k] != want[k]).reshape(len(groups) - 1, -1).any(1))[0][:5]}"
    assert got["seg"].shape == (len(groups) - 1, max_segments)
    return want


def _fields(cands):
    cols = list(zip(*cands)) if cands else [[]] * 7
    return dict(zip(("score", "q_lo", "q_hi", "g_lo", "g_hi", "rc", "contig"), (list(c) for c in cols)))


def _border_groups():
    """Groups of 0, 1, 2, 63, 64, 65 and 130 candidates.  The read has a part per candidate of its group's first hundred, all
    of a low eligible score; three candidates are planted over them: the winner (the top score), one that conflicts with
    it (the second score, the same part of the read elsewhere in the genome) and one that does not (the third) -- each at
    every lane-chunk border of the group in turn."""
    cands, groups = [], [0]
    for size in (0, 1, 2, 63, 64, 65, 130):
        borders = sorted({p for p in (0, 1, 62, 63, 64, 65, 127, 128, 129, size - 1) if 0 <= p < size})
        for w in borders or [None]:
            for c in borders or [None]:
                if size > 1 and c == w:
                    continue
                group = [(50 + k % 7, 10 * k, 10 * k + 10, 100_000 + 1000 * k, 100_000 + 1000 * k + 10, k % 2, 0) for k in range(size)]
                if w is not None:
                    group[w] = (10 ** 13 if w % 2 else 900, 0, 400, 5_000_000, 5_000_400, 0, 0)
                if size > 1:
                    group[c] = (800, 100, 500, 7_000_000, 7_000_400, 1, 0)
                    third = next(p for p in reversed(range(size)) if p not in (w, c)) if size > 2 else None
                    if third is not None:
                        group[third] = (700, 1400, 1900, 9_000_000, 9_000_500, 0, 0)
                cands += group
                groups.append(len(cands))
    return _fields(cands), groups


@pytest.mark.gpu
def test_pick_alone_at_the_lane_chunk_borders():
    f, groups = _border_groups()
    assert len(groups) > 100
    v = _verifier()
    for ms in (1, 2, 16):
        want = _check_pick(v, f, groups, 40, 500, ms, f"borders, max_segments {ms}")
        assert want["n_seg"].max() == ms
        st = v.split_stats()
        assert st["ms_range"] == 0 and st["ms_pick"] > 0 and st["columns"] == 0 and st["n_segments"] == int(want["n_seg"].sum())
    # the groups of 130 under a rule that lets every part in: 16 rounds over three chunks, and s2 of the winner is the one that
    # conflicts with it
    want = _check_pick(v, f, groups, 40, 0, 16, "borders, 0 permille")
    big = np.nonzero(np.diff(groups) == 130)[0]
    assert (want["n_seg"][big] == 16).all() and (want["s2"][big, 0] == 800).all()
    v.close()


@pytest.mark.gpu
def test_pick_alone_threshold_cases():
    """The cases of tests/test_split.py that sit on a threshold, a group each, in one call per parameter set."""
    seg = (90, 0, 100, 0, 100, 0, 0)
    cases = [
        [(90, 0, 200, 0, 200, 0, 0), (80, 150, 250, 5000, 5100, 0, 0)],      # 50 of 100 shared: at 500 permille
        [(90, 0, 200, 0, 200, 0, 0), (80, 149, 249, 5000, 5100, 0, 0)],      # 51
        [seg, (85, 90, 190, 1090 - 1000, 1190 - 1000, 0, 0)],                # a dup
        [seg, (85, 90, 190, 90, 190, 1, 0)], [seg, (85, 90, 190, 90, 190, 0, 1)],      # the other strand, another contig
        [seg, (85, 100, 200, 50, 150, 0, 0)],                                # a tandem copy: ovl_g > 0, ovl_q = 0
        [seg, (85, 90, 190, 100, 200, 0, 0)],                                # the reference intervals touch
        [(40, 0, 10, 0, 10, 0, 0), (39, 20, 30, 50, 60, 0, 0)],              # the min_score border
        [seg, (39, 50, 300, 5000, 5250, 0, 0)], [seg, (39, 51, 300, 5000, 5249, 0, 0)],      # half of the segment, one base less
        [seg, (50, 50, 300, 5000, 5250, 0, 0)], [seg, (50, 51, 300, 5000, 5249, 0, 0)],
        [(50, 0, 100, 0, 100, 0, 0), (60, 0, 100, 500, 600, 0, 0), (60, 0, 100, 900, 1000, 0, 0)],        # a score tie
        [(2 ** 43, 0, 100, 2 ** 61, 2 ** 61 + 100, 0, 0), (2 ** 43 - 1, 100, 200, 0, 100, 1, 0), (2 ** 43 + 1, 50, 150, 2 ** 62, 2 ** 62 + 100, 0, 0),
         (2 ** 32 + 5, 0, 100, 77, 177, 0, 0), (5, 0, 100, 2 ** 33, 2 ** 33 + 100, 0, 0)],             # scores and coordinates beyond 32 bits
        [(100 - k, 10 * k, 10 * k + 10, 1000 * k, 1000 * k + 10, k % 2, 0) for k in range(20)] + [(70, 0, 10, 77000, 77010, 0, 0)],
    ]
    groups = np.concatenate([[0], np.cumsum([len(c) for c in cases])])
    f = _fields([x for c in cases for x in c])
    v = _verifier()
    for min_score, permille, ms in ((40, 500, 8), (40, 499, 8), (40, 510, 2), (40, 0, 16), (40, 1000, 16), (39, 500, 1), (1, 250, 16)):
        _check_pick(v, f, groups, min_score, permille, ms, f"thresholds {min_score}/{permille}/{ms}", contig=f["contig"])
        _check_pick(v, f, groups, min_score, permille, ms, f"thresholds {min_score}/{permille}/{ms}, one contig")
    want = _check_pick(v, f, groups, 40, 500, 8, "thresholds", contig=f["contig"])
    assert want["n_seg"][:7].tolist() == [2, 1, 1, 2, 2, 2, 2] and want["s2"][8, 0] == 39 and want["s2"][9, 0] == NONE
    g13 = int(groups[13])                                        # 50 shared bases of 100 are no conflict at 500 permille
    assert want["seg"][13, :4].tolist() == [g13 + 2, g13, g13 + 1, BEYOND] and want["s2"][13, :3].tolist() == [2 ** 32 + 5, 2 ** 32 + 5, NONE]
    v.close()


@pytest.mark.gpu
def test_pick_alone_on_random_groups():
    """1 000 random groups of 0 .. 11 candidates (every fiftieth of up to 200) over few scores, short reads and a small genome,
    so that ties, overlaps at the threshold and dups are common."""
    rng = np.random.default_rng(74)
    sizes = np.where(np.arange(1000) % 50 == 7, rng.integers(60, 200, 1000), rng.integers(0, 12, 1000))
    groups = np.concatenate([[0], np.cumsum(sizes)])
    n = int(groups[-1])
    m = np.repeat(rng.integers(20, 60, 1000), sizes)
    q_lo = rng.integers(0, m)
    f = dict(score=(rng.integers(0, 8, n) * 5 - 5).tolist(), q_lo=q_lo.tolist(), q_hi=(q_lo + rng.integers(0, m - q_lo + 1)).tolist(),
             rc=rng.integers(0, 2, n).tolist())
    g_lo = rng.integers(0, 120, n)
    f["g_lo"], f["g_hi"] = g_lo.tolist(), (g_lo + rng.integers(0, 40, n)).tolist()
    contig = rng.integers(0, 2, n).tolist()
    v = _verifier()
    chosen = 0
    for min_score, permille, ms, cn in ((1, 500, 8, contig), (10, 250, 3, None), (20, 0, 16, contig), (1, 1000, 16, None), (1, 999, 1, contig)):
        chosen += int(_check_pick(v, f, groups, min_score, permille, ms, f"random {min_score}/{permille}/{ms}", contig=cn)["n_seg"].sum())
    v.close()
    assert chosen > 5000


# ------------------------------------------------------------------------------------------------ 3. the whole call

CONTIG = 200_000                                                  # plain_genome as two contigs: [0, CONTIG) and the rest


def _chimeras(rng, g, count=200, m=600, width=640):
    """`count` reads of `m` bases in two or three parts from unrelated places of g, either strand each, 2 % edits.  Per part a
    candidate whose window holds the part where the whole read would lie around it -- as the locator places a long read's
    window --, for every other part a second candidate from a window shifted by a few bases (the same alignment through
    another bucket), and two windows at unrelated places; the candidates of a read in shuffled order.  Returns the batch, the
    groups, contig per alignment, and per read the parts as (q_lo, q_hi, text_rc, genome interval)."""
    b, groups, contig, truth = _Batch(), [0], [], []
    for r in range(count):
        cuts = [int(rng.integers(150, m - 150))]                # every part has at least 150 bases
        if r % 2:
            cuts = [int(rng.integers(150, m - 300))]
            cuts.append(int(rng.integers(cuts[0] + 150, m - 149)))
        edges = [0] + cuts + [m]
        read, parts, cands = [], [], []
        for k in range(len(edges) - 1):
            lo, hi, rc = edges[k], edges[k + 1], int(rng.integers(0, 2))
            # the part's bases lie at genome [at, at + len); the read as a whole would begin `lo` (forward) or m - hi (reverse)
            # bases before them
            lead = m - hi if rc else lo
            at = int(rng.integers(lead + 40, len(g) - m - 80))
            if at < CONTIG <= at + m:
                at -= 2 * m                                    # (no part across the contig border)
            src = g[at: at + hi - lo]
            read.append(_mutate(rng, _revcomp(src) if rc else src, 0.012, 0.004, 0.004))
            parts.append((rc, at, hi - lo, lead))
        edges = np.concatenate([[0], np.cumsum([len(x) for x in read])]).tolist()
        read = np.concatenate(read)
        for k, (rc, at, length, lead) in enumerate(parts):
            start = at - lead - 20
            cands.append((start, rc))
            if (r + k) % 2:
                cands.append((start + int(rng.integers(3, 18)), rc))
        for _ in range(2):
            cands.append((int(rng.integers(0, len(g) - width)), int(rng.integers(0, 2))))
        for k in rng.permutation(len(cands)):
            start, rc = cands[k]
            # every candidate aligns the same read: the batch holds it once per candidate (query_start may repeat, it does not here)
            b.add(read, start, width + len(read) - m, rc)
            contig.append(int(start >= CONTIG))
        groups.append(len(contig))
        truth.append([(edges[k], edges[k + 1], rc, at, at + length) for k, (rc, at, length, lead) in enumerate(parts)])
    return b.args(), np.array(groups, np.uint32), np.array(contig, np.uint32), truth


def _whole_call(v, g, made, align, what):
    batch, groups, contig, truth = made
    score, begin, off, cg = align(*batch)
    want = _ranges(g, batch, begin, off, cg, 1, 2)
    clipped = v.clip(*batch, begin, off, cg)
    got = v.split(*batch, begin, off, cg, groups, contig=contig)
    pick = _assert_split(got, want, groups, 40, 500, 8, what, contig=contig, clipped=clipped, batch=batch)
    # the planted parts are what is chosen: every part of at least 150 bases is a segment within a few bases of its place, no
    # read has more segments than parts, and the unrelated windows give none
    found = parts = 0
    for r, read in enumerate(truth):
        segs = [int(a) for a in got["seg"][r, : int(got["n_seg"][r])]]
        assert len(segs) <= len(read), (what, r)
        for q_lo, q_hi, rc, g_lo, g_hi in read:
            parts += 1
            found += any(int(batch[3][a]) == rc and abs(int(got["q_lo"][a]) - q_lo) <= 25 and abs(int(got["q_hi"][a]) - q_hi) <= 25
                         and abs(int(got["g_lo"][a]) - g_lo) <= 25 and abs(int(got["g_hi"][a]) - g_hi) <= 25 for a in segs)
    assert found >= 0.97 * parts, (what, found, parts)
    # chosen segments through clip alone: AS = S
    chosen = got["seg"][got["seg"] != BEYOND].astype(np.int64)
    sub_off, sub_cg = _packed([_unpack(cg[int(off[a]): int(off[a + 1])]) for a in chosen])
    again = v.clip(batch[0], *(x[chosen] for x in batch[1:]), begin[chosen], sub_off, sub_cg)
    assert np.array_equal(again["score"], got["score"][chosen]) and (again["score"] >= 40).all()
    return got, pick, (begin, off, cg)


@pytest.mark.gpu
def test_whole_call_on_planted_chimeric_reads(plain_genome, monkeypatch):
    """200 reads of 600 bases in two and three parts, on both strands and two contigs, with duplicate candidates from
    overlapping windows and unrelated windows mixed in: align_long, then split, against clip_range plus select_segments; the
    same with the aligner cutting every read into tiles (BMV_LONG_FROM=200); and on a reused context after this larger batch a
    smaller one, every row of the other calls unchanged across all of it."""
    rng = np.random.default_rng(75)
    made = _chimeras(rng, plain_genome)
    batch, groups, contig, truth = made
    assert len(contig) > 900 and 0 < contig.sum() < len(contig) and {len(t) for t in truth} == {2, 3}
    v = _verifier()
    v.load_genome(plain_genome)
    got, pick, path = _whole_call(v, plain_genome, made, v.align_long, "after align_long")
    assert (pick["n_seg"] >= 2).mean() > 0.9 and pick["n_seg"].max() == 3
    monkeypatch.setenv("BMV_LONG_FROM", "200")
    _whole_call(v, plain_genome, made, v.align_long, "after align_long in tiles")
    monkeypatch.delenv("BMV_LONG_FROM")
    # a smaller batch on the reused context
    few = tuple(x[: int(groups[7])] if k else x for k, x in enumerate(batch))
    _whole_call(v, plain_genome, (few, groups[:8], contig[: int(groups[7])], truth[:7]), v.align_long, "a smaller batch afterwards")
    # the rows of the other calls, filled by a small batch through align, clip, align_best and pair ...
    small = tuple(x[:40] if k else x for k, x in enumerate(batch))
    results = v.align(*small)
    clip_before = v.clip(*small, *results[1:])
    best_before = v.align_best(*small, [0, 10, 40], [5, 5])
    v.pair(small[1], small[2], small[3], small[5], best_before["edits"], best_before["end"], [0, 10, 40], 1, 1000)
    stats = lambda: (v.stats(), v.clip_stats(), v.best_stats(), v.pair_stats(), v.annotate_stats(), v.realign_stats(), v.leftalign_stats(),
                     v.rescue_stats(), v.bounded_stats())
    rows = lambda: _rows(v, 40, 2, len(clip_before["xcigar"]), len(clip_before["ref_bases"]))
    stats_before, rows_before = stats(), rows()
    # ... are what they were after split calls of every kind: the large batch, the pick alone, a refused call, n = 0 in groups,
    # and no groups at all
    again = v.split(*batch, *path, groups, contig=contig)
    assert all(np.array_equal(again[k], got[k]) for k in got)
    alone = v.split_pick(got["score"], got["q_lo"], got["q_hi"], got["g_lo"], got["g_hi"], batch[3], groups, contig=contig)
    assert all(np.array_equal(alone[k], got[k]) for k in got)
    with pytest.raises(verify.BmvError):
        v.split(*batch, *path, groups, max_segments=17)
    empty = v.split(np.zeros(0, np.uint8), [], [], [], [], [], [], [0], [], [0, 0, 0])
    assert empty["n_seg"].tolist() == [0, 0] and (empty["seg"] == BEYOND).all() and (empty["s2"] == NONE).all() and len(empty["score"]) == 0
    empty = v.split(np.zeros(0, np.uint8), [], [], [], [], [], [], [0], [], [0])
    assert empty["seg"].shape == (0, 8) and v.split_stats() == {"ms_range": 0.0, "ms_pick": 0.0, "columns": 0, "n_segments": 0}
    after = rows()
    assert all(np.array_equal(x, y) for x, y in zip(after, rows_before)), [k for k, (x, y) in enumerate(zip(after, rows_before)) if not np.array_equal(x, y)]
    assert stats() == stats_before
    v.close()


def _rows(v, n, n_groups, n_x, n_r):
    """What bmv_results, bmv_clipped, bmv_best and bmv_pairs return, through the ABI."""
    L = verify.lib()
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    u32, u64, i32, i64, u8 = (lambda k: np.zeros(max(k, 1), np.uint32)), (lambda k: np.zeros(max(k, 1), np.uint64)), \
        (lambda k: np.zeros(max(k, 1), np.int32)), (lambda k: np.zeros(max(k, 1), np.int64)), (lambda k: np.zeros(max(k, 1), np.uint8))
    res = [i32(n), u32(n), u64(n + 1)]                          # (not the entries: their count depends on who aligned last)
    assert L.bmv_results(v._h, p(res[0], C.c_int32), p(res[1], C.c_uint32), p(res[2], C.c_uint64), None) == 0
    cl = [i64(n), u32(n), u32(n), u32(n), u32(n), u32(n), u64(n + 1), u32(n_x), u64(n + 1), u8(n_r)]
    assert L.bmv_clipped(v._h, p(cl[0], C.c_int64), *(p(x, C.c_uint32) for x in cl[1:6]), p(cl[6], C.c_uint64), p(cl[7], C.c_uint32),
                         p(cl[8], C.c_uint64), p(cl[9], C.c_uint8)) == 0
    best = [u32(n_groups), u32(n), u32(n)]
    assert L.bmv_best(v._h, *(p(x, C.c_uint32) for x in best)) == 0
    pr = [u32(n_groups), u8(n_groups // 2), u64(n_groups // 2), u64(n_groups // 2), u32(n_groups)]
    assert L.bmv_pairs(v._h, p(pr[0], C.c_uint32), p(pr[1], C.c_uint8), p(pr[2], C.c_uint64), p(pr[3], C.c_uint64), p(pr[4], C.c_uint32)) == 0
    return res + cl + best + pr


# ------------------------------------------------------------------------------------------------ 4. refusals

@pytest.mark.gpu
def test_refusals_leave_the_context_usable(plain_genome):
    rng = np.random.default_rng(76)
    made = _chimeras(rng, plain_genome, count=12)
    batch, groups, contig, truth = made
    n = len(contig)
    with pytest.raises(verify.BmvError) as e:
        verify.Verifier().split(*batch, np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64), np.zeros(0, np.uint32), groups)
    assert e.value.code == 3                                     # BMV_ERR_STATE: no genome yet
    v = _verifier()
    v.load_genome(plain_genome)
    score, begin, off, cg = v.align(*batch)
    want = _ranges(plain_genome, batch, begin, off, cg, 1, 2)
    check = lambda what: _assert_split(v.split(*batch, begin, off, cg, groups, contig=contig), want, groups, 40, 500, 8, what, contig=contig, batch=batch)
    check("before the refusals")
    before, stats = v._segments(n, len(groups) - 1, 8), v.split_stats()

    def refused(call, *words):
        with pytest.raises(verify.BmvError) as e:
            call()
        assert e.value.code == 1 and all(w in str(e.value) for w in words), str(e.value)
        now = v._segments(n, len(groups) - 1, 8)
        assert all(np.array_equal(now[k], before[k]) for k in before) and v.split_stats() == stats, "a refused call changed the results"

    for kw, word in ((dict(match=0), "1..1024"), (dict(penalty=1025), "1..1024"), (dict(min_score=0), "min_score"),
                     (dict(max_overlap_permille=1001), "max_overlap_permille"), (dict(max_segments=0), "max_segments"),
                     (dict(max_segments=17), "max_segments")):
        refused(lambda: v.split(*batch, begin, off, cg, groups, **kw), "bmv_split", word)
    # what bmv_clip refuses: alignment 2 with an entry of length 0
    cigs = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in range(n)]
    bad = list(cigs)
    bad[2] = [(M, int(batch[5][2]) - 1), (I, 0), (M, 1)]
    o2, c2 = _packed(bad)
    refused(lambda: v.split(*batch, begin, o2, c2, groups), "alignment 2")
    moved = batch[1].copy()
    moved[5] = 2 ** 62 + 5
    refused(lambda: v.split(batch[0], moved, *batch[2:], begin, off, cg, groups), "alignment 5")
    # groups: not from 0, not monotone, not ending at n
    for g, word in (([1] + groups[1:].tolist(), "group_offset[0]"), (groups[:3].tolist() + [0] + groups[4:].tolist(), "group 2"),
                    (groups[:-1].tolist() + [n - 1], f"group {len(groups) - 2}")):
        refused(lambda: v.split(*batch, begin, off, cg, g), word)
    # the pick alone: its own checks
    f = {k: before[k].copy() for k in PER_ALIGNMENT}
    ok = v.split_pick(f["score"], f["q_lo"], f["q_hi"], f["g_lo"], f["g_hi"], batch[3], groups, contig=contig)
    assert all(np.array_equal(ok[k], before[k]) for k in before), "the pick alone over the call's ranges differs from the call"
    stats = v.split_stats()
    assert stats["ms_range"] == 0 and stats["columns"] == 0
    f["q_lo"][3], f["q_hi"][3] = 10, 9
    refused(lambda: v.split_pick(f["score"], f["q_lo"], f["q_hi"], f["g_lo"], f["g_hi"], batch[3], groups), "alignment 3", "q_lo")
    f["q_lo"][3] = 0
    f["g_hi"][4] = f["g_lo"][4] - 1
    refused(lambda: v.split_pick(f["score"], f["q_lo"], f["q_hi"], f["g_lo"], f["g_hi"], batch[3], groups), "alignment 4", "g_lo")
    refused(lambda: v.split_pick([1], [0], [1], [0], [1], [0], [0, 1], max_segments=17), "bmv_split_pick", "max_segments")
    refused(lambda: v.split_pick([1], [0], [1], [0], [1], [0], [0, 2]), "group 0")
    check("after the refusals")
    v.close()


# ------------------------------------------------------------------------------------------------ 5. the tool

TOOL_FLAGS = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "16384", "-r", "100", "-f", "1", "-u", "0", "-q", "r.fastq"]
READ, EDGE = 600, 700
# where a 600-base read is cut: with -r 100 its five sampling windows begin at 0, 125, 250, 375 and 499, so every part of
# these holds at least one window whole
CUTS = ([300], [235, 365], [240], [360], [230, 370])
WINDOWS = (0, 125, 250, 375, 499)


def make_split_job(d, n_chimeric=60, n_plain=40, seed=77):
    """A two-contig genome, `n_chimeric` reads in two or three parts from unrelated places -- either strand, either contig,
    each part placed so that the whole read laid around it stays EDGE bases clear of a 16 384-base bucket border -- and
    `n_plain` ordinary reads, all with a few substitutions.  Returns per read its parts as (q_lo, q_hi, reverse, contig,
    0-based position of the part's first reference base)."""
    from bucket_map_amd import host
    g = host.Genome.synth(seed, [330_000, 170_000])
    recs = [bytearray(bytes(g.record_seq(i))) for i in range(2)]
    rng = np.random.default_rng(seed)
    # four stretches of the first contig lie in the second once more, with four substitutions near one end: the last four
    # ordinary reads come from them, so that a segment has a competitor at another locus (MAPQ below 60)
    repeats = [(16384 * (10 + j) + 3000, 16384 * (2 + j) + 5000) for j in range(4)]
    for src, dst in repeats:
        copy = bytearray(recs[0][src: src + READ])
        for x in range(560, READ, 10) if dst != repeats[0][1] else []:     # (the first copy is exact: MAPQ 0)
            copy[x] = b"ACGT"[(b"ACGT".index(copy[x]) + 1) % 4]
        recs[1][dst: dst + READ] = copy
    recs = [bytes(x) for x in recs]
    with open(d / "g.fa", "w") as f:
        for i, seq in enumerate(recs):
            f.write(f">{g.record_id(i)}\n" + "".join(seq[x: x + 80].decode() + "\n" for x in range(0, len(seq), 80)))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    truth, lines = [], []
    for r in range(n_chimeric + n_plain):
        cuts = list(CUTS[r % len(CUTS)]) if r < n_chimeric else []
        edges = [0] + cuts + [READ]
        read, parts = b"", []
        for k in range(len(edges) - 1):
            lo, hi, rc, c = edges[k], edges[k + 1], int(rng.integers(0, 2)), int(rng.integers(0, 2))
            lead = READ - hi if rc else lo                      # the read as a whole begins `lead` bases before the part
            bucket = int(rng.integers(0, len(recs[c]) // 16384 - 1))
            at = bucket * 16384 + int(rng.integers(EDGE + lead, 16384 - EDGE - READ + lead))
            if r >= n_chimeric + n_plain - len(repeats):
                c, at = 0, repeats[r - (n_chimeric + n_plain - len(repeats))][0]
            src = bytearray(recs[c][at: at + hi - lo])
            # three substitutions a part; a part that holds a single sampling window gets them outside it, so that the locator
            # finds every part (tests check that it does)
            inside = [w for w in WINDOWS if lo <= w and w + 100 <= hi]
            in_read = lambda x: hi - 1 - x if rc else lo + x    # where base x of the part's reference stretch lies in the read
            free = [x for x in range(hi - lo) if len(inside) > 1 or not inside[0] <= in_read(x) < inside[0] + 100]
            for x in rng.choice(free, 3, replace=False):
                src[x] = b"ACGT"[(b"ACGT".index(src[x]) + 1 + int(rng.integers(0, 3))) % 4]
            read += bytes(src).translate(comp)[::-1] if rc else bytes(src)
            parts.append((lo, hi, rc, c, at))
        truth.append(parts)
        lines.append(f"@read{r}\n{read.decode()}\n+\n{'I' * READ}\n")
    open(d / "r.fastq", "w").write("".join(lines))
    return truth, recs


def _run_tool(exe, d, out, *extra, env=None):
    r = subprocess.run([exe, *TOOL_FLAGS, "-o", out, *extra], cwd=str(d), capture_output=True, text=True,
                       env=dict(os.environ, BM_VERIFY_BLOCK_READS="23", **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def expected_split_records(dump_lines, fastq, contigs, match=1, penalty=2, min_score=40, permille=500, max_segments=8):
    """`bucketmap_align --split`'s records restated from the tool's own BM_DUMP_ALIGNMENTS lines (every candidate the
    verifier aligned: read, text start in the concatenated genome, text length, strand, query length, score, begin, CIGAR):
    restate_clip per candidate, select_segments per read, split_mapq and sa_entry per chosen segment.  contigs: (name,
    sequence) in FASTA order; fastq: (name, sequence, qualities) in file order.  Returns the record lines' fields."""
    from test_clip import restate_clip
    flat = "".join(s for _, s in contigs).encode()
    starts = np.cumsum([0] + [len(s) for _, s in contigs])
    by_read = {}
    for line in dump_lines:
        f = line.split()
        if f:
            by_read.setdefault(int(f[0]), []).append(f)
    out = []
    for r, (name, seq, qual) in enumerate(fastq):
        cands = by_read.get(r, [])
        if not cands:
            continue
        clips, fields = [], {k: [] for k in ("score", "q_lo", "q_hi", "g_lo", "g_hi", "rc", "contig")}
        for f in cands:
            ts, tl, rc, m, begin = int(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[6])
            cigar = [("MID".index(op), int(n)) for n, op in re.findall(r"(\d+)([MID])", f[7])]
            c = restate_clip(flat[ts: ts + tl], rc, seq.encode(), begin, cigar, match, penalty)
            clips.append(c)
            cl, cr = c["clip_left"], c["clip_right"]
            fields["score"].append(c["score"]); fields["rc"].append(rc)
            fields["q_lo"].append(cr if rc else cl); fields["q_hi"].append(m - (cl if rc else cr))
            fields["g_lo"].append(ts + c["pos"]); fields["g_hi"].append(ts + c["pos"] + c["ref_len"])
            fields["contig"].append(int(np.searchsorted(starts, ts, side="right")) - 1)
        pick = verify.select_segments(fields["score"], fields["q_lo"], fields["q_hi"], fields["g_lo"], fields["g_hi"], fields["rc"],
                                      [0, len(cands)], min_score, permille, max_segments, fields["contig"])
        segs = []
        for k in range(int(pick["n_seg"][0])):
            a = int(pick["seg"][0, k])
            c, contig = clips[a], fields["contig"][a]
            segs.append(dict(rname=contigs[contig][0], pos=fields["g_lo"][a] - int(starts[contig]), rc=fields["rc"][a], clip=c,
                             mapq=verify.split_mapq(c["score"], pick["s2"][0, k]),
                             packed=[(n << 4) | op for op, n in c["xcigar"]]))
        sa = [verify.sa_entry(s["rname"], s["pos"], s["rc"], s["packed"], s["mapq"], s["clip"]["nm"]) for s in segs]
        for i, s in enumerate(segs):
            rc_seq = seq.translate(str.maketrans("ACGT", "TGCA"))[::-1]
            rec = [name, str((16 if s["rc"] else 0) | (0x800 if i else 0)), s["rname"], str(s["pos"] + 1), str(s["mapq"]),
                   verify.xcigar_string(s["packed"]), "*", "0", "0", rc_seq if s["rc"] else seq, qual[::-1] if s["rc"] else qual,
                   f"NM:i:{s['clip']['nm']}", f"MD:Z:{s['clip']['md']}", f"AS:i:{s['clip']['score']}"]
            if len(segs) > 1:
                rec.append("SA:Z:" + "".join(e for o, e in enumerate(sa) if o != i))
            out.append(rec)
    return out


def check_split_records(recs, contigs, fastq, truth, n_chimeric):
    """Every record walked over the FASTA, and what --split promises about a read's records."""
    ref = dict(contigs)
    reads = {name: (seq, qual) for name, seq, qual in fastq}
    by_read = {}
    for f in recs:
        qname, flag, rname, pos, cigar, seq, qual = f[0], int(f[1]), f[2], int(f[3]), f[5], f[9], f[10]
        tags = dict(t.split(":", 2)[::2] for t in f[11:])
        assert [t[:2] for t in f[11:14]] == ["NM", "MD", "AS"] and set(tags) <= {"NM", "MD", "AS", "SA"} and flag & ~0x810 == 0, f
        ops = [(int(n), op) for n, op in re.findall(r"(\d+)([=XIDS])", cigar)]
        assert "".join(f"{n}{op}" for n, op in ops) == cigar and ops and all(a[1] != b[1] for a, b in zip(ops, ops[1:])), (qname, cigar)
        assert all(op != "S" for _, op in ops[1:-1]) and [op for _, op in ops if op != "S"][0] == "=" and [op for _, op in ops if op != "S"][-1] == "="
        r_seq, r_qual = reads[qname]
        if flag & 16:
            assert seq == r_seq.translate(str.maketrans("ACGT", "TGCA"))[::-1] and qual == r_qual[::-1], qname
        else:
            assert seq == r_seq and qual == r_qual, qname
        chrom, ti, qi, nm, md, run, score = ref[rname], pos - 1, 0, 0, "", 0, 0
        for n, op in ops:
            if op in "SI":
                qi += n
                nm += n if op == "I" else 0
                score -= 2 * n if op == "I" else 0
                continue
            t = chrom[ti: ti + n]
            assert len(t) == n, f"{qname}: the CIGAR leaves {rname}"
            if op == "D":
                md += f"{run}^{t}"
                run, nm, score = 0, nm + n, score - 2 * n
            else:
                same = [a == b for a, b in zip(t, seq[qi: qi + n])]
                assert len(same) == n and (all(same) if op == "=" else not any(same)), f"{qname}: {n}{op} at {ti} does not hold"
                if op == "=":
                    run, score = run + n, score + n
                else:
                    for c in t:
                        md += f"{run}{c}"
                        run = 0
                    nm, score = nm + n, score - 2 * n
                qi += n
            ti += n
        assert qi == len(seq) == READ and (int(tags["NM"]), tags["MD"], int(tags["AS"])) == (nm, md + str(run), score), (qname, tags, nm, md, score)
        s_left = ops[0][0] if ops[0][1] == "S" else 0
        s_right = ops[-1][0] if ops[-1][1] == "S" else 0
        q_lo, q_hi = (s_right, READ - s_left) if flag & 16 else (s_left, READ - s_right)
        merged = re.sub(r"(\d+)[=X]", lambda m: m.group(1) + "M", cigar)
        while re.search(r"(\d+)M(\d+)M", merged):
            merged = re.sub(r"(\d+)M(\d+)M", lambda m: f"{int(m.group(1)) + int(m.group(2))}M", merged, count=1)
        by_read.setdefault(qname, []).append(dict(flag=flag, rname=rname, pos=pos, q_lo=q_lo, q_hi=q_hi, tags=tags,
                                                  sa=f"{rname},{pos},{'-' if flag & 16 else '+'},{merged},{f[4]},{nm};"))
    names = [name for name, _, _ in fastq]
    assert [f[0] for f in recs] == sorted((f[0] for f in recs), key=names.index), "the records are not in read order"
    found = parts = 0
    for r, name in enumerate(names):
        mine = by_read.get(name, [])
        assert mine, f"{name} has no record"
        # one primary, first; every other record supplementary; the SA tags name each other exactly, the others in order
        assert not mine[0]["flag"] & 0x800 and all(x["flag"] & 0x800 for x in mine[1:]), name
        for i, x in enumerate(mine):
            assert x["tags"].get("SA") == ("".join(o["sa"] for k, o in enumerate(mine) if k != i) if len(mine) > 1 else None), (name, i)
        # the chosen stretches share at most half of the shorter one
        for i, x in enumerate(mine):
            for y in mine[:i]:
                ovl = max(0, min(x["q_hi"], y["q_hi"]) - max(x["q_lo"], y["q_lo"]))
                assert ovl * 1000 <= 500 * min(x["q_hi"] - x["q_lo"], y["q_hi"] - y["q_lo"]), name
        assert len(mine) == len(truth[r]), (name, len(mine), len(truth[r]))
        for lo, hi, rc, c, at in truth[r]:
            parts += 1
            found += any(bool(x["flag"] & 16) == bool(rc) and x["rname"] == contigs[c][0] and abs(x["pos"] - 1 - at) <= 12
                         and abs(x["q_lo"] - lo) <= 12 and abs(x["q_hi"] - hi) <= 12 for x in mine)
    assert found == parts, (found, parts)
    return by_read


def _job_inputs(d):
    from test_annotate_gpu import _fasta
    contigs = list(_fasta(d / "g.fa").items())
    lines = open(d / "r.fastq").read().split("\n")
    fastq = [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)]
    return contigs, fastq


def test_the_locator_finds_every_planted_part(tmp_path):
    """On the CPU, with the oracle-backed tool: every planted read has a candidate on the right strand at each of its loci
    (BM_DUMP_ALIGNMENTS), and the records restated from those candidates are true against the FASTA and find every planted
    part at its place -- what the GPU test below asks of the tool's own records."""
    truth, recs = make_split_job(tmp_path)
    exe = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")
    _run_tool(exe, tmp_path, "plain.sam", env={"BM_DUMP_ALIGNMENTS": str(tmp_path / "dump.txt")})
    dump = open(tmp_path / "dump.txt").read().split("\n")
    off = [0, len(recs[0])]
    cands = {}
    for line in dump:
        f = line.split()
        if f:
            cands.setdefault(int(f[0]), []).append((int(f[1]), int(f[2]), int(f[3])))
    for r, parts in enumerate(truth):
        for lo, hi, rc, c, at in parts:
            first = off[c] + at - (READ - hi if rc else lo)     # where the whole read would begin around this part
            assert any(trc == rc and ts <= first + 15 and first + READ - 15 <= ts + tl for ts, tl, trc in cands.get(r, [])), (r, lo, hi, rc, c, at)
    contigs, fastq = _job_inputs(tmp_path)
    want = expected_split_records(dump, fastq, contigs)
    by_read = check_split_records(want, contigs, fastq, truth, 60)
    assert sum(len(v) == 2 for v in by_read.values()) >= 30 and sum(len(v) == 3 for v in by_read.values()) >= 20
    # the oracle-backed verifier has no clipping pass: --split says so
    r = subprocess.run([exe, *TOOL_FLAGS, "-o", "s.sam", "--split"], cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode != 0 and "--split" in r.stderr and "clipping pass" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_bucketmap_align_with_split(tmp_path):
    """60 chimeric and 40 ordinary reads of 600 bases on a two-contig genome: the tool's records are the restatement's, true
    against the FASTA, one primary and 0x800 supplementary records per read tied by SA:Z, every planted part at its place;
    ordinary reads get --clip's record but for the MAPQ; two contexts write the same bytes; and without --split the tool
    writes what the parent commit's build wrote (tests/golden/split_tool_parent.sha256, taken from that build)."""
    truth, _ = make_split_job(tmp_path)
    exe = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    err = _run_tool(exe, tmp_path, "split.sam", "--split", env={"BM_DUMP_ALIGNMENTS": str(tmp_path / "dump.txt")})
    assert "GPU split alignments" in err and "GPU alignment clipping" in err
    contigs, fastq = _job_inputs(tmp_path)
    from test_annotate_gpu import _records
    got = _records(tmp_path / "split.sam")
    want = expected_split_records(open(tmp_path / "dump.txt").read().split("\n"), fastq, contigs)
    assert len(got) == len(want) and all(g == w for g, w in zip(got, want)), next((g, w) for g, w in zip(got, want) if g != w)
    by_read = check_split_records(got, contigs, fastq, truth, 60)
    assert sum(len(v) == 2 for v in by_read.values()) >= 30 and sum(len(v) == 3 for v in by_read.values()) >= 20
    assert {f[4] for f in got} - {"60"}, "every MAPQ is 60: no segment had a competitor"
    # the header is the plain run's; ordinary reads: --clip's record of the same alignment but for the MAPQ
    _run_tool(exe, tmp_path, "plain.sam")
    _run_tool(exe, tmp_path, "clip.sam", "--clip")
    head = lambda p: [l for l in open(tmp_path / p).read().split("\n") if l.startswith("@")]
    assert head("split.sam") == head("plain.sam") == head("clip.sam")
    clip = _records(tmp_path / "clip.sam")
    for name, _, _ in fastq[60:]:
        mine = [f for f in got if f[0] == name]
        assert len(mine) == 1 and any(c[:4] + c[5:] == mine[0][:4] + mine[0][5:] for c in clip if c[0] == name), name
    # other parameters reach the device: one segment a read, and a score nobody reaches
    _run_tool(exe, tmp_path, "one.sam", "--split-max", "1")
    one = _records(tmp_path / "one.sam")
    assert [f for f in one] == [f[:14] for f in got if not int(f[1]) & 0x800] and len(one) == len(fastq)
    _run_tool(exe, tmp_path, "none.sam", "--split-min-score", "601")
    assert _records(tmp_path / "none.sam") == [] and head("none.sam") == head("plain.sam")
    # two contexts: the same bytes
    _run_tool(exe, tmp_path, "split2.sam", "--split", "--gpus", "0,0")
    assert (tmp_path / "split2.sam").read_bytes() == (tmp_path / "split.sam").read_bytes()
    # without --split: the parent's bytes
    _run_tool(exe, tmp_path, "ann.sam", "--annotate")
    golden = dict(line.split()[::-1] for line in open(os.path.join(ROOT, "tests", "golden", "split_tool_parent.sha256")))
    for name in ("plain.sam", "ann.sam", "clip.sam"):
        assert hashlib.sha256((tmp_path / name).read_bytes()).hexdigest() == golden[name], f"{name}: not the parent commit's bytes"
