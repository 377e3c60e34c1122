"""Every entry point of the verifier on a REUSED context, after a larger batch (include/bmv.h).

A context keeps its device buffers: GrowBuf never shrinks, and between calls only six counter words are cleared.  Everything
else is right only if each kernel writes every element it later reads -- also the elements of the items that leave a kernel
early.  So each test here runs, on ONE context, big (n = 2 100: more than one 2 048-item tile of bm_scan.hip.h, so block sums
and the carry are live; 150-base queries), small (3 or 65 items, mostly the ones that leave early, at the low indices where
big left its values; queries of 0, 33, 64 and 200 bases: other words-per-lane classes), empty (n = 0), small, big.  A leftover
of big is in range for buffers that only grow, so a missed initialisation shows as a wrong answer, never as a wild access.

Every comparison is exact: against the CPU oracle of the call (oracle.oracle_c for the alignments, the plain restatements of
bucket_map_amd.verify -- select_best, select_pairs, frag_spans, frag_histogram, clip_range and select_segments, which
tests/test_pair.py, tests/test_frag.py and tests/test_split.py hold against brute force --, tests/test_annotate.py,
tests/test_clip.py, tests/test_realign.py and tests/test_leftalign.py for the rest) and against the same call on a fresh
context.  Timings (the ms_* fields) are compared nowhere.

One state outlives a call on the device: bmv_paired_begin leaves its batch's (edits, end) and group offsets there for
bmv_paired_finish.  The tests "between the two halves" put a larger batch with other offsets through every call that may come
in between, and every call that ends a pending begin through its refusal.

The one place where the oracle covers less than the batch: test_realign.restate_realign is a Python loop over the band (17 ms
per 150-base alignment), so of a BIG realign batch the oracle restates the first 70 alignments, every 16th and the ones either
side of the 2 048 border; the fresh context covers all 2 100.  Every small batch is restated in full.

OWNS, below, is the one table of which call owns which result accessor and which stats call; the last test holds all of them
against it over random sequences of calls."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle_c as oc
from test_align_long_gpu import _verifier
from test_annotate import D, EQ, I, M, X, restate
from test_annotate_gpu import _Batch, _mutate, _plant, _revcomp, _unpack
from test_best_gpu import _Groups
from test_clip import restate_clip
from test_leftalign import restate_leftalign
from test_realign import DEFAULT, restate_realign
from test_rescue_gpu import Jobs

BIG, SMALL, M_BIG, W_BIG = 2100, (3, 65), 150, 170
SMALL_M = (0, 33, 200, 64)
STEPS = ("big", "small", "empty", "small", "big")
REJECTED, BEYOND = -(2 ** 31), 2 ** 32 - 1
FAMILY, FAMILY_AT, FAMILY_LEN = 8, lambda c: 5_000 + 2_500 * c, 400
BAND, CLIP = 16, (1, 2)
SLACK = 1 << 19                       # elements beyond the expected ones in every array an accessor fills: an accessor that
#                                       returns more than its own last call left runs into zeros that the test owns

# Which call owns what (include/bmv.h: every call's "leaves untouched" sentence and the ownership rules above bmv_results):
# a call replaces what ITS accessors and stats calls return and nothing else; a refused call replaces nothing.
OWNS = {
    "align": ("results", "stats"),
    "align_long": ("results", "stats"),
    "align_bounded": ("results", "stats", "bounded_stats"),
    "align_best": ("results", "stats", "best", "best_stats"),
    "align_paired": ("results", "stats", "best", "best_stats", "pairs", "pair_stats"),
    "pair": ("pairs", "pair_stats"),
    "rescue": ("rescued", "rescue_stats"),
    "annotate": ("annotations", "annotate_stats"),
    "clip": ("clipped", "clip_stats"),
    "realign": ("realigned", "realign_stats"),
    "leftalign": ("leftaligned", "leftalign_stats"),
    # bmv_paired_begin with cap > 0, then bmv_paired_finish: bmv_align_paired's rows and bmv_frag's.  (With cap = 0 the two
    # halves ARE align_paired: World.halves_call files them under that key, and the frag row must stay as it was found.)
    "paired_halves": ("results", "stats", "best", "best_stats", "pairs", "pair_stats", "frag", "frag_stats"),
    "frag_spans": ("frag", "frag_stats"),
    "split": ("segments", "split_stats"),
    "split_pick": ("segments", "split_stats"),
}
ACCESSORS = ("results", "best", "pairs", "frag", "rescued", "segments", "annotations", "clipped", "realigned", "leftaligned")
STATS = ("stats", "bounded_stats", "best_stats", "pair_stats", "frag_stats", "rescue_stats", "split_stats", "annotate_stats", "clip_stats",
         "realign_stats", "leftalign_stats")
# what every accessor fills, in the order of its C signature
SHAPES = {"results": ("int32", "uint32", "uint64", "uint32"), "best": ("uint32",) * 3, "pairs": ("uint32", "uint8", "uint64", "uint64", "uint32"),
          "frag": ("uint32", "uint64"), "rescued": ("uint64", "uint32", "uint8", "uint32", "uint32", "uint8"),
          "segments": ("int64", "uint32", "uint32", "int64", "int64", "uint32", "uint32", "int64"),
          "annotations": ("uint32", "uint32", "uint32", "uint64", "uint32", "uint64", "uint8"),
          "clipped": ("int64",) + ("uint32",) * 5 + ("uint64", "uint32", "uint64", "uint8"),
          "realigned": ("int32", "uint32", "uint8", "uint64", "uint32"), "leftaligned": ("uint32", "uint64", "uint32", "uint8", "uint32")}
# the eleven entry points the table had when seeds 1 .. 4 of the last test were drawn: they keep their draws
ELEVEN = ("align", "align_long", "align_bounded", "align_best", "align_paired", "pair", "rescue", "annotate", "clip", "realign", "leftalign")
# big split batches: match and penalty, under which an alignment keeps its longest stretch without an edit; min_score,
# max_overlap_permille -- only stretches that share nine tenths of the shorter one conflict, so a large group fills many slots --,
# max_segments
SPLIT_BIG = ((1, 30), (15, 900, 16))
SPLIT_SIZES = (1, 63, 64, 65, 130)    # their group sizes, over and over: either side of a wave's 64 lanes
PTR = {"int32": C.c_int32, "uint32": C.c_uint32, "uint64": C.c_uint64, "int64": C.c_int64, "uint8": C.c_uint8}


# ------------------------------------------------------------------------------------------------ plumbing

class Call:
    """One call of one entry point: run(v) makes it; want: accessor -> the arrays it must return afterwards, in the order of
    its C signature; counts: stats call -> the count fields the oracle gives (the other count fields are read back after the
    call and must then stay); refused: the error code a refusal must carry (the call then owns nothing); spoils: the refusal
    comes after a sub-batch was handed on, so the call's own row is unspecified until that row's next successful call
    (include/bmv.h)."""

    def __init__(self, entry, what, run, want=None, counts=None, refused=None, spoils=False):
        self.entry, self.what, self.run, self.want, self.counts, self.refused = entry, what, run, want or {}, counts or {}, refused
        self.spoils = OWNS[entry] if spoils else ()
        assert refused is not None or set(self.want) | set(self.counts) == set(OWNS[entry]), (entry, what)


def _read(v, accessor, like):
    from bucket_map_amd import verify
    got = [np.zeros(len(x) + SLACK, x.dtype) for x in like]
    assert getattr(verify.lib(), "bmv_" + accessor)(v._h, *(x.ctypes.data_as(C.POINTER(PTR[x.dtype.name])) for x in got)) == 0
    return got


def _counts(v, name):
    return {k: x for k, x in getattr(v, name)().items() if not k.startswith("ms")}


def _assert_arrays(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g[: len(w)] != w)
        assert bad.size == 0, f"{what}: array {k} differs at {bad[:8]}: got {g[bad[:8]]}, want {w[bad[:8]]}"
        assert not g[len(w):].any(), f"{what}: array {k} holds more than {len(w)} elements"


def _make(v, call, state, what):
    """call on v; then EVERY accessor and stats call returns what its own last successful call left (state), the call's own
    being the oracle's."""
    from bucket_map_amd import verify
    if call.refused is not None:
        with pytest.raises(verify.BmvError) as e:
            call.run(v)
        assert e.value.code == call.refused, f"{what}: {e.value}"
        for name in call.spoils:
            state.pop(name, None)
    else:
        call.run(v)
        for name in OWNS[call.entry]:
            if name in ACCESSORS:
                state[name] = call.want[name]
            else:
                got = _counts(v, name)
                for k, x in call.counts[name].items():
                    assert got[k] == x, f"{what}: {name}[{k}] is {got[k]}, the oracle says {x}"
                state[name] = got
    for name, want in state.items():
        if name in ACCESSORS:
            _assert_arrays(_read(v, name, want), want, f"{what}: bmv_{name}")
        else:
            assert _counts(v, name) == want, f"{what}: {name} changed"


def _fresh_agrees(genome, call, scratch_mb=None):
    """the same call on a context of its own"""
    w = _verifier(scratch_mb)
    w.load_genome(genome)
    try:
        _make(w, call, {}, f"{call.what} on a fresh context")
    finally:
        w.close()


def _five(genome, v, calls, scratch_mb=None, fresh=True):
    state = {}
    for k, step in enumerate(STEPS):
        _make(v, calls[step], state, f"step {k}, {calls[step].what}")
    if fresh:
        for step in ("big", "small", "empty"):
            _fresh_agrees(genome, calls[step], scratch_mb)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.uint64)


def _sized_groups(n, sizes):
    """group offsets over n alignments: groups of sizes[0], sizes[1], ... over and over, the last one cut"""
    off, k = [0], 0
    while off[-1] < n:
        off.append(min(n, off[-1] + sizes[k % len(sizes)]))
        k += 1
    return np.array(off, np.uint32)


def _cut_groups(off, n):
    """the groups of the first n alignments, the last one cut"""
    off = [int(x) for x in off if x <= n]
    return np.array(off if off[-1] == n else off + [n], np.uint32)


def _pack(entries):
    return [(n << 4) | op for op, n in entries]


def _packed(cigars):
    return _offsets([len(c) for c in cigars]), np.array([e for c in cigars for e in _pack(c)], np.uint32)


def _sub(batch, idx):
    """the alignments idx of a batch as a batch of their own (the read buffer stays)"""
    return (batch[0], *(x[idx] for x in batch[1:]))


def _take(full, idx):
    """... and their results out of the whole batch's"""
    s, b, o, c = full
    o = o.astype(np.int64)
    return (s[idx].copy(), b[idx].copy(), _offsets((o[1:] - o[:-1])[idx]),
            np.concatenate([c[o[a]: o[a + 1]] for a in idx] + [np.zeros(0, np.uint32)]).astype(np.uint32))


def _keep_only(full, keep):
    """bmv_results where only the alignments keep[a] carry a result (align_bounded, align_best, align_paired)"""
    s, b, _, c = _take(full, np.flatnonzero(keep))
    o = full[2].astype(np.int64)
    score, begin = np.full(len(keep), REJECTED, np.int32), np.zeros(len(keep), np.uint32)
    score[keep], begin[keep] = s, b
    return [score, begin, _offsets(np.where(keep, o[1:] - o[:-1], 0)), c]


def _distances(full):
    """d and end = begin + the M and D lengths of every alignment"""
    s, b, o, c = full
    run = np.concatenate([[0], np.cumsum(np.where((c & 15) != I, c >> 4, 0).astype(np.int64))])
    return -s.astype(np.int64), b.astype(np.int64) + run[o[1:].astype(np.int64)] - run[o[:-1].astype(np.int64)]


def _cells(batch):
    return int((batch[2].astype(np.uint64) * batch[5].astype(np.uint64)).sum())


# ------------------------------------------------------------------------------------------------ the ground

def _genome():
    """60 kbp: a repeat family (eight copies of 400 bases, diverged by 0 .. 2 %) for ties in best and pair, and stretches of
    homopolymers and dinucleotide runs in which a gap can move."""
    rng = np.random.default_rng(20260101)
    g = rng.choice(list(b"ACGT"), 60_000).astype(np.uint8)
    unit = g[1_000: 1_000 + FAMILY_LEN].copy()
    for c in range(FAMILY):
        g[FAMILY_AT(c): FAMILY_AT(c) + FAMILY_LEN] = _mutate(rng, unit, 0.003 * c, 0, 0)
    for at in range(30_000, 40_000, 250):
        g[at: at + 14] = ord("A")
        g[at + 100: at + 124] = np.tile(np.frombuffer(b"CA", np.uint8), 12)
    return g


def _read_at(rng, g, pos, m, rc, err):
    q = _mutate(rng, g[pos: pos + m + 24], *err)[:m]
    assert len(q) == m
    return _revcomp(q) if rc else q


def _place(rng, g, k, m):
    """where read k comes from: the repeat family, the low-complexity stretches, anywhere"""
    if k % 3 == 0:
        return FAMILY_AT(int(rng.integers(0, FAMILY))) + int(rng.integers(0, FAMILY_LEN - min(m, 160)))
    if k % 3 == 1:
        return 30_000 + int(rng.integers(0, 9_700))
    return int(rng.integers(100, len(g) - m - 200))


def _big_reads(rng, g, err=(0.03, 0.01, 0.01), decoys=False):
    b = _Batch()
    for k in range(BIG):
        rc, pos = k & 1, _place(rng, g, k, M_BIG)
        q = _read_at(rng, g, pos, M_BIG, rc, err)
        if decoys and k % 2:
            pos = (pos + 20_000 + int(rng.integers(0, 9_000))) % (len(g) - 400) + 100
        b.add(q, pos - int(rng.integers(0, 9)), W_BIG, rc)
    return b.args()


class World:
    """The genome and every batch with its oracle, each made once and left unchanged."""

    def __init__(self):
        self.genome = _genome()
        self.memo = {}

    def once(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def align(self, batch):
        return oc.align_batch(self.genome, *batch)

    # ---- align, align_long
    def big_reads(self):
        def make():
            batch = _big_reads(np.random.default_rng(1), self.genome)
            full = self.align(batch)
            assert (full[0] < 0).sum() > BIG * 3 // 4 and len(set(full[1].tolist())) > 8, "big fills the buffers with little"
            return batch, full
        return self.once("big reads", make)

    def small_reads(self, n):
        """Mostly what leaves the aligner early, at the low indices: empty queries, empty views; then real ones of 33, 64 and
        200 bases."""
        def make():
            rng, b, g = np.random.default_rng(2 + n), _Batch(), self.genome
            for k in range(n):
                m, rc, pos = SMALL_M[k % 4], k & 1, int(rng.integers(100, 50_000))
                if k < (2 * n) // 3 and m == 0:
                    b.add(np.zeros(0, np.uint8), pos, 40, rc)                          # an empty query
                elif k < (2 * n) // 3:
                    b.add(_read_at(rng, g, pos, m, rc, (0.03, 0.01, 0.01)), pos, 0, rc)  # an empty view
                else:
                    m = m or 33
                    b.add(_read_at(rng, g, pos, m, rc, (0.03, 0.01, 0.01)), pos - 3, m + 20, rc)
            batch = b.args()
            full = self.align(batch)
            assert (batch[5] == 0).any() and (batch[2] == 0).any() and (full[0] < 0).any()
            return batch, full
        return self.once(("small reads", n), make)

    def align_call(self, entry, batch, full, what):
        fn = {"align": lambda v: v.align(*batch), "align_long": lambda v: v.align_long(*batch)}[entry]
        return Call(entry, what, fn, {"results": list(full)}, {"stats": {"cells": _cells(batch)}})

    def align_calls(self, entry, n):
        empty = _Batch().args()
        return {"big": self.align_call(entry, *self.big_reads(), f"{entry} of {BIG}"),
                "small": self.align_call(entry, *self.small_reads(n), f"{entry} of {n}"),
                "empty": self.align_call(entry, empty, self.align(empty), f"{entry} of 0")}

    # ---- align_bounded
    def bounded_call(self, batch, full, bound, what):
        keep = -full[0].astype(np.int64) <= bound.astype(np.int64)
        return Call("align_bounded", what, lambda v: v.align_bounded(*batch, bound), {"results": _keep_only(full, keep)},
                    {"stats": {"cells": _cells(batch)}, "bounded_stats": {"n_rejected": int((~keep).sum())}}), keep

    def bounded_calls(self, n):
        def big():
            batch = _big_reads(np.random.default_rng(3), self.genome, (0.03, 0.01, 0.01), decoys=True)
            return batch, self.align(batch)
        batch, full = self.once("bounded big", big)
        call, keep = self.bounded_call(batch, full, (8 + np.arange(BIG) % 9).astype(np.uint32), f"align_bounded of {BIG}")
        assert keep.sum() >= BIG // 4 and (~keep).sum() >= BIG // 4, "big must hold rejected and accepted alike"
        calls = {"big": call}

        def small():
            # rejected at exactly bound + 1 (mostly, and first), accepted at the bound, no screen (max_edits >= query_len)
            rng, b, g, kinds = np.random.default_rng(4 + n), _Batch(), self.genome, []
            for k in range(n):
                kind = ("rejected", "accepted", "unscreened")[k % 3] if n == 3 or k >= (2 * n) // 3 else "rejected"
                m, rc, pos = (33, 64, 200)[k % 3], k & 1, int(rng.integers(100, 50_000))
                b.add(_read_at(rng, g, pos, m, rc, (0.15, 0.03, 0.03)), pos - 3, m + 20, rc)
                kinds.append(kind)
            batch = b.args()
            return batch, self.align(batch), kinds
        batch, full, kinds = self.once(("bounded small", n), small)
        d = -full[0].astype(np.int64)
        assert (d >= 1).all()
        bound = np.array([d[k] - 1 if kind == "rejected" else d[k] if kind == "accepted" else batch[5][k] for k, kind in enumerate(kinds)],
                         np.uint32)
        calls["small"], keep = self.bounded_call(batch, full, bound, f"align_bounded of {n}")
        assert keep.tolist() == [kind != "rejected" for kind in kinds] and (bound[np.array(kinds) == "accepted"] < batch[5][np.array(kinds) == "accepted"]).all()
        calls["none survives"], keep = self.bounded_call(batch, full, (d - 1).astype(np.uint32), f"align_bounded of {n}, all rejected")
        assert not keep.any()
        empty = _Batch().args()
        calls["empty"], _ = self.bounded_call(empty, self.align(empty), np.zeros(0, np.uint32), "align_bounded of 0")
        return calls

    # ---- align_best, align_paired, pair
    def big_groups(self):
        """Pairs of 150-base mates from fragments of 250 .. 600 bases; groups of 1 .. 8 candidates: the true window, the copies
        of the repeat family (ties and near ties), the same locus through a shifted window (an exact tie), the other strand,
        somewhere else."""
        def make():
            rng, g, gr, k = np.random.default_rng(5), self.genome, _Groups(), 0
            while len(gr.ts) < BIG:
                frag, flip = int(rng.integers(250, 601)), int(rng.integers(0, 2))
                s = _place(rng, g, k, frag)
                for mate in range(2):
                    size = min(1 + k % 8, BIG - len(gr.ts))
                    k += 1
                    if size == 0:
                        gr.close(0)
                        continue
                    forward = (mate == 0) != bool(flip)
                    pos, rc = (s if forward else s + frag - M_BIG), 0 if forward else 1
                    gr.begin(_read_at(rng, g, pos, M_BIG, rc, (0.02, 0.005, 0.005)))
                    cands = [(pos - int(rng.integers(0, 9)), W_BIG, rc)]
                    home = [c for c in range(FAMILY) if 0 <= pos - FAMILY_AT(c) <= FAMILY_LEN - M_BIG]
                    for j in range(size - 1):
                        if j % 4 == 0 and home:
                            c = (home[0] + 1 + j // 4) % FAMILY
                            cands.append((FAMILY_AT(c) + pos - FAMILY_AT(home[0]) - 4, W_BIG, rc))
                        elif j % 4 == 1:
                            cands.append((pos - int(rng.integers(0, 9)), W_BIG, rc))
                        elif j % 4 == 2:
                            cands.append((pos - 4, W_BIG, 1 - rc))
                        else:
                            cands.append((int(rng.integers(100, len(g) - 400)), W_BIG, int(rng.integers(0, 2))))
                    order = rng.permutation(size)
                    for x in order:
                        gr.add(*cands[x])
                    gr.close(int(np.argmin(order)))
            batch, off = gr.args(), gr.offsets()
            assert len(batch[1]) == BIG and (len(off) - 1) % 2 == 0
            size = np.maximum(np.diff(off.astype(np.int64)), 1)
            true_at = np.array(gr.true_at, np.int64)
            margin = (np.arange(len(off) - 1) * 7 % 13).astype(np.uint32)
            return {"batch": batch, "off": off, "margin": margin, "full": self.align(batch), "contig": (batch[1] >= 30_000).astype(np.uint32),
                    "right": (true_at % size).astype(np.uint32), "wrong": ((true_at + 1) % size).astype(np.uint32)}
        return self.once("big groups", make)

    def small_groups(self, n):
        """n alignments: an empty group, a group of one, a group whose hinted member is the true locus and whose other members
        lie beyond its margin, an empty group -- so pair 0 has no proper combination and pair 1 no second mate --, over and
        over; for 65, one pair of two groups of one on the same strand at the end."""
        def make():
            rng, g, gr, margin, hint = np.random.default_rng(6 + n), self.genome, _Groups(), [], []
            for k in range(n // 3):
                m1, m2 = (33, 64, 200)[k % 3], (200, 33, 64)[k % 3]
                pos = int(rng.integers(100, 25_000))
                gr.close(0)                                                         # an empty group
                gr.begin(_read_at(rng, g, pos, m1, 0, (0.03, 0.01, 0.01)))
                gr.add(pos - 3, m1 + 20, 0)
                gr.close(0)                                                         # a group of one
                gr.begin(_read_at(rng, g, pos + 300, m2, 1, (0.0, 0.0, 0.0)))
                gr.add(41_000 + 97 * k, m2 + 20, 1)                                 # somewhere else: beyond the margin
                gr.add(pos + 300 - 3, m2 + 20, 1)                                   # the hinted one: the true locus, exact
                gr.close(1)
                gr.close(0)                                                         # an empty group
                margin += [5, 5, 1, 5]
                hint += [0, 0, 1, 0]
            for k in range(n - 3 * (n // 3)):                                       # (65: two more, one group each, one strand)
                pos = 45_000 + 400 * k
                gr.begin(_read_at(rng, g, pos, 64, 0, (0.03, 0.0, 0.0)))
                gr.add(pos - 3, 84, 0)
                gr.close(0)
                margin.append(2)
                hint.append(0)
            batch, off = gr.args(), gr.offsets()
            assert len(batch[1]) == n and (len(off) - 1) % 2 == 0
            return {"batch": batch, "off": off, "margin": np.array(margin, np.uint32), "full": self.align(batch), "contig": None,
                    "right": np.array(hint, np.uint32), "wrong": np.array(hint, np.uint32)}
        return self.once(("small groups", n), make)

    def no_groups(self):
        batch = _Batch().args()
        return {"batch": batch, "off": np.zeros(1, np.uint32), "margin": np.zeros(0, np.uint32), "full": self.align(batch), "contig": None,
                "right": None, "wrong": None}

    def best_want(self, gb):
        from bucket_map_amd import verify
        d, end = _distances(gb["full"])
        winner, edits, out_end = verify.select_best(d, end, gb["off"], gb["margin"])
        keep = np.zeros(len(d), bool)
        keep[winner[winner != BEYOND]] = True
        return winner, edits, out_end, keep

    def best_call(self, gb, hint, what):
        batch, off, margin = gb["batch"], gb["off"], gb["margin"]
        winner, edits, out_end, keep = self.best_want(gb)
        return Call("align_best", what, lambda v: v.align_best(*batch, off, margin, gb[hint]),
                    {"results": _keep_only(gb["full"], keep), "best": [winner, edits, out_end]},
                    {"stats": {"cells": _cells(batch)}, "best_stats": {"n_seed": int((np.diff(off.astype(np.int64)) > 0).sum())}})

    def paired_call(self, gb, hint, lo, hi, what):
        from bucket_map_amd import verify
        batch, off, margin, contig = gb["batch"], gb["off"], gb["margin"], gb["contig"]
        winner, edits, out_end, _ = self.best_want(gb)
        want = verify.select_pairs(batch[1], batch[2], batch[3], batch[5], edits, out_end, off, lo, hi, contig)
        keep = np.zeros(len(edits), bool)
        keep[want["pick"][want["pick"] != BEYOND]] = True
        sizes = np.diff(off.astype(np.int64))
        call = Call("align_paired", what, lambda v: v.align_paired(*batch, off, margin, lo, hi, gb[hint], contig),
                    {"results": _keep_only(gb["full"], keep), "best": [winner, edits, out_end],
                     "pairs": [want[k] for k in ("pick", "proper", "s1", "s2", "winner")]},
                    {"stats": {"cells": _cells(batch)}, "best_stats": {"n_seed": int((sizes > 0).sum())},
                     "pair_stats": {"combinations": int((sizes[0::2] * sizes[1::2]).sum())}})
        return call, want

    def pair_call(self, arrays, off, lo, hi, contig, what):
        from bucket_map_amd import verify
        ts, tl, trc, ql, ed, en = arrays
        want = verify.select_pairs(ts, tl, trc, ql, ed, en, off, lo, hi, contig)
        sizes = np.diff(off.astype(np.int64))
        call = Call("pair", what, lambda v: v.pair(ts, tl, trc, ql, ed, en, off, lo, hi, contig),
                    {"pairs": [want[k] for k in ("pick", "proper", "s1", "s2", "winner")]},
                    {"pair_stats": {"combinations": int((sizes[0::2] * sizes[1::2]).sum())}})
        return call, want

    def pair_small(self, n):
        """n alignments by numbers alone: a group of two whose edits are BMV_BEYOND throughout beside a group of one, an empty
        group beside a group of one, over and over."""
        ts, tl, trc, ql, ed, en, off = [], [], [], [], [], [], [0]

        def add(rc, k, edits):
            left = (1_000 if rc == 0 else 1_300) + k
            ts.append(left - (10 if rc else 5)); tl.append(115); trc.append(rc); ql.append(100); ed.append(edits); en.append(105)
        for k in range(n // 4 + 1):
            if len(ts) + 3 <= n:
                add(0, k, BEYOND); add(0, k + 1, BEYOND)
                off.append(len(ts))
                add(1, k, 4)
                off.append(len(ts))
            if len(ts) + 1 <= n and n > 3:
                off.append(len(ts))
                add(1, k, k % 5)
                off.append(len(ts))
        while len(ts) < n:
            add(0, 7, 1)
            off.append(len(ts))
            off.append(len(ts))
        assert len(ts) == n and (len(off) - 1) % 2 == 0
        return (np.array(ts, np.uint64), np.array(tl, np.uint32), np.array(trc, np.uint8), np.array(ql, np.uint32), np.array(ed, np.uint32),
                np.array(en, np.uint32)), np.array(off, np.uint32)

    # ---- frag_spans, paired_begin + paired_finish
    def frag_want(self, arrays, off, cap, contig):
        """verify.frag_spans and frag_histogram: bmv_frag's two arrays and the informative pairs"""
        from bucket_map_amd import verify
        ts, tl, trc, ql, ed, en = arrays
        span = verify.frag_spans(ts, tl, trc, ql, ed, en, off, cap, contig)
        hist = verify.frag_histogram(span, cap)
        assert int(hist.sum()) == (len(off) - 1) // 2 and len(hist) == cap + 1
        return [span, hist], {"n_informative": int((span != 0).sum())}

    def frag_call(self, arrays, off, cap, contig, what):
        ts, tl, trc, ql, ed, en = arrays
        want, counts = self.frag_want(arrays, off, cap, contig)
        return Call("frag_spans", what, lambda v: v.frag_spans(ts, tl, trc, ql, ed, en, off, cap, contig), {"frag": want}, {"frag_stats": counts})

    def frag_small(self, n):
        """n alignments by numbers alone, L = left and R = left + 30 on either strand: a pair with an empty first group; a pair
        of one candidate each that spans 40 .. 99 bases (informative under cap = 100); an unsettled pair -- two known loci in its
        first group --; a settled pair that spans 430 bases (beyond cap = 100); over and over."""
        ts, tl, trc, ql, ed, en, off = [], [], [], [], [], [], [0]

        def add(rc, left, edits, m=30):
            ts.append(left - (10 if rc else 5)); tl.append(m + 15); trc.append(rc); ql.append(m); ed.append(edits); en.append(m + 5)
        k = 0
        while len(ts) < n:
            kind = (0, 1, 2, 3)[k % 4]
            if len(ts) + (1, 2, 3, 2)[kind] > n:
                kind = 0
            if kind == 0:
                off.append(len(ts))
                add(1, 1040 + k, k % 3)
            elif kind == 1:
                add(0, 1000, k % 3)
                off.append(len(ts))
                add(1, 1000 + (40 + (7 * k) % 60) - 30, 0)
            elif kind == 2:
                add(0, 1000, 1); add(0, 1007, 2)
                off.append(len(ts))
                add(1, 1040, 0)
            else:
                add(0, 1000, 0)
                off.append(len(ts))
                add(1, 1400, 0)
            off.append(len(ts))
            k += 1
        assert len(ts) == n and (len(off) - 1) % 2 == 0
        return (np.array(ts, np.uint64), np.array(tl, np.uint32), np.array(trc, np.uint8), np.array(ql, np.uint32), np.array(ed, np.uint32),
                np.array(en, np.uint32)), np.array(off, np.uint32)

    def halves_call(self, gb, hint, cap, lo, hi, what):
        """bmv_paired_begin under cap, then bmv_paired_finish under [lo, hi]: bmv_align_paired's oracle in its rows, and for
        cap > 0 the spans of what bmv_best returns in bmv_frag's.  cap = 0 IS align_paired, and is filed as that: the frag row
        is then nobody's, and _make holds it to what it was."""
        paired, _ = self.paired_call(gb, hint, lo, hi, what)
        batch, off, margin, contig = gb["batch"], gb["off"], gb["margin"], gb["contig"]
        want, counts = dict(paired.want), dict(paired.counts)
        if cap:
            _, edits, out_end, _ = self.best_want(gb)
            want["frag"], counts["frag_stats"] = self.frag_want((batch[1], batch[2], batch[3], batch[5], edits, out_end), off, cap, contig)

        def run(v):
            frag = v.paired_begin(*batch, off, margin, cap, gb[hint], contig)
            assert (frag is None) == (cap == 0)
            v.paired_finish(lo, hi)
        return Call("paired_halves" if cap else "align_paired", what, run, want, counts)

    # ---- split, split_pick
    def split_ranges(self, key, paths, scores):
        """verify.clip_range per alignment: the five per-alignment arrays of bmv_segments"""
        def make():
            from bucket_map_amd import verify
            batch, begins, cigars = paths
            out = {k: [] for k in ("score", "q_lo", "q_hi", "g_lo", "g_hi")}
            for a in range(len(begins)):
                window, rc, query = self.views(batch, a)
                r = verify.clip_range(window, query, rc, begins[a], _pack(cigars[a]), *scores)
                out["score"].append(r["score"]); out["q_lo"].append(r["q_lo"]); out["q_hi"].append(r["q_hi"])
                out["g_lo"].append(int(batch[1][a]) + r["g_off_lo"]); out["g_hi"].append(int(batch[1][a]) + r["g_off_hi"])
            return [np.array(out[k], t) for k, t in (("score", np.int64), ("q_lo", np.uint32), ("q_hi", np.uint32), ("g_lo", np.int64), ("g_hi", np.int64))]
        return self.once(("split ranges", key, scores), make)

    def split_call(self, entry, key, paths, five, off, contig, scores, params, what):
        """bmv_split on paths or bmv_split_pick on `five`, their ranges: the ranges as given and verify.select_segments over them"""
        from bucket_map_amd import verify
        batch, begins, cigars = paths
        pick = self.once(("split pick", key, scores, params, contig is None),
                         lambda: verify.select_segments(*five, batch[3], off, *params, contig))
        want = [*five, pick["n_seg"], pick["seg"].reshape(-1), pick["s2"].reshape(-1)]
        counts = {"columns": int(sum(k for c in cigars for _, k in c)) if entry == "split" else 0, "n_segments": int(pick["n_seg"].sum())}
        if entry == "split":
            c_off, cg = _packed(cigars)
            run = lambda v: v.split(*batch, begins, c_off, cg, off, *scores, *params, contig)                     # noqa: E731
        else:
            run = lambda v: v.split_pick(*five, batch[3], off, *params, contig)                                   # noqa: E731
        return Call(entry, what, run, {"segments": want}, {"split_stats": counts}), pick

    def split_first(self, entry, n, params=None):
        """`entry` on the first n of the 2 100 big paths in groups of SPLIT_SIZES, with contigs"""
        batch, begins, cigars = paths = self.big_paths()
        scores, params = SPLIT_BIG[0], params or SPLIT_BIG[1]
        five = [x[:n] for x in self.split_ranges("big", paths, scores)]
        off = _cut_groups(_sized_groups(BIG, SPLIT_SIZES), n)
        contig = (batch[1][:n] >= 30_000).astype(np.uint32)
        return self.split_call(entry, ("first", n), (_sub(batch, np.arange(n)), begins[:n], cigars[:n]), five, off, contig, scores, params,
                               f"{entry} of {n}")

    def split_small(self, entry, n, max_segments):
        """`entry` on the small paths in groups of 0, 2 and 2, without contigs: an empty group, a group of an empty CIGAR and an
        alignment without any = column (nobody reaches min_score), a group that has a segment, over and over; then the real ones"""
        paths = self.small_paths(n)
        scores, params = CLIP, (40, 500, max_segments)
        five = self.split_ranges(("small", n), paths, scores)
        return self.split_call(entry, ("small", n), paths, five, _sized_groups(n, (0, 2, 2)), None, scores, params,
                               f"{entry} of {n}, max_segments {max_segments}")

    def split_calls(self, entry, n):
        """the five steps: 16 segments a group and contigs in big; 1, then 3, and no contigs in small"""
        none = (_Batch().args(), [], [])
        five = [np.zeros(0, t) for t in (np.int64, np.uint32, np.uint32, np.int64, np.int64)]
        empty, _ = self.split_call(entry, "empty", none, five, np.zeros(1, np.uint32), None, CLIP, (40, 500, 8), f"{entry} of 0")
        big, pick = self.split_first(entry, BIG)
        steps = [big, self.split_small(entry, n, 1)[0], empty, self.split_small(entry, n, 3)[0], big]
        return steps, pick

    # ---- rescue
    def rescue_want(self, args, lo, hi):
        """test_rescue_gpu.expected with the CPU aligner: the Python-planned view, the oracle on it, d <= k, select_pairs'
        proper."""
        from bucket_map_amd import verify
        reads, ats, atl, arc, aql, aen, c0, c1, qs, ql, me = args
        n = len(ats)
        view = [verify.rescue_window(ats[j], atl[j], arc[j], aql[j], aen[j], c0[j], c1[j], ql[j], me[j], lo, hi) for j in range(n)]
        ts, tl = np.array([w[0] for w in view], np.uint64), np.array([w[1] for w in view], np.uint32)
        trc = np.array([w[2] for w in view], np.uint8)
        edits, end, proper = np.full(n, BEYOND, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        real = np.flatnonzero((tl > 0) & (ql > 0))
        if len(real):
            d, e = _distances(self.align((reads, ts[real], tl[real], trc[real], qs[real], ql[real])))
            for j, dj, ej in zip(real, d, e):
                if dj > min(int(me[j]), int(ql[j])):
                    continue
                edits[j], end[j] = dj, ej
                proper[j] = verify.select_pairs([int(ats[j]), view[j][0]], [int(atl[j]), view[j][1]], [int(arc[j]), view[j][2]],
                                                [int(aql[j]), int(ql[j])], [0, int(dj)], [int(aen[j]), int(ej)], [0, 1, 2], lo, hi)["proper"][0]
        return [ts, tl, trc, edits, end, proper]

    def rescue_call(self, args, lo, hi, what, parts=None):
        want = self.once(("rescue want", what), lambda: self.rescue_want(args, lo, hi))
        return Call("rescue", what, lambda v: v.rescue(*args, lo, hi), {"rescued": want}, {"rescue_stats": {} if parts is None else {"parts": parts}})

    def rescue_big(self):
        """2 100 jobs as a tool asks for them (test_rescue_gpu._natural_jobs with mates of 150 bases): an anchor somewhere, its
        mate from a fragment of 151 .. 599 bases or from elsewhere, contigs that hold the window, cut it or miss it."""
        def make():
            rng, g, jobs = np.random.default_rng(7), self.genome, Jobs()
            for x in range(BIG):
                m = aql = M_BIG
                frag, left, anchor_fwd = int(rng.integers(m + 1, 600)), int(rng.integers(3_000, 50_000)), x % 2 == 0
                a_l, q_l = (left, left + frag - m) if anchor_fwd else (left + frag - aql, left)
                at = q_l if x % 7 else 55_000
                q = _revcomp(_mutate(rng, g[at: at + m], 0.03, 0, 0)) if anchor_fwd else _read_at(rng, g, at, m, 0, (0.03, 0.005, 0.005))
                slack = int(rng.integers(0, 12))
                anchor = (a_l - slack, aql + 2 * slack + 1, 0 if anchor_fwd else 1, aql, aql + slack + (0 if anchor_fwd else 1))
                contig = ((0, len(g)), (left + 150, len(g)), (0, left + frag - 60), (left - 2_000, left - 1_000), (0, len(g)))[x % 5]
                jobs.add(q, anchor, contig, int(rng.integers(0, m // 5 + 2)) if x % 11 else 4_000_000_000)
            return jobs.args()
        return self.once("rescue big", make)

    def rescue_small(self, n):
        """m = 0, an empty view, a view shorter than m - k, a query of 600 bases (the aligner's fallback) -- 3: one of each,
        which makes four jobs; 65: over and over, then planted mates of 33, 64 and 200 bases."""
        def make():
            rng, g, jobs = np.random.default_rng(8 + n), self.genome, Jobs()
            for k in range(max(n, 4)):
                start, rc = 2_000 + 700 * k, k & 1
                kind = k % 4 if k < max(4, (2 * n) // 3) else 4
                if kind == 0:
                    jobs.add_view(np.zeros(0, np.uint8), start, 300, rc, 5)
                elif kind == 1:
                    jobs.add_view(_read_at(rng, g, start, 33, rc, (0.0, 0.0, 0.0)), start, 0, rc, 5)
                elif kind == 2:
                    jobs.add_view(_read_at(rng, g, start, 200, rc, (0.0, 0.0, 0.0)), start, 64, rc, 2)
                elif kind == 3 and k < 12:
                    jobs.add_view(_read_at(rng, g, start + 40, 600, rc, (0.02, 0.005, 0.005)), start, 690, rc, 60)
                else:
                    m = (33, 64, 200)[k % 3]
                    jobs.add_view(_read_at(rng, g, start + 30, m, rc, (0.03, 0.01, 0.01)), start, m + 120, rc, m // 8)
            return jobs.args()
        return self.once(("rescue small", n), make)

    # ---- annotate, clip, realign, leftalign
    def big_paths(self):
        """2 100 long, indel-rich edit paths: the oracle's CIGARs of reads with 3 % substitutions and 2 % + 2 % indels"""
        def make():
            batch = _big_reads(np.random.default_rng(9), self.genome, (0.03, 0.02, 0.02))
            _, begin, off, cg = self.align(batch)
            cigars = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in range(BIG)]
            assert sum(len(c) for c in cigars) > 6 * BIG and {M, I, D} <= {op for c in cigars for op, _ in c}
            return batch, [int(x) for x in begin], cigars
        return self.once("big paths", make)

    def small_paths(self, n):
        """An empty CIGAR, an all-M CIGAR without any = column, an alignment bmv_realign passes through (a D entry of
        64 - 2 BAND bases), an all-M CIGAR of matches, over and over at the low indices; 65: then the oracle's CIGARs of reads of
        33, 64 and 200 bases."""
        def make():
            rng, g, b, planted = np.random.default_rng(10 + n), self.genome, _Batch(), {}
            for k in range(n):
                rc, kind = k & 1, k % 4 if n == 3 or k < (2 * n) // 3 else 4
                if kind == 0:
                    b.add(rng.choice(list(b"ACGT"), 64).astype(np.uint8), int(rng.integers(0, 50_000)), 70, rc)
                    planted[k] = (int(rng.integers(0, 5)), [])
                elif kind == 1:
                    planted[k] = _plant(rng, g, b, [(X, 33)], rc, exact=True)
                elif kind == 2:
                    planted[k] = _plant(rng, g, b, [(EQ, 100), (D, 64 - 2 * BAND), (EQ, 100)], rc, exact=True)
                elif kind == 3:
                    planted[k] = _plant(rng, g, b, [(EQ, 64)], rc, exact=True)
                else:
                    m, pos = (33, 64, 200)[k % 3], int(rng.integers(30_000, 39_000))
                    b.add(_read_at(rng, g, pos, m, rc, (0.03, 0.02, 0.02)), pos - 3, m + 20, rc)
            batch = b.args()
            _, begin, off, cg = self.align(batch)
            begins = [int(x) for x in begin]
            cigars = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in range(n)]
            for k, (bg, c) in planted.items():
                begins[k], cigars[k] = bg, c
            return batch, begins, cigars
        return self.once(("small paths", n), make)

    def views(self, batch, a):
        reads, ts, tl, trc, qs, ql = batch
        return (bytes(self.genome[int(ts[a]): int(ts[a]) + int(tl[a])]), int(trc[a]), bytes(reads[int(qs[a]): int(qs[a]) + int(ql[a])]))

    def restated(self, entry, paths, which=None):
        """the restatement of `entry` for the alignments `which` (all) of paths: a dict a -> its output"""
        batch, begins, cigars = paths
        fn = {"annotate": restate, "clip": lambda *x: restate_clip(*x, *CLIP), "realign": lambda *x: restate_realign(*x, DEFAULT, BAND),
              "leftalign": restate_leftalign}[entry]
        return {a: fn(*self.views(batch, a), begins[a], cigars[a]) for a in (range(len(begins)) if which is None else which)}

    def path_call(self, entry, key, paths, what, which=None):
        """The call of `entry` on paths.  which: the alignments the restatement covers (a big realign); the call's arrays are
        then the fresh context's, held against the restatement where it speaks."""
        batch, begins, cigars = paths
        off, cg = _packed(cigars)
        n, ql = len(begins), batch[5].astype(np.int64)
        columns = int(sum(k for c in cigars for _, k in c))
        w = self.once(("restated", entry, key), lambda: self.restated(entry, paths, which))
        flat = lambda lists: np.array([e for x in lists for e in _pack(x)], np.uint32)                  # noqa: E731
        if entry == "annotate":
            ws = [w[a] for a in range(n)]
            want = [np.array([x[3] for x in ws], np.uint32), np.array([x[0] for x in ws], np.uint32), np.array([x[1] for x in ws], np.uint32),
                    _offsets([len(x[2]) for x in ws]), flat([x[2] for x in ws]), _offsets([len(x[4]) for x in ws]),
                    np.frombuffer(b"".join(x[4] for x in ws), np.uint8)]
            return Call(entry, what, lambda v: v.annotate(*batch, begins, off, cg), {"annotations": want}, {"annotate_stats": {"columns": columns}})
        if entry == "clip":
            ws = [w[a] for a in range(n)]
            want = [np.array([x["score"] for x in ws], np.int64)] + [np.array([x[k] for x in ws], np.uint32) for k in
                                                                     ("clip_left", "clip_right", "nm", "pos", "ref_len")]
            want += [_offsets([len(x["xcigar"]) for x in ws]), flat([x["xcigar"] for x in ws]), _offsets([len(x["ref_bases"]) for x in ws]),
                     np.frombuffer(b"".join(x["ref_bases"] for x in ws), np.uint8)]
            return Call(entry, what, lambda v: v.clip(*batch, begins, off, cg, *CLIP), {"clipped": want}, {"clip_stats": {"columns": columns}})
        if entry == "leftalign":
            ws = [w[a] for a in range(n)]
            want = [np.array([x["begin"] for x in ws], np.uint32), _offsets([len(x["cigar"]) for x in ws]), flat([x["cigar"] for x in ws]),
                    np.array([x["changed"] for x in ws], np.uint8), np.array([x["dropped"] for x in ws], np.uint32)]
            counts = {"compared": sum(x["compared"] for x in ws), "n_changed": sum(x["changed"] for x in ws),
                      "merges": sum(x["merges"] for x in ws), "dropped": sum(x["dropped"] for x in ws)}
            return Call(entry, what, lambda v: v.leftalign(*batch, begins, off, cg), {"leftaligned": want}, {"leftalign_stats": counts})
        run = lambda v: v.realign(*batch, begins, off, cg, *DEFAULT, BAND)                                    # noqa: E731
        passed = np.array([not c or max([k for op, k in c if op == D], default=0) > 63 - 2 * BAND for c in cigars], bool)   # (the header's rule)
        counts = {"cells": 64 * int(ql[~passed].sum()), "n_passed_through": int(passed.sum())}
        if which is None:
            ws = [w[a] for a in range(n)]
            assert [x["realigned"] for x in ws] == (~passed).astype(int).tolist()
            want = [np.array([x["score"] for x in ws], np.int32), np.array([x["begin"] for x in ws], np.uint32),
                    np.array([x["realigned"] for x in ws], np.uint8), _offsets([len(x["cigar"]) for x in ws]), flat([x["cigar"] for x in ws])]
        else:
            want = self.memo[("fresh realign", key)]
            o = want[3].astype(np.int64)
            for a, x in w.items():
                got = dict(score=int(want[0][a]), begin=int(want[1][a]), realigned=int(want[2][a]), cigar=_unpack(want[4][o[a]: o[a + 1]]))
                assert got == x, f"{what}: alignment {a} on a fresh context differs from the restatement"
        return Call(entry, what, run, {"realigned": want}, {"realign_stats": counts})

    def path_calls(self, entry, n):
        none = (_Batch().args(), [], [])
        which = None
        if entry == "realign":                                  # (the module's docstring: what of big the restatement covers)
            which = sorted(set(range(70)) | set(range(0, BIG, 16)) | set(range(2040, 2056)))
            self.fresh_realign("big", self.big_paths())
        return {"big": self.path_call(entry, "big", self.big_paths(), f"{entry} of {BIG}", which),
                "small": self.path_call(entry, n, self.small_paths(n), f"{entry} of {n}"),
                "empty": self.path_call(entry, 0, none, f"{entry} of 0")}

    def fresh_realign(self, key, paths):
        def make():
            batch, begins, cigars = paths
            w = _verifier()
            w.load_genome(self.genome)
            got = w.realign(*batch, begins, *_packed(cigars), *DEFAULT, BAND)
            w.close()
            return [got[k] for k in ("score", "begin", "realigned", "cigar_offset", "cigar")]
        return self.once(("fresh realign", key), make)


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture
def ctx(world, request):
    """a context that holds the genome, closed after the test; the parameter: BMV_SCRATCH_MB"""
    v = _verifier(getattr(request, "param", None))
    v.load_genome(world.genome)
    yield v
    v.close()


# ------------------------------------------------------------------------------------------------ one test per entry point

@pytest.mark.gpu
@pytest.mark.parametrize("ctx", [None, 1], indirect=True, ids=["scratch by default", "1 MB of scratch"])
@pytest.mark.parametrize("n", SMALL)
def test_align(world, ctx, n, request):
    """bmv_align.  Stale: out_score and out_begin (an empty query or view must still write its score and begin), nops and offsets
    (the CIGAR lengths of the slots of a piece: an alignment without entries at a slot that held 20), ops_rev and packed, order
    (the class order of 2 100 against that of 3), trace.  Under 1 MB of scratch big goes through in five pieces and small in
    one, so the slots of small are the first piece's of big."""
    _five(world.genome, ctx, world.align_calls("align", n), request.node.callspec.params["ctx"])


@pytest.mark.gpu
@pytest.mark.parametrize("ctx", [None, 1], indirect=True, ids=["scratch by default", "1 MB of scratch"])
@pytest.mark.parametrize("n", SMALL)
def test_align_long(world, ctx, n, request, monkeypatch, capfd):
    """bmv_align_long with BMV_LONG_FROM=64: the 150-base queries of big and the 64- and 200-base ones of small take the tile,
    checkpoint and traceback kernels, the shorter ones bmv_align's own.  Stale: long_slots and long_tiles (2 100 slots, then
    one or a few), trace (the checkpoints and bottom-row minima of big's regions), ops_rev / nops / offsets, out_score and
    out_begin of the alignments the short sub-batch wrote before the long ones overwrite the batch's.  Under 1 MB of scratch
    big goes through in several pieces and small in one."""
    scratch_mb = request.node.callspec.params["ctx"]
    monkeypatch.setenv("BMV_LONG_FROM", "64")
    monkeypatch.setenv("BMV_LOG_CLASSES", "1")
    calls, state, pieces = world.align_calls("align_long", n), {}, {}
    for k, step in enumerate(STEPS):
        capfd.readouterr()
        _make(ctx, calls[step], state, f"step {k}, {calls[step].what}")
        pieces[step] = capfd.readouterr().err.count("[bmv] long piece of")
    if scratch_mb:
        assert pieces["big"] > 1 and pieces["small"] == 1 and pieces["empty"] == 0, pieces
    monkeypatch.delenv("BMV_LOG_CLASSES")
    for step in ("big", "small", "empty"):
        _fresh_agrees(world.genome, calls[step], scratch_mb)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_align_bounded(world, ctx, n):
    """bmv_align_bounded.  Stale: keep (uploaded as ones: a screened alignment the kernel leaves early must still be a one or
    a zero of THIS call), keep_at and scan_tmp (the survivors' prefix sum: 2 100 is two tiles, 3 is one), survivors,
    screen_list, max_edits; then the aligner's buffers under a sub-batch of another size than the batch.  Small: rejected at
    exactly bound + 1 (the screen must not reject at the bound), accepted at the bound, max_edits >= query_len (no screen); and
    a batch with no survivor, after which the aligner has seen an empty sub-batch right after a full one."""
    calls = world.bounded_calls(n)
    _five(world.genome, ctx, calls)
    state = {}
    for k, step in enumerate(("none survives", "small", "big", "none survives")):
        _make(ctx, calls[step], state, f"step {5 + k}, {calls[step].what}")
    _fresh_agrees(world.genome, calls["none survives"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_align_best(world, ctx, n):
    """bmv_align_best.  Stale: bs_d and bs_end (uploaded whole before the distance round: a listed alignment the kernel proves
    beyond must write BMV_BEYOND over big's distance), bs_bound, bs_list, bs_full, bs_winner and bs_need (an empty group writes
    BMV_BEYOND and 0), bs_need_at and scan_tmp (470 groups against 4), bs_realign, bs_edits and bs_out_end (beyond the margin:
    BMV_BEYOND and 0).  Big: groups of 1 .. 8 with ties, the hint wrong the first time and right the second."""
    big, small, none = world.big_groups(), world.small_groups(n), world.no_groups()
    winner, edits, _, _ = world.best_want(small)
    off = small["off"].astype(np.int64)
    sizes = np.diff(off)
    assert (sizes == 0).sum() >= 2 and (sizes == 1).any() and (winner[sizes == 0] == BEYOND).all()
    for g in np.flatnonzero(sizes == 2):                       # every member but the hinted one lies beyond its margin
        others = np.delete(np.arange(off[g], off[g + 1]), small["right"][g])
        assert winner[g] == off[g] + small["right"][g] and (edits[others] == BEYOND).all()
    w_big, e_big, _, _ = world.best_want(big)
    d_big = _distances(big["full"])[0]
    ties = sum(int((d_big[off_g: off_h] == d_big[w]).sum() > 1) for off_g, off_h, w in zip(big["off"][:-1], big["off"][1:], w_big) if w != BEYOND)
    assert ties > 50 and (e_big == BEYOND).sum() > BIG // 10 and (w_big != big["off"][:-1] + big["right"])[w_big != BEYOND].sum() > 20
    calls = {"big": world.best_call(big, "wrong", f"align_best of {BIG}, wrong hints"), "small": world.best_call(small, "right", f"align_best of {n}"),
             "empty": world.best_call(none, "right", "align_best of 0")}
    state = {}
    for k, step in enumerate(STEPS):
        call = world.best_call(big, "right", f"align_best of {BIG}, right hints") if k == 4 else calls[step]
        _make(ctx, call, state, f"step {k}, {call.what}")
    for step in ("big", "small", "empty"):
        _fresh_agrees(world.genome, calls[step])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_align_paired(world, ctx, n):
    """bmv_align_paired.  Stale: what bmv_align_best leaves (above) and pr_pick, pr_winner, pr_proper, pr_s1, pr_s2 (a pair
    with an empty mate or without a proper combination must write its own winners, 0 and BMV_PAIR_NONE), pr_contig (big passes
    contigs, small none), bs_group_offset (uploaded by the pick, or by the pair kernel's host step when every group is its seed
    alone).  Small: pair 0 has no proper combination, pair 1 no second mate."""
    big, small, none = world.big_groups(), world.small_groups(n), world.no_groups()
    calls = {}
    calls["big"], want = world.paired_call(big, "wrong", 200, 700, f"align_paired of {BIG}")
    assert want["proper"].sum() > 50 and (want["proper"] == 0).any() and (want["s2"] != 2 ** 64 - 1).any()
    calls["small"], want = world.paired_call(small, "right", 200, 700, f"align_paired of {n}")
    sizes = np.diff(small["off"].astype(np.int64))
    assert not want["proper"].any() and (sizes[1::2] == 0).any() and (sizes[0::2] == 0).any() and (want["pick"] != BEYOND).any()
    calls["empty"], _ = world.paired_call(none, "right", 200, 700, "align_paired of 0")
    _five(world.genome, ctx, calls)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_pair(world, ctx, n):
    """bmv_pair, by numbers alone: big is what bmv_align_best's oracle leaves for the 2 100 alignments of its big batch, with
    contigs.  Stale: bs_edits and bs_out_end (shared with bmv_align_best), bs_group_offset, pr_contig -- small passes
    contig = NULL after a call that passed contigs, so the kernel must not read the contigs that lie there --, pr_pick,
    pr_winner, pr_proper, pr_s1, pr_s2.  Small: BMV_BEYOND throughout one group of every pair that has two mates."""
    big = world.big_groups()
    _, edits, out_end, _ = world.best_want(big)
    b = big["batch"]
    calls = {}
    calls["big"], want = world.pair_call((b[1], b[2], b[3], b[5], edits, out_end), big["off"], 200, 700, big["contig"], f"pair of {BIG}")
    assert want["proper"].sum() > 50 and len(set(big["contig"].tolist())) == 2
    arrays, off = world.pair_small(n)
    calls["small"], want = world.pair_call(arrays, off, 200, 700, None, f"pair of {n}")
    assert (want["winner"] == BEYOND).any() and not want["proper"].any() and (arrays[4][off[0]: off[1]] == BEYOND).all()
    calls["empty"], _ = world.pair_call(tuple(x[:0] for x in arrays), np.zeros(1, np.uint32), 200, 700, None, "pair of 0")
    _five(world.genome, ctx, calls)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_rescue(world, ctx, n, monkeypatch):
    """bmv_rescue: big with BMV_RESCUE_PARTS=8, small and empty as the host chooses, the last big with BMV_RESCUE_PARTS=1.
    Stale: rs_text_start / rs_text_len / rs_text_rc (the plan kernel writes every job's view, also an empty one), rs_list,
    rs_d and rs_end (uploaded whole as BMV_BEYOND / 0 before the distance kernel: m = 0, an empty view and a view shorter than
    m - k never enter it or leave it at once), rs_out_edits, rs_out_end, rs_out_proper (the finish kernel writes every job);
    the query of 600 bases goes through bmv_align_long, which must leave bmv_results alone and whose buffers hold big's."""
    from bucket_map_amd import verify
    big, small = world.rescue_big(), world.rescue_small(n)
    calls = {"big": world.rescue_call(big, 1, 600, f"rescue of {BIG}", 8), "small": world.rescue_call(small, 1, 5000, f"rescue of {n} kinds that leave early"),
             "empty": world.rescue_call(tuple(x[:0] for x in big), 1, 600, "rescue of 0", 1)}
    w = calls["big"].want["rescued"]
    assert w[5].sum() > BIG // 8 and (w[1] == 0).sum() > BIG // 10 and (w[3] == verify.BEYOND).sum() > BIG // 8
    ts, tl, trc, edits, end, proper = calls["small"].want["rescued"]
    ql, me = small[9].astype(np.int64), small[10].astype(np.int64)
    early = (ql == 0) | (tl == 0) | (tl < ql - np.minimum(me, ql))
    assert (ql == 0).any() and ((tl == 0) & (ql > 0)).any() and ((tl > 0) & (tl < ql - me)).any() and (ql > 512).any()
    assert (edits[early] == verify.BEYOND).all() and (edits[ql > 512] != verify.BEYOND).all()
    last = world.rescue_call(big, 1, 600, f"rescue of {BIG}", 1)
    state = {}
    for k, step in enumerate(STEPS):
        if k == 0:
            monkeypatch.setenv("BMV_RESCUE_PARTS", "8")
        elif k == 4:
            monkeypatch.setenv("BMV_RESCUE_PARTS", "1")
        else:
            monkeypatch.delenv("BMV_RESCUE_PARTS", raising=False)
        call = last if k == 4 else calls[step]
        _make(ctx, call, state, f"step {k}, {call.what}")
    monkeypatch.delenv("BMV_RESCUE_PARTS")
    _fresh_agrees(world.genome, calls["small"])
    _fresh_agrees(world.genome, calls["empty"])
    monkeypatch.setenv("BMV_RESCUE_PARTS", "8")
    _fresh_agrees(world.genome, calls["big"])


def _assert_small_paths(world, n):
    """what the small batch of the four passes claims to hold, on the restatements' output"""
    paths = world.small_paths(n)
    cigars = paths[2]
    kinds = [k % 4 for k in range(n) if n == 3 or k < (2 * n) // 3]
    ann, cl = world.restated("annotate", paths, range(len(kinds))), world.restated("clip", paths, range(len(kinds)))
    ra, la = world.restated("realign", paths, range(len(kinds))), world.restated("leftalign", paths, range(len(kinds)))
    for k, kind in enumerate(kinds):
        if kind == 0:
            assert cigars[k] == [] and ann[k][2] == [] and cl[k]["xcigar"] == [] and ra[k]["realigned"] == 0 and la[k]["changed"] == 0
        elif kind == 1:                                        # all M, no = column: clip keeps the empty range
            assert [op for op, _ in cigars[k]] == [M] and EQ not in [op for op, _ in ann[k][2]] and cl[k]["xcigar"] == [(4, 33)]
            assert la[k]["changed"] == 0 and la[k]["cigar"] == cigars[k]
        elif kind == 2:                                        # passed through
            assert ra[k]["realigned"] == 0 and ra[k]["cigar"] == cigars[k]
        else:                                                  # all M, all =: unchanged
            assert [op for op, _ in ann[k][2]] == [EQ] and la[k]["changed"] == 0 and la[k]["cigar"] == cigars[k] and ra[k]["realigned"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("entry", ["annotate", "clip", "realign", "leftalign"])
def test_the_passes_over_known_paths(world, ctx, entry, n):
    """bmv_annotate, bmv_clip, bmv_realign and bmv_leftalign on the oracle's CIGARs.  Stale: an_begin, an_cigar and
    an_cigar_offset (the inputs all four share), emit.nm / pos / ref_len / n_xcigar / n_ref (an empty CIGAR writes zeros in the
    count pass: the two prefix sums read every element), emit.xcigar_offset, emit.ref_offset and scan_tmp (2 100 is two tiles
    with a carry), cl_l / cl_r / cl_score / cl_left / cl_right / cl_pos0 (no = column: the empty range), ra_pass, ra_row_at,
    ra_ops_at, ra_nops, ra_begin, ra_score, ra_end_lane, ra_codes (a pass-through writes its given path, score and begin, and no
    codes), la_slot_at, la_stack, la_nops, la_begin, la_changed, la_dropped, la_merges, la_compared (an unchanged or empty
    alignment writes zeros)."""
    _assert_small_paths(world, n)
    _five(world.genome, ctx, world.path_calls(entry, n), fresh=entry != "realign")
    if entry == "realign":                                     # (big on a fresh context is where its arrays come from)
        for step in ("small", "empty"):
            _fresh_agrees(world.genome, world.path_calls(entry, n)[step])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("order", [("annotate", "clip", "realign", "leftalign"), ("leftalign", "realign", "clip", "annotate")],
                         ids=["annotate first", "leftalign first"])
def test_the_passes_back_to_back(world, ctx, order, n):
    """The four passes share an_begin, an_cigar, an_cigar_offset and (annotate and clip) emit: big through the first, then small
    through the other three, in both orders; every result accessor keeps what its own call left."""
    _assert_small_paths(world, n)
    state = {}
    for k, entry in enumerate(order):
        call = world.path_calls(entry, n)["small" if k else "big"]
        _make(ctx, call, state, f"step {k}, {call.what}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("entry", ["split", "split_pick"])
def test_split(world, ctx, entry, n):
    """bmv_split and bmv_split_pick.  Stale: sp_score / sp_q_lo / sp_q_hi / sp_g_lo / sp_g_hi (an empty CIGAR and an alignment
    without an = column write their zeros over big's ranges), sp_group_offset, sp_contig -- small passes contig = NULL after a
    call that passed contigs --, sp_n_seg, sp_seg and sp_s2: big fills 16 slots a group, small has 1 and then 3 slots a group, so
    group g's slots begin where another group's lay, and a group that leaves early -- no members, or nobody at min_score -- must
    still write n_seg = 0 and BMV_BEYOND / BMV_SPLIT_NONE over every one of its slots; text_rc, which bmv_split_pick puts into
    the views' buffer.  Big: 2 100 alignments under scores that keep a part of each, in groups of 1, 63, 64, 65 and 130."""
    from bucket_map_amd import verify
    calls, pick = world.split_calls(entry, n)
    sizes = np.diff(_sized_groups(BIG, SPLIT_SIZES).astype(np.int64))
    assert set(SPLIT_SIZES) <= set(sizes.tolist()) and pick["n_seg"].max() >= 4 and (pick["n_seg"][sizes >= 63] >= 2).sum() > 15
    assert (pick["s2"][:, 0] != verify.SPLIT_NONE).sum() > 10 and 0 < (world.big_paths()[0][1] >= 30_000).sum() < BIG
    for ms in (1, 3):                                          # what the small batches claim to hold, on the restatement's output
        _, small = world.split_small(entry, n, ms)
        cigars, off = world.small_paths(n)[2], _sized_groups(n, (0, 2, 2))
        early = [g for g in range(len(off) - 1) if g % 3 < 2 and off[g + 1] <= (2 * n) // 3 + (n == 3)]
        assert len(early) >= 2 and any(off[g] == off[g + 1] for g in early) and any(cigars[a] == [] for g in early for a in range(off[g], off[g + 1]))
        assert not small["n_seg"][early].any() and (small["seg"][early] == BEYOND).all() and (small["s2"][early] == verify.SPLIT_NONE).all()
        assert small["seg"].shape[1] == ms and (n == 3 or small["n_seg"].any())
    state = {}
    for k, call in enumerate(calls):
        _make(ctx, call, state, f"step {k}, {call.what}")
    for call in calls[:4]:
        _fresh_agrees(world.genome, call)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
def test_frag_spans(world, ctx, n):
    """bmv_frag_spans.  Stale: bs_edits, bs_out_end and bs_group_offset (shared with bmv_align_best and bmv_pair), pr_contig --
    small passes contig = NULL after a call that passed contigs --, fr_span (a pair with an empty group, an unsettled one and
    one beyond cap write their 0) and fr_hist: big counts under cap = 65 535 by global atomics, small under cap = 100 in LDS,
    then big again, and the bins are the call's own every time -- hist sums to n_groups / 2 (World.frag_want asserts it of the
    restatement, which the call must equal).  Big: what bmv_align_best's oracle leaves for its 2 100 alignments."""
    big = world.big_groups()
    _, edits, out_end, _ = world.best_want(big)
    b = big["batch"]
    arrays, off = world.frag_small(n)
    calls = {"big": world.frag_call((b[1], b[2], b[3], b[5], edits, out_end), big["off"], 65_535, big["contig"], f"frag_spans of {BIG}"),
             "small": world.frag_call(arrays, off, 100, None, f"frag_spans of {n}"),
             "empty": world.frag_call(tuple(x[:0] for x in arrays), np.zeros(1, np.uint32), 100, None, "frag_spans of 0")}
    span = calls["big"].want["frag"][0]
    assert (span != 0).sum() > 50 and (span == 0).sum() > 50 and len(set(span.tolist())) > 40
    span, sizes = calls["small"].want["frag"][0], np.diff(off.astype(np.int64))
    assert (sizes == 0).any() and (span != 0).any() and span.max() <= 100 and (span == 0).sum() >= (1 if n == 3 else 3 * (len(span) // 4))
    _five(world.genome, ctx, calls)


@pytest.mark.gpu
@pytest.mark.parametrize("ctx", [None, 1], indirect=True, ids=["scratch by default", "1 MB of scratch"])
@pytest.mark.parametrize("n", SMALL)
def test_paired_begin_and_finish(world, ctx, n, request):
    """bmv_paired_begin with cap > 0, then bmv_paired_finish: every step is bmv_align_paired's oracle in that call's six rows
    -- and bmv_align_paired itself with the same range on a fresh context is held to the same arrays --, and the spans of what
    bmv_best returns in bmv_frag's two.  Stale: everything test_align_paired and test_frag_spans name, between the two halves
    too.  Big under cap = 65 535, small and empty under cap = 1 000; a sixth step makes the small batch's halves with cap = 0,
    which is bmv_align_paired and must leave bmv_frag and its stats as the big batch before it left them."""
    scratch_mb = request.node.callspec.params["ctx"]
    big, small, none = world.big_groups(), world.small_groups(n), world.no_groups()
    calls = {"big": world.halves_call(big, "wrong", 65_535, 200, 700, f"the halves of {BIG}"),
             "small": world.halves_call(small, "right", 1_000, 200, 700, f"the halves of {n}"),
             "empty": world.halves_call(none, "right", 1_000, 200, 700, "the halves of 0")}
    assert (calls["big"].want["frag"][0] != 0).sum() > 50 and not calls["small"].want["frag"][0].any()
    state = {}
    for k, step in enumerate(STEPS):
        call = world.halves_call(big, "right", 65_535, 200, 700, f"the halves of {BIG}, right hints") if k == 4 else calls[step]
        _make(ctx, call, state, f"step {k}, {call.what}")
    held = [x.copy() for x in state["frag"]]
    call = world.halves_call(small, "right", 0, 200, 700, f"the halves of {n}, cap 0")
    assert call.entry == "align_paired" and "frag" not in call.want
    _make(ctx, call, state, f"step 5, {call.what}")
    _assert_arrays(_read(ctx, "frag", held), held, "bmv_frag after the halves with cap 0")
    for step in ("big", "small", "empty"):
        _fresh_agrees(world.genome, calls[step], scratch_mb)
    for gb, hint, what in ((big, "wrong", BIG), (small, "right", n), (none, "right", 0)):
        _fresh_agrees(world.genome, world.paired_call(gb, hint, 200, 700, f"align_paired of {what}")[0], scratch_mb)


# ------------------------------------------------------------------------------------------------ between the two halves

BETWEEN = ("frag_spans", "pair", "frag", "annotate", "clip", "realign", "leftalign", "split", "split_pick", "rescue", "accessors")
ENDING = ("align", "align_long", "align_bounded", "align_best", "align_paired", "a refused paired_begin", "rescue beyond 512 bases")
RANGE = (200, 700)


def _halves_batches(world):
    """A: the first 70 groups of the big groups, with contigs.  B, by numbers alone: every alignment of the big groups but the
    first and the last group's -- 2 000 and more, and group g of B is group g + 1 of big, so hardly an offset of B is A's.  That the
    test cannot pass by accident is asserted here, on the CPU: were bmv_paired_finish to pick over what B's call left in
    bs_edits / bs_out_end under A's offsets, or over A's (edits, end) under what B's call left in bs_group_offset, it would
    pick otherwise for some pair of A."""
    def make():
        from bucket_map_amd import verify
        big = world.big_groups()
        a_gb = _first_groups(world, int(big["off"][70]))
        assert len(a_gb["off"]) == 71
        _, a_ed, a_en, _ = world.best_want(a_gb)
        _, ed, en, _ = world.best_want(big)
        off, bt = big["off"].astype(np.int64), big["batch"]
        lo, hi = int(off[1]), int(off[-2])
        b_off = (off[1:-1] - off[1]).astype(np.uint32)
        b = {"arrays": tuple(x[lo:hi] for x in (bt[1], bt[2], bt[3], bt[5], ed, en)), "off": b_off, "contig": big["contig"][lo:hi]}
        assert (len(b_off) - 1) % 2 == 0 and hi - lo > 4 * len(a_ed) and (b_off[1:71] != a_gb["off"][1:]).sum() >= 60
        at = a_gb["batch"]
        views, n_a = (at[1], at[2], at[3], at[5]), len(a_ed)
        true = verify.select_pairs(*views, a_ed, a_en, a_gb["off"], *RANGE, a_gb["contig"])["pick"]
        stale_edits = verify.select_pairs(*views, b["arrays"][4][:n_a], b["arrays"][5][:n_a], a_gb["off"], *RANGE, a_gb["contig"])["pick"]
        size = int(b_off[70])                                    # what 70 groups under B's offsets reach of A's arrays (beyond them: nothing known)
        fit = lambda x, fill: np.concatenate([x, np.full(max(size - n_a, 0), fill, x.dtype)])[:size]      # noqa: E731
        stale_offsets = verify.select_pairs(*(fit(x, 0) for x in views), fit(a_ed, BEYOND), fit(a_en, 0), b_off[:71], *RANGE,
                                            fit(a_gb["contig"], 0))["pick"]
        assert (stale_edits != true).any() and (stale_offsets != true).any(), "A and B would not tell a stale buffer from a fresh one"
        return a_gb, b
    return world.once("the halves' batches", make)


def _read_everything(v):
    """every accessor and every stats call, whatever they hold"""
    for name in ACCESSORS:
        _read(v, name, [np.zeros(0, t) for t in SHAPES[name]])
    for name in STATS:
        _counts(v, name)


def _begin(world, v, state):
    """bmv_paired_begin on A with cap = 1 000, which fills bmv_frag's row; returns A's groups, B and what finish must leave"""
    a_gb, b = _halves_batches(world)
    want = world.halves_call(a_gb, "right", 1_000, *RANGE, "the halves of A")
    frag = v.paired_begin(*a_gb["batch"], a_gb["off"], a_gb["margin"], 1_000, a_gb["right"], a_gb["contig"])
    _assert_arrays([frag["span"], frag["hist"]], want.want["frag"], "bmv_paired_begin's spans")
    state["frag"], state["frag_stats"] = want.want["frag"], _counts(v, "frag_stats")
    assert state["frag_stats"] == want.counts["frag_stats"]
    paired = world.paired_call(a_gb, "right", *RANGE, "align_paired of A")[0]
    return a_gb, b, paired


@pytest.mark.gpu
@pytest.mark.parametrize("between", BETWEEN)
def test_calls_that_may_come_between_the_halves(world, ctx, between):
    """bmv_paired_begin keeps (edits, end) and the group offsets of its batch A on the device for bmv_paired_finish -- the one
    state of the library that outlives a call there.  One call on a larger batch B with other group offsets comes in between;
    the finish then leaves, row for row, what bmv_align_paired leaves for A under the same range on a fresh context (the
    oracle's arrays for both).  bmv_pair and bmv_frag_spans put B's arrays where A's lay; the passes, the split calls and a
    rescue of queries of at most 512 bases use the views' buffers and their own; the accessors use none.  The in-between call
    is held to its own oracle too, and after the finish its row is still what it left."""
    state = {}
    a_gb, b, paired = _begin(world, ctx, state)
    if between == "frag_spans":
        call = world.frag_call(b["arrays"], b["off"], 65_535, b["contig"], "frag_spans of B")
    elif between == "pair":
        call = world.pair_call(b["arrays"], b["off"], 1, 5_000, b["contig"], "pair of B")[0]
    elif between in ("frag", "accessors"):
        call = None
    else:
        call = _any_call(world, between, BIG)
    if call is not None:
        if between == "rescue":
            assert call.want["rescued"][1].max() > 0 and max(world.rescue_big()[9]) <= 512
        _make(ctx, call, state, f"between the halves: {call.what}")
    elif between == "frag":
        got = ctx.frag(35, 1_000)
        _assert_arrays([got["span"], got["hist"]], state["frag"], "bmv_frag between the halves")
        ctx.frag_stats()
    else:
        _read_everything(ctx)
    finish = Call("align_paired", f"bmv_paired_finish of A after {between}", lambda v: v.paired_finish(*RANGE), paired.want, paired.counts)
    _make(ctx, finish, state, finish.what)
    world.once("A on a fresh context", lambda: _fresh_agrees(world.genome, paired))


@pytest.mark.gpu
@pytest.mark.parametrize("ending", ENDING)
def test_calls_that_end_a_pending_begin(world, ctx, ending):
    """Every call that aligns ends a pending bmv_paired_begin -- bmv_rescue too, when a query beyond 512 bases sends it to the
    aligner, and a new begin that its checks refuse: bmv_paired_finish then says BMV_ERR_STATE and changes nothing, and the
    context serves bmv_align_paired of the same batch as a fresh one would."""
    from bucket_map_amd import verify
    state = {}
    a_gb, b, paired = _begin(world, ctx, state)
    if ending == "a refused paired_begin":
        with pytest.raises(verify.BmvError) as e:
            ctx.paired_begin(*a_gb["batch"], a_gb["off"], a_gb["margin"], 65_536, a_gb["right"], a_gb["contig"])
        assert e.value.code == 1 and "cap" in str(e.value)
    else:
        if ending == "rescue beyond 512 bases":
            small = world.rescue_small(3)
            assert (small[9] > 512).any()
            call = world.rescue_call(small, 1, 5000, "rescue of 3 kinds that leave early")
        else:
            call = _any_call(world, ending, 3 if ending == "align_paired" else 70)
        _make(ctx, call, state, f"after the begin: {call.what}")
    refused = Call("align_paired", f"bmv_paired_finish after {ending}", lambda v: v.paired_finish(*RANGE), refused=3)
    _make(ctx, refused, state, refused.what)
    _make(ctx, paired, state, f"{paired.what} after {ending}")


# ------------------------------------------------------------------------------------------------ "leaves untouched"

def _prefix_groups(off, n):
    """the groups of the first n alignments (the last one cut), an empty one appended where their number is odd"""
    off = [int(x) for x in off if x <= n]
    if off[-1] != n:
        off.append(n)
    if len(off) % 2 == 0:
        off.append(n)
    return np.array(off, np.uint32)


def _first_groups(world, n):
    """the first n alignments of the big groups, in big's groups and with its margins, hints and contigs"""
    big, idx = world.big_groups(), np.arange(n)
    off = _prefix_groups(big["off"], n)
    g = len(off) - 1
    hint = np.minimum(np.resize(big["right"], g), np.maximum(np.diff(off.astype(np.int64)), 1) - 1).astype(np.uint32)
    return {"batch": _sub(big["batch"], idx), "off": off, "margin": np.resize(big["margin"], g).astype(np.uint32), "full": _take(big["full"], idx),
            "contig": big["contig"][:n], "right": hint}


def _any_call(world, entry, n):
    """`entry` on the first n items of its big batch, with the oracle's results for them"""
    idx = np.arange(n)
    if entry in ("align", "align_long"):
        batch, full = world.big_reads()
        return world.align_call(entry, _sub(batch, idx), _take(full, idx), f"{entry} of {n}")
    if entry == "align_bounded":
        world.bounded_calls(3)
        batch, full = world.memo["bounded big"]
        return world.bounded_call(_sub(batch, idx), _take(full, idx), (8 + idx % 9).astype(np.uint32), f"align_bounded of {n}")[0]
    if entry in ("align_best", "align_paired", "pair", "frag_spans", "paired_halves", "the halves with cap 0"):
        gb = _first_groups(world, n)
        if entry == "align_best":
            return world.best_call(gb, "right", f"align_best of {n}")
        if entry == "align_paired":
            return world.paired_call(gb, "right", 200, 700, f"align_paired of {n}")[0]
        if entry == "paired_halves":                           # (the largest cap only where the batch is large: 65 536 bins to check)
            return world.halves_call(gb, "right", 65_535 if n == BIG else 1_000, 200, 700, f"the halves of {n}")
        if entry == "the halves with cap 0":
            return world.halves_call(gb, "right", 0, 200, 700, f"the halves of {n}, cap 0")
        _, edits, out_end, _ = world.best_want(gb)
        b, off = gb["batch"], gb["off"]
        if entry == "frag_spans":
            return world.frag_call((b[1], b[2], b[3], b[5], edits, out_end), off, 65_535 if n == BIG else 100, gb["contig"], f"frag_spans of {n}")
        return world.pair_call((b[1], b[2], b[3], b[5], edits, out_end), off, 200, 700, gb["contig"], f"pair of {n}")[0]
    if entry in ("split", "split_pick"):                       # (fewer slots a group where the batch is cut)
        return world.split_first(entry, n, None if n == BIG else (SPLIT_BIG[1][0], SPLIT_BIG[1][1], (1, 3, 8)[n % 3]))[0]
    if entry == "rescue":
        args = world.rescue_big()
        return world.rescue_call((args[0], *(x[:n] for x in args[1:])), 1, 600, f"rescue of {n}")
    batch, begins, cigars = world.big_paths()
    if entry == "realign" and n == BIG:
        return world.path_calls("realign", 3)["big"]
    return world.path_call(entry, ("first", n), (_sub(batch, idx), begins[:n], cigars[:n]), f"{entry} of {n}")


def _new_refusal(world, rng):
    """... of the entries beyond ELEVEN: max_segments beyond 16, q_lo behind q_hi, a cap beyond 65 535 -- of bmv_frag_spans, and
    of bmv_paired_begin, which is then no begin at all: no finish follows"""
    batch, begins, cigars = world.big_paths()
    three, off3 = _sub(batch, np.arange(3)), np.array([0, 1, 3], np.uint32)
    which = int(rng.integers(0, 4))
    if which == 0:
        c_off, cg = _packed(cigars[:3])
        return Call("split", "split with 17 segments a group", lambda v: v.split(*three, begins[:3], c_off, cg, off3, max_segments=17), refused=1)
    if which == 1:
        return Call("split_pick", "split_pick with q_lo behind q_hi",
                    lambda v: v.split_pick([50, 60, 70], [0, 9, 0], [10, 8, 10], [0, 0, 0], [10, 10, 10], [0, 1, 0], off3), refused=1)
    big = world.big_groups()
    b = _sub(big["batch"], np.arange(3))
    if which == 2:
        return Call("frag_spans", "frag_spans with a cap beyond 65 535",
                    lambda v: v.frag_spans(b[1], b[2], b[3], b[5], np.zeros(3, np.uint32), b[5], off3, 65_536), refused=1)
    return Call("paired_halves", "paired_begin with a cap beyond 65 535", lambda v: v.paired_begin(*b, off3, np.ones(2, np.uint32), 65_536), refused=1)


def _refusal(world, rng, kinds=5):
    """a call that is refused before anything runs: it owns nothing"""
    g = world.genome
    batch, _ = world.big_reads()
    three = _sub(batch, np.arange(3))
    kind = int(rng.integers(0, kinds))
    if kind == 5:
        return _new_refusal(world, rng)
    if kind == 0:                                              # a text outside the genome, through any call that takes views
        outside = (three[0], np.array([0, len(g) - 100, 0], np.uint64), *three[2:])
        entry = ("align", "align_long", "align_bounded", "align_best", "annotate", "clip")[int(rng.integers(0, 6))]
        run = {"align": lambda v: v.align(*outside), "align_long": lambda v: v.align_long(*outside),
               "align_bounded": lambda v: v.align_bounded(*outside, np.full(3, 9, np.uint32)),
               "align_best": lambda v: v.align_best(*outside, np.array([0, 3], np.uint32), np.array([2], np.uint32)),
               "annotate": lambda v: v.annotate(*outside, np.zeros(3, np.uint32), np.zeros(4, np.uint64), np.zeros(0, np.uint32)),
               "clip": lambda v: v.clip(*outside, np.zeros(3, np.uint32), np.zeros(4, np.uint64), np.zeros(0, np.uint32))}[entry]
        return Call(entry, f"{entry} with a text outside the genome", run, refused=1)
    big = world.big_groups()
    b, odd = _sub(big["batch"], np.arange(3)), np.array([0, 1, 2, 3], np.uint32)
    if kind == 1:                                              # an odd n_groups
        if rng.integers(0, 2):
            return Call("align_paired", "align_paired with an odd n_groups",
                        lambda v: v.align_paired(*b, odd, np.ones(3, np.uint32), 200, 700), refused=1)
        return Call("pair", "pair with an odd n_groups", lambda v: v.pair(b[1], b[2], b[3], b[5], np.zeros(3, np.uint32), b[5], odd, 200, 700), refused=1)
    even = np.array([0, 1, 3], np.uint32)
    if kind == 2:                                              # min_frag > max_frag
        which = int(rng.integers(0, 3))
        if which == 0:
            return Call("pair", "pair with min_frag > max_frag",
                        lambda v: v.pair(b[1], b[2], b[3], b[5], np.zeros(3, np.uint32), b[5], even, 701, 700), refused=1)
        if which == 1:
            return Call("align_paired", "align_paired with min_frag > max_frag",
                        lambda v: v.align_paired(*b, even, np.ones(2, np.uint32), 701, 700), refused=1)
        args = world.rescue_big()
        return Call("rescue", "rescue with min_frag > max_frag", lambda v: v.rescue(args[0], *(x[:3] for x in args[1:]), 601, 600), refused=1)
    # a trace beyond 1 MB of scratch: 8 000 bases against 8 200 lie beyond the context's limits and take the long path, whose
    # checkpoints alone are 1.3 MB; 20 000 rows of direction codes are 1.3 MB
    if kind == 3:
        long = (g[10_000:18_000], np.array([9_900], np.uint64), np.array([8_200], np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.uint64),
                np.array([8_000], np.uint32))
        which = int(rng.integers(0, 3))
        if which == 0:
            return Call("align_long", "align_long with a trace beyond the scratch", lambda v: v.align_long(*long), refused=5)
        if which == 1:                                         # (refused in the survivors' sub-batch: the call's own row is unspecified)
            return Call("align_bounded", "align_bounded with a trace beyond the scratch",
                        lambda v: v.align_bounded(*long, np.array([100], np.uint32)), refused=5, spoils=True)
        return Call("align_best", "align_best with a trace beyond the scratch",
                    lambda v: v.align_best(*long, np.array([0, 1], np.uint32), np.array([9], np.uint32)), refused=5, spoils=True)
    rows = (g[10_000:30_000], np.array([10_000], np.uint64), np.array([20_000], np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.uint64),
            np.array([20_000], np.uint32))
    return Call("realign", "realign with direction codes beyond the scratch",
                lambda v: v.realign(*rows, np.zeros(1, np.uint32), np.array([0, 1], np.uint64), np.array([20_000 << 4], np.uint32)), refused=5)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,sizes,table", [(1, (0, 1, 3, 70, BIG), ELEVEN), (2, (0, 1, 3, 70, BIG), ELEVEN), (3, (0, 1, 3, 70, BIG), ELEVEN),
                                               (4, (BIG,), ELEVEN), (5, (0, 1, 3, 70, BIG), None), (6, (0, 1, 3, 70, BIG), None), (7, (BIG,), None)],
                         ids=["seed 1", "seed 2", "seed 3", "seed 4, every n 2100", "seed 5, every entry", "seed 6, every entry",
                              "seed 7, every entry, every n 2100"])
def test_every_call_leaves_the_others_results_untouched(world, seed, sizes, table):
    """40 calls drawn over eleven entry points (seeds 1 .. 4: the table as it stood when they were drawn), or 55 over every key
    of OWNS and the two halves with cap = 0, which are bmv_align_paired (seeds 5 .. 7); one in five a refusal (a text outside the
    genome, an odd n_groups,
    min_frag > max_frag, a trace beyond the scratch -- which bmv_align_long refuses before anything runs, and bmv_align_bounded and
    bmv_align_best after they handed a sub-batch on: their own row is then unspecified, every other one stays --; from seed 5 on
    also what bmv_split, bmv_split_pick, bmv_frag_spans and bmv_paired_begin refuse), on a context
    of 4 096-base limits and 1 MB of scratch.  After every call
    each of bmv_results, bmv_best, bmv_pairs, bmv_frag, bmv_rescued, bmv_segments, bmv_annotations, bmv_clipped, bmv_realigned and
    bmv_leftaligned, and
    the count fields of every bmv_last_*_stats, is what its own last successful call left: the oracle's for the owner (OWNS),
    unchanged for everybody else.  With every n 2 100 no buffer is ever reallocated."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(seed)
    entries = sorted(table or (*OWNS, "the halves with cap 0"))
    calls, kinds = (40, 5) if table else (55, 6)
    old = os.environ.get("BMV_SCRATCH_MB")
    os.environ["BMV_SCRATCH_MB"] = "1"
    try:
        v = verify.Verifier(4096, 4400)
    finally:
        if old is None:
            del os.environ["BMV_SCRATCH_MB"]
        else:
            os.environ["BMV_SCRATCH_MB"] = old
    v.load_genome(world.genome)
    state, seen, first, refused = {}, set(), [entries[x] for x in rng.permutation(len(entries))], 0     # every entry point once, then any
    try:
        for k in range(calls):
            if k % 5 == 4:
                call = _refusal(world, rng, kinds)
                refused += 1
            else:
                entry = first.pop() if first else entries[int(rng.integers(0, len(entries)))]
                call = _any_call(world, entry, int(sizes[int(rng.integers(0, len(sizes)))]))
            _make(v, call, state, f"seed {seed}, call {k}, {call.what}")
            seen |= set(state)
    finally:
        v.close()
    assert refused == calls // 5 and seen == {row for entry in (table or OWNS) for row in OWNS[entry]}
    assert table or seen == set(ACCESSORS) | set(STATS)
