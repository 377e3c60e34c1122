"""Best alignment per group on the GPU (bmv_align_best, include/bmv.h): the winner of every group, the distances and end
columns within the margin, and the winners' full alignments -- all against Verifier.align_long on the WHOLE batch plus the
plain-numpy contract verify.select_best, exactly, and whatever the hint."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
BASES = np.frombuffer(b"ACGT", np.uint8)


def _revcomp(a):
    return np.frombuffer(bytes(bytearray(a)).translate(COMP)[::-1], np.uint8)


def _mutate(rng, seq, sub, ins, dele):
    seq = np.asarray(seq, np.uint8)
    r = rng.random(len(seq))
    keep = r >= dele
    insert = (r >= dele) & (r < dele + ins)
    out = np.where(rng.random(len(seq)) < sub, BASES[rng.integers(0, 4, len(seq))], seq)
    ins_b = BASES[rng.integers(0, 4, len(seq))]
    pair = np.stack([np.where(insert, ins_b, 0), np.where(keep, out, 0)], 1).ravel()
    return pair[pair != 0].astype(np.uint8)


def _few_edits(rng, src, m, e):
    """A read of m bases out of src (longer than m) with at most e edit operations, out of the first m + 3 bases of src."""
    s, net = list(src), 0                                    # net deletions: at most 3, so that the read's source spans <= m + 3
    for _ in range(e):
        at = int(rng.integers(0, m - 1))
        kind = int(rng.integers(0, 3))
        if kind == 1:
            s.insert(at, int(BASES[rng.integers(0, 4)]))
            net -= 1
        elif kind == 2 and net < 3:
            del s[at]
            net += 1
        else:
            s[at] = int(BASES[rng.integers(0, 4)])
    return np.array(s[:m], np.uint8)


class _Groups:
    """A batch in groups: add() appends an alignment to the group begun by the last begin()."""

    def __init__(self):
        self.reads, self.at = [], 0
        self.ts, self.tl, self.trc, self.qs, self.ql, self.off, self.true_at = [], [], [], [], [], [0], []

    def begin(self, q):
        self.reads.append(np.asarray(q, np.uint8))
        self.q_at, self.q_len = self.at, len(q)
        self.at += len(q)

    def add(self, start, width, rc):
        self.ts.append(start); self.tl.append(width); self.trc.append(rc); self.qs.append(self.q_at); self.ql.append(self.q_len)

    def close(self, true_at=0):
        self.off.append(len(self.ts))
        self.true_at.append(true_at)

    def args(self):
        reads = np.concatenate(self.reads) if self.at else np.zeros(0, np.uint8)
        return (reads, np.array(self.ts, np.uint64), np.array(self.tl, np.uint32), np.array(self.trc, np.uint8),
                np.array(self.qs, np.uint64), np.array(self.ql, np.uint32))

    def offsets(self):
        return np.array(self.off, np.uint32)


def _reference(v, batch):
    """align_long on the whole batch: (score, begin, cigar_offset, cigar), d and end = begin + M and D lengths."""
    s, b, o, c = v.align_long(*batch)
    ref_cols = np.where((c & 15) != 1, c >> 4, 0).astype(np.int64)
    run = np.concatenate([[0], np.cumsum(ref_cols)])
    r_len = run[o[1:].astype(np.int64)] - run[o[:-1].astype(np.int64)]
    return (s, b, o, c), -s.astype(np.int64), b.astype(np.int64) + r_len


def _assert_best(got, ref, d, end, off, margin, what):
    from bucket_map_amd import verify
    s2, b2, o2, c2 = ref
    winner, edits, out_end = verify.select_best(d, end, off, margin)
    assert np.array_equal(got["winner"], winner), f"{what}: winners differ at groups {np.flatnonzero(got['winner'] != winner)[:10]}"
    bad = np.flatnonzero(got["edits"] != edits)
    assert bad.size == 0, f"{what}: edits differ at {bad[:10]}: got {got['edits'][bad[:10]]}, want {edits[bad[:10]]} (d {d[bad[:10]]})"
    bad = np.flatnonzero(got["end"] != out_end)
    assert bad.size == 0, f"{what}: ends differ at {bad[:10]}: got {got['end'][bad[:10]]}, want {out_end[bad[:10]]}"
    n = len(d)
    s, b, o, c = got["score"], got["begin"], got["cigar_offset"], got["cigar"]
    wins = np.zeros(n, bool)
    wins[winner[winner != verify.BEYOND]] = True
    lens = np.diff(o.astype(np.int64))
    assert o[0] == 0 and o[n] == len(c), f"{what}: total_cigar is not the sum of the winners' CIGARs"
    assert (s[~wins] == verify.REJECTED).all() and (b[~wins] == 0).all() and (lens[~wins] == 0).all(), \
        f"{what}: an alignment that did not win carries a result"
    assert np.array_equal(s[wins], s2[wins]) and np.array_equal(b[wins], b2[wins]), f"{what}: winners' scores or begins differ"
    assert np.array_equal(lens[wins], np.diff(o2.astype(np.int64))[wins]), f"{what}: winners' CIGAR lengths differ"
    for a in np.flatnonzero(wins):
        assert np.array_equal(c[o[a]: o[a + 1]], c2[o2[a]: o2[a + 1]]), f"{what}: CIGAR of winner {a} differs"
    return winner


def _hints(rng, g, off):
    """hint = None, the true locus, a wrong candidate, random."""
    size = np.diff(off.astype(np.int64))
    true_at = np.array(g.true_at, np.int64)
    some = np.maximum(size, 1)
    return (("none", None), ("true", (true_at % some).astype(np.uint32)), ("wrong", ((true_at + 1) % some).astype(np.uint32)),
            ("random", (rng.integers(0, 1 << 30, len(size)) % some).astype(np.uint32)))


LANE_LENGTHS = (1, 63, 64, 65, 128, 300, 511, 512)
WAVE_LENGTHS = (513, 700, 1500, 4096, 4097, 9000)
PAIRS, PAIR_LEN = 6, 11_000


@pytest.fixture(scope="module")
def sweep():
    """About 600 groups over a 200-kbp genome with planted copies (six pairs of 11 kbp, diverged by 0 .. 12 %), N bases in
    the genome and in reads, both strands, overlapping windows of one locus, group sizes 0 .. 6 and one group of 70; the
    reference is computed once."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(20250901)
    genome = rng.choice(list(b"ACGT"), 200_000).astype(np.uint8)
    pair_at = []
    for p, div in enumerate((0.0, 0.004, 0.01, 0.03, 0.06, 0.12)):
        s, t = 2_000 + p * 2 * (PAIR_LEN + 400), 2_000 + p * 2 * (PAIR_LEN + 400) + PAIR_LEN + 400
        copy = _mutate(rng, genome[s: s + PAIR_LEN], div * 0.8, div * 0.1, div * 0.1)[:PAIR_LEN]
        genome[t: t + len(copy)] = copy
        pair_at.append((s, t))
    genome[rng.integers(0, len(genome), 300)] = ord("N")
    g = _Groups()
    plan = [(m, 56) for m in LANE_LENGTHS] + [(m, 40) for m in WAVE_LENGTHS[:3]] + [(m, 12) for m in WAVE_LENGTHS[3:]]
    for m, count in plan:
        for i in range(count):
            size = int(rng.integers(0, 7))
            slack = m // 10 + 4
            width = m + 1 + slack
            in_pair = i % 2 == 0
            if in_pair:
                s, t = pair_at[int(rng.integers(0, PAIRS))]
                pos = s + int(rng.integers(slack, PAIR_LEN - m - slack))
            else:
                s = t = 0
                pos = int(rng.integers(140_000, len(genome) - width - slack))
            rc = int(rng.integers(0, 2))
            src = genome[pos: pos + m]
            q = _mutate(rng, _revcomp(src) if rc else src, 0.03, 0.01, 0.01)[:m]
            if len(q) < m:
                q = np.concatenate([q, rng.choice(list(b"ACGT"), m - len(q)).astype(np.uint8)])
            if i % 9 == 0:
                q[rng.integers(0, m, 1 + m // 100)] = ord("N")
            g.begin(q)
            lead = int(rng.integers(0, slack + 1))
            cands = [(pos - lead, width, rc)]                                     # the true locus
            kinds = rng.permutation(5)
            for kind in kinds[: max(size - 1, 0)]:
                if kind == 0:                                                      # the same locus through a shifted window
                    cands.append((pos - int(rng.integers(0, slack + 1)), width, rc))
                elif kind == 1 and in_pair:                                        # the planted copy
                    cands.append((t + (pos - s) - slack // 2, width, rc))
                elif kind == 2:                                                    # the other strand of the true window
                    cands.append((pos - lead, width, 1 - rc))
                else:                                                              # somewhere else
                    cands.append((int(rng.integers(0, len(genome) - width)), width, int(rng.integers(0, 2))))
            order = rng.permutation(len(cands)) if size else []
            for k in order:
                g.add(*cands[k])
            g.close(int(np.argmin(order)) if size else 0)
    # one group of 70 members: the wave-per-group pick
    m, slack = 300, 34
    pos = 150_000
    q = _mutate(rng, genome[pos: pos + m], 0.03, 0.01, 0.01)[:m]
    g.begin(q)
    for k in range(70):
        if k in (17, 40):
            g.add(pos - (k % slack), m + 1 + slack, 0)
        else:
            g.add(int(rng.integers(0, len(genome) - 400)), m + 1 + slack, int(rng.integers(0, 2)))
    g.close(17)
    v = verify.Verifier()
    v.load_genome(genome)
    batch, off = g.args(), g.offsets()
    ref, d, end = _reference(v, batch)
    return {"v": v, "g": g, "batch": batch, "off": off, "ref": ref, "d": d, "end": end, "rng": rng}


def _margins(kind, sw):
    off, d, ql = sw["off"].astype(np.int64), sw["d"], sw["batch"][5]
    n_groups = len(off) - 1
    if kind == "zero":
        return np.zeros(n_groups, np.uint32), None
    if kind == "huge":
        # at least the query length: everything is within the margin; every other group takes 2^32 - 1 (the 64-bit sum)
        mg = np.array([int(ql[off[g]]) if off[g + 1] > off[g] else 0 for g in range(n_groups)], np.uint32)
        mg[::2] = 2 ** 32 - 1
        return mg, None
    # from the reference's distances: the runner-up exactly at the margin (even groups), exactly one past it (odd groups)
    mg, at, past = np.zeros(n_groups, np.uint32), 0, 0
    for g in range(n_groups):
        dg = np.sort(d[off[g]: off[g + 1]])
        if len(dg) < 2:
            continue
        gap = int(dg[1] - dg[0])
        if g % 2 == 0 or gap == 0:
            mg[g] = gap
            at += 1
        else:
            mg[g] = gap - 1
            past += 1
    return mg, (at, past)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["runner_up", "zero", "huge"])
def test_sweep_is_exact_whatever_the_hint(sweep, kind):
    sw = sweep
    v, batch, off = sw["v"], sw["batch"], sw["off"]
    margin, occur = _margins(kind, sw)
    if occur is not None:
        assert occur[0] > 50 and occur[1] > 50, f"runner-up at the margin in {occur[0]} groups, one past it in {occur[1]}"
    sizes = np.diff(off.astype(np.int64))
    assert (sizes == 0).any() and (sizes == 70).any() and set(range(7)) <= set(sizes.tolist())
    first = None
    for name, hint in _hints(np.random.default_rng(5), sw["g"], off):
        got = v.align_best(*batch, off, margin, hint)
        _assert_best(got, sw["ref"], sw["d"], sw["end"], off, margin, f"margin {kind}, hint {name}")
        st = v.best_stats()
        print(f"margin {kind}, hint {name}: {st}")
        assert st["n_seed"] == int((sizes > 0).sum())
        if first is None:
            first = got
        for key in first:
            assert np.array_equal(first[key], got[key]), f"margin {kind}: {key} depends on the hint ({name})"


@pytest.mark.gpu
def test_ties_go_to_the_lowest_index():
    """The same window twice in a group, and a true duplicate at another coordinate."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(77)
    genome = rng.choice(list(b"ACGT"), 60_000).astype(np.uint8)
    g = _Groups()
    for m in (40, 300, 512, 700, 5000):
        pos, dup = 1_000, 30_000
        genome[dup: dup + m + 40] = genome[pos: pos + m + 40]                      # a true duplicate
        q = _mutate(rng, genome[pos + 7: pos + 7 + m], 0.02, 0.005, 0.005)[:m]
        width = m + 30
        for order in ([0, 0, 1], [1, 0, 0], [2, 1, 0, 0, 1]):
            g.begin(q)
            for k in order:
                g.add((pos, dup, 45_000)[k], width, 0)
            g.close(0)
    batch, off = g.args(), g.offsets()
    v = verify.Verifier()
    v.load_genome(genome)
    ref, d, end = _reference(v, batch)
    margin = np.full(len(off) - 1, 3, np.uint32)
    for name, hint in _hints(rng, g, off):
        got = v.align_best(*batch, off, margin, hint)
        winner = _assert_best(got, ref, d, end, off, margin, f"ties, hint {name}")
        # the duplicates tie, so the first of them wins
        for gi, w in enumerate(winner):
            a0, a1 = int(off[gi]), int(off[gi + 1])
            assert (d[a0:a1] == d[w]).sum() >= 2 and w == a0 + int(np.argmin(d[a0:a1]))
    v.close()


@pytest.mark.gpu
def test_a_query_beyond_the_limits_takes_the_long_path():
    from bucket_map_amd import verify
    rng = np.random.default_rng(78)
    genome = rng.choice(list(b"ACGT"), 200_000).astype(np.uint8)
    m = 70_000
    q = _mutate(rng, genome[10_000: 10_000 + m + 2000], 0.02, 0.01, 0.01)[:m]
    g = _Groups()
    g.begin(q)
    g.add(110_000, m + 3000, 0)
    g.add(9_000, m + 3000, 0)
    g.close(1)
    batch, off = g.args(), g.offsets()
    v = verify.Verifier()
    v.load_genome(genome)
    ref, d, end = _reference(v, batch)
    margin = np.array([100], np.uint32)
    for name, hint in _hints(rng, g, off):
        got = v.align_best(*batch, off, margin, hint)
        winner = _assert_best(got, ref, d, end, off, margin, f"70 000 bases, hint {name}")
        assert winner[0] == 1
        st = v.best_stats()
        assert st["n_seed"] == 1 and st["n_distance"] == 0 and st["n_realigned"] == 0, st   # not a case for the kernels
    v.close()


def _planted(rng, genome, n_groups, m, width, max_edits, decoys=3):
    g = _Groups()
    for _ in range(n_groups):
        pos = int(rng.integers(0, len(genome) - width - 40))
        q = _few_edits(rng, genome[pos + 3: pos + 3 + m + 20], m, int(rng.integers(0, max_edits + 1)))
        g.begin(q)
        g.add(pos, width, 0)
        for _ in range(decoys):
            g.add(int(rng.integers(0, len(genome) - width)), width, 0)
        g.close(0)
    return g


@pytest.mark.gpu
def test_what_the_feature_is_for_short_reads():
    """2 000 groups x 4 of (300 x 307), the hint is the true locus (<= 5 % edits), three uniform random decoys, margin 15: one
    full alignment per group, nothing realigned, nothing undecided (a lane holds every word of a <= 512-base query)."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(79)
    genome = rng.choice(list(b"ACGT"), 1_000_000).astype(np.uint8)
    g = _planted(rng, genome, 2000, 300, 307, 15)
    batch, off = g.args(), g.offsets()
    v = verify.Verifier()
    v.load_genome(genome)
    ref, d, end = _reference(v, batch)
    margin = np.full(2000, 15, np.uint32)
    hint = np.zeros(2000, np.uint32)
    got = v.align_best(*batch, off, margin, hint)
    winner = _assert_best(got, ref, d, end, off, margin, "2 000 x 4 of 300 x 307")
    # a decoy cannot beat the true locus: by the reference's distances, not by assumption
    assert np.array_equal(winner, off[:-1]) and (d[0::4] <= 15).all()
    st = v.best_stats()
    print(st, v.stats())
    assert st["n_seed"] == 2000 and st["n_distance"] == 6000 and st["n_realigned"] == 0 and st["n_undecided"] == 0, st
    assert 0 < st["distance_cells"] < 6000 * 320 * 307
    v.close()


@pytest.mark.gpu
def test_what_the_feature_is_for_long_reads():
    """The same shape with 200 groups x 4 of (5 000 x 5 501): correct against the reference (the wave kernels)."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(80)
    genome = rng.choice(list(b"ACGT"), 1_000_000).astype(np.uint8)
    g = _planted(rng, genome, 200, 5000, 5501, 250)
    batch, off = g.args(), g.offsets()
    v = verify.Verifier()
    v.load_genome(genome)
    ref, d, end = _reference(v, batch)
    margin = np.full(200, 250, np.uint32)
    got = v.align_best(*batch, off, margin, np.zeros(200, np.uint32))
    _assert_best(got, ref, d, end, off, margin, "200 x 4 of 5 000 x 5 501")
    st = v.best_stats()
    print(st, v.stats())
    assert st["n_seed"] == 200 and st["n_distance"] == 600
    v.close()


@pytest.mark.gpu
def test_refusals_leave_the_context_usable():
    from bucket_map_amd import verify
    rng = np.random.default_rng(81)
    genome = rng.choice(list(b"ACGT"), 50_000).astype(np.uint8)
    g = _planted(rng, genome, 20, 200, 230, 6, decoys=2)
    batch, off = g.args(), g.offsets()
    v = verify.Verifier()
    v.load_genome(genome)
    ref, d, end = _reference(v, batch)
    margin = np.full(20, 5, np.uint32)
    before = v.align_best(*batch, off, margin)
    bad_off = off.copy()
    bad_off[5], bad_off[6] = off[6], off[5]
    with pytest.raises(verify.BmvError) as e:
        v.align_best(*batch, bad_off, margin)
    assert e.value.code == 1 and "group 5" in str(e.value)
    short = off.copy()
    short[-1] -= 1
    with pytest.raises(verify.BmvError) as e:
        v.align_best(*batch, short, margin)
    assert e.value.code == 1
    hint = np.zeros(20, np.uint32)
    hint[7] = 3
    with pytest.raises(verify.BmvError) as e:
        v.align_best(*batch, off, margin, hint)
    assert e.value.code == 1 and "group 7" in str(e.value)
    after = v.align_best(*batch, off, margin, np.full(20, 2, np.uint32))
    _assert_best(after, ref, d, end, off, margin, "after the refusals")
    for key in before:
        assert np.array_equal(before[key], after[key])
    v.close()


def _small_batch(rng, genome, n, m=100, width=110):
    """n reads of m bases with a few substitutions, either strand, one window each."""
    reads, ts, rc = [], [], []
    for _ in range(n):
        start, r = int(rng.integers(0, len(genome) - width)), int(rng.integers(0, 2))
        src = genome[start + 1: start + 1 + m]
        reads.append(_mutate(rng, _revcomp(src) if r else src, 0.03, 0, 0))
        ts.append(start)
        rc.append(r)
    return (np.concatenate(reads), np.array(ts, np.uint64), np.full(n, width, np.uint32), np.array(rc, np.uint8),
            np.arange(n, dtype=np.uint64) * m, np.full(n, m, np.uint32))


def _flat(res):
    return list(res.values()) if isinstance(res, dict) else list(res)


@pytest.mark.gpu
def test_view_refusals_through_every_entry_point():
    """A query or a text that leaves its buffer is refused by all six calls that take a batch, with the alignment's index
    and the same words; the context then does a good batch as a fresh one does (and align as the oracle does)."""
    from bucket_map_amd import verify
    from oracle import oracle_c as oc
    rng = np.random.default_rng(82)
    genome = rng.choice(list(b"ACGT"), 2000).astype(np.uint8)
    good = _small_batch(rng, genome, 3)
    n_read_bytes, n_genome = len(good[0]), len(genome)
    s_ref, b_ref, o_ref, c_ref = oc.align_batch(genome, *good)
    off, margin, bound = np.array([0, 2, 3], np.uint32), np.array([5, 5], np.uint32), np.full(3, 10, np.uint32)
    calls = {
        "align": lambda v, b: v.align(*b),
        "align_long": lambda v, b: v.align_long(*b),
        "align_bounded": lambda v, b: v.align_bounded(*b, bound),
        "align_best": lambda v, b: v.align_best(*b, off, margin),
        "annotate": lambda v, b: v.annotate(*b, b_ref, o_ref, c_ref),
        "clip": lambda v, b: v.clip(*b, b_ref, o_ref, c_ref),
    }

    def with_(k, value):                                       # alignment 1's entry of array k replaced
        b = [x.copy() for x in good]
        b[k][1] = value
        return b

    bad = {
        "a query one byte past the read buffer": (with_(4, n_read_bytes + 1 - 100), "query lies outside the read buffer"),
        "query_start beyond the read buffer": (with_(4, n_read_bytes + 1), "query lies outside the read buffer"),
        "a text one base past the genome": (with_(1, n_genome - 110 + 1), "text lies outside the genome"),
        "text_start beyond the genome": (with_(1, n_genome + 1), "text lies outside the genome"),
    }
    v = verify.Verifier()
    v.load_genome(genome)
    for name, call in calls.items():
        for what, (batch, words) in bad.items():
            with pytest.raises(verify.BmvError) as e:
                call(v, batch)
            assert e.value.code == 1 and "alignment 1:" in str(e.value) and words in str(e.value), (name, what, str(e.value))
    got = v.align(*good)
    assert all(np.array_equal(x, y) for x, y in zip(got, (s_ref, b_ref, o_ref, c_ref))), "align after the refusals"
    fresh = verify.Verifier()
    fresh.load_genome(genome)
    for name, call in calls.items():
        assert all(np.array_equal(x, y) for x, y in zip(_flat(call(v, good)), _flat(call(fresh, good)))), name
    v.close()
    fresh.close()


@pytest.mark.gpu
def test_results_survive_other_calls_and_buffers_survive_size_changes():
    """One context: align (n = 3), annotate of those, clip of another batch (n = 70: a second block in the grids and the
    scans), align_best (n = 5 in two groups), annotate (n = 3) again.  After every call each of bmv_results, bmv_annotations,
    bmv_clipped and bmv_best returns what its own last call left -- which is what a fresh context leaves for that call (align:
    the oracle) -- and the last annotate equals the first."""
    import ctypes as C

    from bucket_map_amd import verify
    from oracle import oracle_c as oc
    rng = np.random.default_rng(83)
    genome = rng.choice(list(b"ACGT"), 20_000).astype(np.uint8)
    three, seventy, five = _small_batch(rng, genome, 3), _small_batch(rng, genome, 70, 300, 310), _small_batch(rng, genome, 5)
    five = (five[0], *five[1:4], np.array([0, 0, 0, 100, 100], np.uint64), five[5])            # two reads: 3 + 2 candidates
    off, margin = np.array([0, 3, 5], np.uint32), np.array([4, 4], np.uint32)
    r3, r70 = oc.align_batch(genome, *three), oc.align_batch(genome, *seventy)
    L = verify.lib()
    p = lambda x: x.ctypes.data_as(C.POINTER({"int32": C.c_int32, "uint32": C.c_uint32, "uint64": C.c_uint64, "int64": C.c_int64,
                                             "uint8": C.c_uint8}[x.dtype.name]))
    accessor = {"results": L.bmv_results, "annotations": L.bmv_annotations, "clipped": L.bmv_clipped, "best": L.bmv_best}
    last = {}                                                  # accessor -> the arrays its own last call should have left

    def fresh(call):
        w = verify.Verifier()
        w.load_genome(genome)
        out = call(w)
        w.close()
        return out

    def check(step):
        for name, want in last.items():
            got = [np.zeros(max(len(x), 1), x.dtype) for x in want]
            assert accessor[name](v._h, *(p(x) for x in got)) == 0
            assert all(np.array_equal(g[: len(x)], x) for g, x in zip(got, want)), f"after {step}: bmv_{name} changed"

    v = verify.Verifier()
    v.load_genome(genome)
    got = v.align(*three)
    assert all(np.array_equal(x, y) for x, y in zip(got, r3))
    last["results"] = list(r3)
    check("align")
    first = v.annotate(*three, *r3[1:])
    want = fresh(lambda w: w.annotate(*three, *r3[1:]))
    assert all(np.array_equal(x, y) for x, y in zip(first, want))
    last["annotations"] = list(want)
    check("annotate")
    got = v.clip(*seventy, *r70[1:])
    want = fresh(lambda w: w.clip(*seventy, *r70[1:]))
    assert all(np.array_equal(got[k], want[k]) for k in want)
    last["clipped"] = [want[k] for k in ("score", "clip_left", "clip_right", "nm", "pos", "ref_len", "xcigar_offset", "xcigar",
                                         "ref_offset", "ref_bases")]
    check("clip")
    got = v.align_best(*five, off, margin)
    want = fresh(lambda w: w.align_best(*five, off, margin))
    assert all(np.array_equal(got[k], want[k]) for k in want)
    last["results"] = [want[k] for k in ("score", "begin", "cigar_offset", "cigar")]
    last["best"] = [want[k] for k in ("winner", "edits", "end")]
    check("align_best")
    again = v.annotate(*three, *r3[1:])
    assert all(np.array_equal(x, y) for x, y in zip(again, first)), "the second annotate differs from the first"
    check("the second annotate")
    v.close()


GPU_TOOL = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
ORACLE_TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")


@pytest.fixture(scope="module")
def duplicated(tmp_path_factory):
    """The small duplicated genome of tests/test_best.py: a 30-kbp record, a second one with a copy of 12 kbp of it (half
    exact, half diverged by 1 %), 150 reads of 150 bases; and the oracle-backed tool's files for every option set."""
    d = tmp_path_factory.mktemp("best_gpu")
    rng = np.random.default_rng(5)

    def mutate(seq, rate):
        s = seq.copy()
        hit = rng.random(len(s)) < rate
        s[hit] = BASES[rng.integers(0, 4, int(hit.sum()))]
        return s
    a = BASES[rng.integers(0, 4, 30_000)]
    b = np.concatenate([BASES[rng.integers(0, 4, 3000)], a[5000:11000], mutate(a[11000:17000], 0.01), BASES[rng.integers(0, 4, 2000)]])
    with open(d / "g.fa", "w") as f:
        f.write(f">chrA\n{bytes(a).decode()}\n>chrB\n{bytes(b).decode()}\n")
    with open(d / "reads.fastq", "w") as f:
        for i in range(150):
            p = int(rng.integers(0, 30_000 - 160)) if i % 3 else int(rng.integers(5000, 16_800))
            s = bytes(mutate(a[p: p + 150], 0.02))
            if i % 2:
                s = s.translate(COMP)[::-1]
            f.write(f"@r{i}\n{s.decode()}\n+\n{'I' * 150}\n")
    return d


TOOL_ARGS = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "4096", "-r", "150", "-f", "1", "-q", "reads.fastq"]


def _tool(exe, d, out, *extra, dump=None):
    env = dict(os.environ, BM_VERIFY_BLOCK_READS="37")
    if dump:
        env["BM_DUMP_ALIGNMENTS"] = str(d / dump)
    r = subprocess.run([exe, *TOOL_ARGS, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return (d / out).read_bytes(), r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra", [("alone", []), ("annotate", ["--annotate"]), ("clip", ["--clip"]),
                                        ("bounded", ["--max-edit-rate", "0.1"])])
def test_tool_equals_the_oracle_backed_tool(duplicated, name, extra):
    """bucketmap_align --best writes, byte for byte, what the oracle-backed tool writes, whose verifier aligns every candidate
    and selects on the host; --gpus 0,0 writes the same bytes.  The oracle-backed verifier has no annotation or clipping
    pass, so with --annotate and --clip the file is held, byte for byte as well, against the records the tool writes
    WITHOUT --best: the winner's record of that run (winners by verify.select_best over its dump) with the helper's MAPQ
    and the X0 tag."""
    from test_best import expected_best_records
    d = duplicated
    gpu, err = _tool(GPU_TOOL, d, f"gpu_{name}.sam", "--best", *extra, dump=f"gpu_{name}.txt")
    assert "best per read" in err
    two, _ = _tool(GPU_TOOL, d, f"gpu2_{name}.sam", "--best", *extra, "--gpus", "0,0")
    assert two == gpu, "--gpus 0,0 differs from --gpus 0"
    recs = [l for l in gpu.decode().split("\n") if l and not l.startswith("@")]
    if name in ("annotate", "clip"):
        plain, _ = _tool(GPU_TOOL, d, f"all_{name}.sam", *extra, dump=f"all_{name}.txt")
        want, dump, sizes = expected_best_records(plain.decode(), open(d / f"all_{name}.txt").read(), 0.05)
        assert (sizes > 1).sum() >= 10
        assert recs == want
        assert open(d / f"gpu_{name}.txt").read().split("\n")[:-1] == dump
        assert all(l.split("\t")[-1].startswith("X0:i:") and l.split("\t")[11].startswith("NM:i:") for l in recs)
    else:
        cpu, _ = _tool(ORACLE_TOOL, d, f"cpu_{name}.sam", "--best", *extra)
        assert gpu == cpu
    assert len(recs) > 100 and any(l.split("\t")[4] == "0" for l in recs) and any(l.split("\t")[4] == "60" for l in recs)
