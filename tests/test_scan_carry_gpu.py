"""The device-wide prefix sum beyond 256 tiles (bm_scan.hip.h).

scan_sums_kernel scans the tile sums 256 at a time and carries the running total from one round of 256 into the next; a tile is
2 048 items, so the carry between rounds is live only beyond 256 x 2 048 = 524 288 items.  Every packed output of the verifier,
the filter and the BGZF gather goes through this scan, and no other test reaches its second round with counts that would show
a wrong carry.  Here n = 256 x 2 048 + 2 048 + 5: 258 tiles, the last one partial, the second round two tile sums long.  One
call per instance of the template, each held exactly against plain numpy / the CPU oracle in batch order."""
import time

import numpy as np
import pytest

from oracle import oracle_c as oc
from test_annotate import restate

N = 256 * 2048 + 2048 + 5
REJECTED = -(2 ** 31)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def _flat(first, second, count, off):
    """the packed array of items that own count[a] in {0, 1, 2} elements from off[a] on: first[a], then second[a]"""
    out = np.zeros(int(off[-1]), first.dtype)
    at = off[:-1].astype(np.int64)
    out[at[count >= 1]] = first[count >= 1]
    out[at[count == 2] + 1] = second[count == 2]
    return out


@pytest.mark.gpu
def test_scan_64_bit_offsets_beyond_256_tiles():
    """bmv_annotate (exclusive_sum<uint64_t>, twice: the =/X entries and the reference bases) on N alignments of 2-base queries
    of three kinds in a random order: `2=` on the reverse strand (1 entry, no base), `1=1X` forward (2 entries, 1 base) and an
    empty CIGAR (nothing).  The offsets are the numpy cumsum of those counts, the entries and bases each kind's restated once."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(20260301)
    genome = rng.choice(list(b"ACGT"), 64).astype(np.uint8)
    #        window            rc  begin  query (as sequenced)                                        cigar
    kinds = [(genome[10:14], 1, 1, COMP[genome[10:14][::-1]][1:3].copy(), [(0, 2)]),
             (genome[30:34], 0, 1, np.array([genome[31], COMP[genome[32]]], np.uint8), [(0, 2)]),
             (genome[50:54], 0, 0, genome[40:42].copy(), [])]
    want = [restate(bytes(w), rc, bytes(q), b, c) for w, rc, b, q, c in kinds]
    assert [x[2] for x in want] == [[(7, 2)], [(7, 1), (8, 1)], []] and [len(x[4]) for x in want] == [0, 1, 0]
    assert [x[0] for x in want] == [1, 1, 0] and [x[3] for x in want] == [0, 1, 0]

    kind = rng.integers(0, 3, N)
    kind[[0, 2047, 2048, 524287, 524288, N - 1]] = (1, 1, 0, 1, 1, 1)       # (something to carry across each border)
    per = lambda values, t: np.array(values, t)[kind]                                                     # noqa: E731
    reads = np.concatenate([k[3] for k in kinds])
    ts, tl = per([10, 30, 50], np.uint64), np.full(N, 4, np.uint32)
    trc, qs, ql = per([k[1] for k in kinds], np.uint8), per([0, 2, 4], np.uint64), np.full(N, 2, np.uint32)
    begin = per([k[2] for k in kinds], np.uint32)
    n_in = per([1, 1, 0], np.int64)
    cig_off = np.concatenate([[0], np.cumsum(n_in)]).astype(np.uint64)
    cigar = np.full(int(cig_off[-1]), (2 << 4) | 0, np.uint32)

    n_x, n_r = per([len(x[2]) for x in want], np.int64), per([len(x[4]) for x in want], np.int64)
    x_off, r_off = np.concatenate([[0], np.cumsum(n_x)]).astype(np.uint64), np.concatenate([[0], np.cumsum(n_r)]).astype(np.uint64)
    entry = lambda k: [((x[2][k][1] << 4) | x[2][k][0]) if len(x[2]) > k else 0 for x in want]           # noqa: E731
    x_want = _flat(per(entry(0), np.uint32), per(entry(1), np.uint32), n_x, x_off)
    r_want = _flat(per([(x[4] or b"\0")[0] for x in want], np.uint8), np.zeros(N, np.uint8), n_r, r_off)
    assert int(x_off[-1]) > N // 2 and int(x_off[524288]) != int(x_off[-1]) and len(set(np.diff(x_off[::2048].astype(np.int64)).tolist())) > 50

    v = verify.Verifier()
    v.load_genome(genome)
    t0 = time.perf_counter()
    nm, pos, ref_len, xo, xc, ro, rb = v.annotate(reads, ts, tl, trc, qs, ql, begin, cig_off, cigar)
    print(f"bmv_annotate of {N} alignments: {time.perf_counter() - t0:.2f} s")
    columns = v.annotate_stats()["columns"]
    v.close()
    for got, exp, what in ((xo, x_off, "xcigar_offset"), (ro, r_off, "ref_offset"), (xc, x_want, "xcigar"), (rb, r_want, "ref_bases"),
                           (nm, per([x[3] for x in want], np.uint32), "nm"), (pos, per([x[0] for x in want], np.uint32), "pos"),
                           (ref_len, per([x[1] for x in want], np.uint32), "ref_len")):
        assert len(got) == len(exp), f"{what}: {len(got)} elements, {len(exp)} expected"
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{what} differs from {bad[0]} on ({bad.size} elements): got {got[bad[:4]]}, want {exp[bad[:4]]}"
    assert columns == 2 * int(n_in.sum())


@pytest.mark.gpu
def test_scan_32_bit_offsets_beyond_256_tiles():
    """bmv_align_bounded (exclusive_sum<uint32_t>: the survivors' places, then the CIGAR offsets of the survivors' sub-batch) on
    N alignments of 8-base queries in 12-base windows under max_edits = 0, either strand: exact copies of their window's middle
    and random queries in an irregular order, so that about half survive the screen and every survivor's place depends on all
    before it.  Scores, begins and CIGARs against the CPU oracle in batch order."""
    from bucket_map_amd import verify
    from test_verifier_reuse_gpu import _keep_only
    rng = np.random.default_rng(20260302)
    genome = rng.choice(list(b"ACGT"), 100_000).astype(np.uint8)
    ts = rng.integers(0, len(genome) - 12, N).astype(np.uint64)
    trc = rng.integers(0, 2, N).astype(np.uint8)
    window = genome[ts.astype(np.int64)[:, None] + np.arange(12)[None, :]]
    seen = np.where(trc[:, None] != 0, COMP[window[:, ::-1]], window)           # the text as the aligner sees it
    exact = rng.random(N) < 0.5
    exact[[0, 2047, 2048, 524287, 524288, N - 1]] = True
    queries = np.where(exact[:, None], seen[:, 2:10], rng.choice(list(b"ACGT"), (N, 8)).astype(np.uint8))
    batch = (queries.reshape(-1), ts, np.full(N, 12, np.uint32), trc, (8 * np.arange(N)).astype(np.uint64), np.full(N, 8, np.uint32))
    bound = np.zeros(N, np.uint32)
    full = oc.align_batch(genome, *batch)
    keep = full[0] == 0
    assert keep[exact].all() and N // 3 < keep.sum() < 2 * N // 3 and 0 < (keep & ~exact).sum() < 200
    runs = np.diff(np.flatnonzero(np.diff(keep.astype(np.int8))))
    assert len(set(runs.tolist())) > 8, "the pattern is regular"
    want = _keep_only(full, keep)
    assert (want[2][1:][keep] - want[2][:-1][keep] == 1).all() and (want[3] == (8 << 4)).all()          # an exact copy: 8M

    v = verify.Verifier()
    v.load_genome(genome)
    t0 = time.perf_counter()
    got = v.align_bounded(*batch, bound)
    print(f"bmv_align_bounded of {N} alignments: {time.perf_counter() - t0:.2f} s")
    rejected = v.bounded_stats()["n_rejected"]
    v.close()
    for g, w, what in zip(got, want, ("score", "begin", "cigar_offset", "cigar")):
        assert len(g) == len(w), f"{what}: {len(g)} elements, {len(w)} expected"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what} differs from {bad[0]} on ({bad.size} elements): got {g[bad[:4]]}, want {w[bad[:4]]}"
    assert rejected == int((~keep).sum())
    assert (got[0][~keep] == REJECTED).all()
