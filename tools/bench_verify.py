#!/usr/bin/env python3
"""Throughput of the alignment verifier (include/bmv.h) on a synthetic batch shaped like `bucketmap_align`'s
work on BASELINE configs[1]: one located candidate per read, text window = read + 1 + 2 % (bucket_locator.h:550).

    python tools/bench_verify.py [--reads 1000000] [--len 300] [--indel-rate 0.02] [--cpu-sample 2000]
    python tools/bench_verify.py --long [--long-reads 1000] [--long-len 100000]
    python tools/bench_verify.py --annotate [--reads 20000 --len 10000 --indel-rate 0.1]
    python tools/bench_verify.py --clip [--reads 20000 --len 10000 --indel-rate 0.1]
    python tools/bench_verify.py --realign [--reads 20000 --len 10000 --indel-rate 0.1]
    python tools/bench_verify.py --leftalign [--reads 20000 --len 10000 --indel-rate 0.1]
    python tools/bench_verify.py --best [--groups 20000 --len 10000 --text-len 11001] [--groups 200000 --len 300 --text-len 307]
    python tools/bench_verify.py --paired [--pairs 500000 --len 300] [--frag-auto [--frag-cap 10000]]
    python tools/bench_verify.py --rescue [--rescue-jobs 500000,4000 --rescue-len 150]
    python tools/bench_verify.py --split [--reads 200000 --len 300] [--reads 20000 --len 10000]

Prints one JSON line: alignments/s and cell updates/s of the device kernels (HIP events inside bmv_align),
the wall time of the call (host buffers in, results out), and the CPU restatement (oracle, full DP matrix,
1 core) on a sample beside it.

--long: Verifier.align_long (bmv_align_long, reads beyond 65 536 bases): --long-reads alignments of --long-len bases against
text = len + 1 + 10 % at ONT-like error rates (3 % substitutions, 2.5 % insertions, 2.5 % deletions), then one lone
1 048 576-base query against a 1.15 Mbp text; one JSON line each.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))


def _ont(rng, src, sub=0.03, ins=0.025, dele=0.025):
    """ONT-like noise, vectorised: per base a deletion, else an optional inserted base before it and a substitution."""
    bases = np.frombuffer(b"ACGT", np.uint8)
    r = rng.random(len(src))
    out = np.where(rng.random(len(src)) < sub, bases[rng.integers(0, 4, len(src))], src)
    pair = np.stack([np.where((r >= dele) & (r < dele + ins), bases[rng.integers(0, 4, len(src))], 0),
                     np.where(r >= dele, out, 0)], 1).ravel()
    return pair[pair != 0].astype(np.uint8)


def long_main(args):
    from bucket_map_amd import verify

    rng = np.random.default_rng(20241005)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 16 << 20, dtype=np.uint8)]
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    v = verify.Verifier()
    v.load_genome(genome)

    def run(reads, ts, tl, rc, qs, ql, what, extra):
        best = None
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            score, _, _, cg = v.align_long(reads, ts, tl, rc, qs, ql)
            wall = time.perf_counter() - t0
            st = v.stats()
            if best is None or st["ms_kernels"] < best[0]:
                best = (st["ms_kernels"], wall)
        print(json.dumps({
            "metric": f"bmv_align_long: {what}", "value": st["cells"] / (best[0] * 1e-3), "unit": "cell updates/s",
            "ms_kernels": best[0], "wall_ms": best[1] * 1e3, "cells": st["cells"], "alignments": len(ts),
            "mean_edits_per_base": float((-score / ql).mean()), "cigar_entries": int(len(cg)), **extra}), flush=True)

    # many: ONT-like reads of --long-len bases, either strand
    m, n = args.long_len, args.long_len + 1 + args.long_len // 10
    ts = rng.integers(0, len(genome) - n - 8, args.long_reads).astype(np.uint64)
    rc = rng.integers(0, 2, args.long_reads).astype(np.uint8)
    parts = []
    for a in range(args.long_reads):
        src = genome[int(ts[a]) + 1: int(ts[a]) + 1 + m]
        parts.append(_ont(rng, comp[src][::-1] if rc[a] else src))
    ql = np.array([len(p) for p in parts], np.uint32)
    qs = np.concatenate([[0], np.cumsum(ql[:-1], dtype=np.uint64)]).astype(np.uint64)
    run(np.concatenate(parts), ts, np.full(args.long_reads, n, np.uint32), rc, qs, ql,
        f"{args.long_reads} x ({m} x {n}), ONT-like errors", {"query_len": m, "text_len": n})
    del parts
    # one: a lone 1 048 576-base query against a 1.15 Mbp text
    m, n = 1 << 20, 1_150_000
    t0 = int(rng.integers(0, len(genome) - n))
    q = _ont(rng, genome[t0 + 40_000: t0 + 40_000 + m])[:m]
    run(q, np.array([t0], np.uint64), np.array([n], np.uint32), np.zeros(1, np.uint8), np.zeros(1, np.uint64),
        np.array([len(q)], np.uint32), f"one {len(q)} x {n} alignment, ONT-like errors", {"query_len": len(q), "text_len": n})


def best_main(args):
    """Verifier.align_best on groups of five candidates: the true locus (ONT-like errors from 1 000 bases on, else
    substitutions at --sub), two near copies of it -- planted in the genome, diverged by substitutions worth 0.5 x to 3 x the
    margin -- and two unrelated windows, in random order.  Run with hint = the true locus and with hint = a wrong candidate,
    beside Verifier.align and Verifier.align_bounded (rates 0.15 and 0.1) on the same batch; one JSON line."""
    from bucket_map_amd import verify

    rng = np.random.default_rng(20250903)
    G, m, n = args.groups, args.len, args.text_len or args.len + 1 + int(np.float32(args.indel_rate) * np.float32(args.len))
    margin = max(1, int(np.float32(args.margin_rate) * np.float32(m)))
    bases = np.frombuffer(b"ACGT", np.uint8)
    # the genome: per group its true window and two diverged copies of it, back to back
    genome = bases[rng.integers(0, 4, (G, 3, n), dtype=np.uint8)]
    for c in (1, 2):
        genome[:, c, :] = genome[:, 0, :]
        for g0 in range(0, G, 2048):
            part = genome[g0: g0 + 2048, c, :]
            rate = rng.uniform(0.5, 3.0, (len(part), 1)) * margin / m
            hit = rng.random(part.shape) < rate
            part[hit] = bases[(np.searchsorted(bases, part[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    genome = genome.reshape(-1)
    lead = (n - m) // 2
    parts = []
    for g in range(G):
        src = genome[g * 3 * n + lead: g * 3 * n + lead + m + m // 8]
        if m >= 1000:
            parts.append(_ont(rng, src)[:m])
        else:
            q = src[:m].copy()
            hit = rng.random(m) < args.sub
            q[hit] = bases[rng.integers(0, 4, int(hit.sum()))]
            parts.append(q)
    ql_g = np.array([len(p) for p in parts], np.uint32)
    qs_g = np.concatenate([[0], np.cumsum(ql_g[:-1], dtype=np.uint64)]).astype(np.uint64)
    reads = np.concatenate(parts)
    del parts
    order = np.argsort(rng.random((G, 5)), axis=1)                 # member k of group g is candidate order[g, k]; 0 = true
    own = (np.arange(G, dtype=np.uint64) * 3 * n)[:, None]
    cand = np.concatenate([own + np.arange(3, dtype=np.uint64)[None, :] * n,
                           rng.integers(0, len(genome) - n, (G, 2)).astype(np.uint64)], axis=1)
    ts = np.take_along_axis(cand, order, axis=1).reshape(-1)
    tl = np.full(5 * G, n, np.uint32)
    rc = np.zeros(5 * G, np.uint8)
    qs, ql = np.repeat(qs_g, 5), np.repeat(ql_g, 5)
    off = (np.arange(G + 1, dtype=np.uint32) * 5)
    true_at = np.argmin(order, axis=1).astype(np.uint32)
    wrong_at = np.argmax(order, axis=1).astype(np.uint32)          # an unrelated window
    mg = np.full(G, margin, np.uint32)

    v = verify.Verifier()
    v.load_genome(genome)
    batch = (reads, ts, tl, rc, qs, ql)
    a_ms, a_wall = [], []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        score, begin, co, cg = v.align(*batch)
        a_wall.append(time.perf_counter() - t0)
        a_ms.append(v.stats()["ms_kernels"])
    cells = v.stats()["cells"]
    ref_cols = np.where((cg & 15) != 1, cg >> 4, 0).astype(np.int64)
    run_sum = np.concatenate([[0], np.cumsum(ref_cols)])
    d = -score.astype(np.int64)
    end = begin.astype(np.int64) + run_sum[co[1:].astype(np.int64)] - run_sum[co[:-1].astype(np.int64)]
    del cg
    bounded = {}
    for rate in (0.15, 0.1):
        b_ms, b_screen = [], []
        for _ in range(args.repeat):
            v.align_bounded(*batch, (np.float32(rate) * ql.astype(np.float32)).astype(np.uint32))
            b_ms.append(v.stats()["ms_kernels"])
            b_screen.append(v.bounded_stats()["ms_screen"])
        bst = v.bounded_stats()
        bounded[str(rate)] = {"ms_kernels": b_ms, "ms_screen": b_screen, "rejected_share": bst["n_rejected"] / (5 * G),
                              "screen_cells_share": bst["screen_cells"] / max(cells, 1)}
    want = verify.select_best(d, end, off, mg)
    runs = {}
    for name, hint in (("hint_true", true_at), ("hint_wrong", wrong_at)):
        ms, wall, dist, pick = [], [], [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            got = v.align_best(*batch, off, mg, hint)
            wall.append(time.perf_counter() - t0)
            ms.append(v.stats()["ms_kernels"])
            st = v.best_stats()
            dist.append(st["ms_distance"])
            pick.append(st["ms_pick"])
        wins = got["winner"]
        ok = bool(np.array_equal(wins, want[0]) and np.array_equal(got["edits"], want[1]) and np.array_equal(got["end"], want[2])
                  and np.array_equal(got["score"][wins], score[wins]) and np.array_equal(got["begin"][wins], begin[wins]))
        runs[name] = {"ms_kernels": ms, "ms_distance": dist, "ms_pick": pick,
                      "ms_full_alignments": [a - b - c for a, b, c in zip(ms, dist, pick)], "wall_s": wall,
                      **{k: st[k] for k in ("n_seed", "n_distance", "n_beyond", "n_undecided", "n_realigned", "distance_cells")},
                      "distance_cells_share": st["distance_cells"] / max(cells, 1),
                      "full_alignments_per_group": (st["n_seed"] + st["n_undecided"] + st["n_realigned"]) / G,
                      "best_over_align": min(ms) / min(a_ms), "checks": {"identical_to_align_plus_select_best": ok}}
    print(json.dumps({
        "metric": "bmv_align_best kernels ms (hint = true locus)", "value": min(runs["hint_true"]["ms_kernels"]), "unit": "ms",
        "config": {"groups": G, "candidates": 5, "query_len": m, "text_len": n, "margin": margin},
        "cells": cells, "true_locus_wins": float((want[0] == off[:-1] + true_at).mean()), "mean_edits_true": float(d[off[:-1] + true_at].mean()),
        "align": {"ms_kernels": a_ms, "wall_s": a_wall}, "align_bounded": bounded, "align_best": runs}), flush=True)


def paired_main(args):
    """Verifier.align_paired on --pairs pairs of --len-base reads, fragments of 2 x len: per mate three candidates in random
    order -- the true window, a planted copy of the pair's whole region diverged by substitutions worth 0.5 x to 3 x the margin
    (so the copy holds a second proper combination), and an unrelated window.  Beside it Verifier.align_best on the same batch,
    the mates as groups of their own: ms_pair of the one next to ms_pick of the other.  The picks of the first 2 000 pairs are
    held against verify.select_pairs.  One JSON line."""
    from bucket_map_amd import verify

    rng = np.random.default_rng(20251005)
    P, m = args.pairs, args.len
    n = m + 1 + int(np.float32(args.indel_rate) * np.float32(m))
    frag, lead = 2 * m, 8
    region = frag + 2 * lead + (n - m)
    margin = max(1, int(np.float32(args.margin_rate) * np.float32(m)))
    bases = np.frombuffer(b"ACGT", np.uint8)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    genome = bases[rng.integers(0, 4, (P, 2, region), dtype=np.uint8)]
    genome[:, 1, :] = genome[:, 0, :]
    for p0 in range(0, P, 4096):
        part = genome[p0: p0 + 4096, 1, :]
        hit = rng.random(part.shape) < rng.uniform(0.5, 3.0, (len(part), 1)) * margin / m
        part[hit] = bases[(np.searchsorted(bases, part[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4]
    # mate 1 forward from the fragment's left end, mate 2 the reverse complement of its right end, substitutions at --sub
    reads = np.stack([genome[:, 0, lead: lead + m], comp[genome[:, 0, lead + frag - m: lead + frag]][:, ::-1]], 1).copy()
    hit = rng.random(reads.shape) < args.sub
    reads[hit] = bases[rng.integers(0, 4, int(hit.sum()))]
    reads = reads.reshape(-1)
    genome = genome.reshape(-1)
    at = np.array([lead - (n - m) // 2, lead + frag - m - (n - m) // 2], np.uint64)              # the two mates' windows in a region
    own = (np.arange(P, dtype=np.uint64) * 2 * region)[:, None, None] + at[None, :, None]         # [pair, mate, 1]
    cand = np.concatenate([own, own + np.uint64(region), rng.integers(0, len(genome) - n, (P, 2, 1)).astype(np.uint64)], axis=2)
    order = np.argsort(rng.random((P, 2, 3)), axis=2)
    ts = np.take_along_axis(cand, order, axis=2).reshape(-1)
    N = 6 * P
    tl = np.full(N, n, np.uint32)
    rc = np.tile(np.repeat(np.array([0, 1], np.uint8), 3), P)
    qs = np.repeat(np.arange(2 * P, dtype=np.uint64) * m, 3)
    ql = np.full(N, m, np.uint32)
    off = np.arange(2 * P + 1, dtype=np.uint32) * 3
    mg = np.full(2 * P, margin, np.uint32)
    hint = np.argmin(order, axis=2).reshape(-1).astype(np.uint32)                                 # the true window
    v = verify.Verifier()
    v.load_genome(genome)
    batch = (reads, ts, tl, rc, qs, ql)
    best, pair = {"ms_kernels": [], "ms_pick": [], "ms_distance": [], "wall_s": []}, {"ms_kernels": [], "ms_pair": [], "wall_s": []}
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        v.align_best(*batch, off, mg, hint)
        best["wall_s"].append(time.perf_counter() - t0)
        st = v.best_stats()
        best["ms_kernels"].append(v.stats()["ms_kernels"])
        best["ms_pick"].append(st["ms_pick"])
        best["ms_distance"].append(st["ms_distance"])
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        got = v.align_paired(*batch, off, mg, 1, 1000, hint)
        pair["wall_s"].append(time.perf_counter() - t0)
        pair["ms_kernels"].append(v.stats()["ms_kernels"])
        pair["ms_pair"].append(v.pair_stats()["ms_pair"])
    st, pst = v.best_stats(), v.pair_stats()
    auto = None
    if args.frag_auto:
        # --frag-auto: the same batch through paired_begin (cap 10 000: the tool's default) + paired_finish under the range its
        # own histogram gives; ms_frag is the span and histogram kernels, ms_kernels the whole of begin + finish
        auto = {"ms_kernels": [], "ms_frag": [], "ms_pair": [], "wall_s": []}
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            frag = v.paired_begin(*batch, off, mg, args.frag_cap, hint)
            learned = verify.frag_range(frag["hist"], 64, (1, 1000))
            v.paired_finish(learned["min_frag"], learned["max_frag"])
            auto["wall_s"].append(time.perf_counter() - t0)
            auto["ms_kernels"].append(v.stats()["ms_kernels"])
            auto["ms_frag"].append(v.frag_stats()["ms_kernels"])
            auto["ms_pair"].append(v.pair_stats()["ms_pair"])
        spans = verify.frag_spans(ts[: 6 * min(P, 2000)], tl[: 6 * min(P, 2000)], rc[: 6 * min(P, 2000)], ql[: 6 * min(P, 2000)],
                                  got["edits"][: 6 * min(P, 2000)], got["end"][: 6 * min(P, 2000)], off[: 2 * min(P, 2000) + 1], args.frag_cap)
        auto.update({"cap": args.frag_cap, "histogram_path": "LDS" if args.frag_cap + 1 <= 16384 else "global atomics",
                     "range": [learned["min_frag"], learned["max_frag"]], "learned": learned["learned"],
                     "n_informative": v.frag_stats()["n_informative"], "quartiles": list(learned["quartiles"]),
                     "first_pairs_identical_to_frag_spans": bool(np.array_equal(frag["span"][: len(spans)], spans))})
    k = min(P, 2000)
    want = verify.select_pairs(ts[: 6 * k], tl[: 6 * k], rc[: 6 * k], ql[: 6 * k], got["edits"][: 6 * k], got["end"][: 6 * k],
                               off[: 2 * k + 1], 1, 1000)
    ok = all(np.array_equal(np.asarray(got[key])[: len(want[key])], want[key]) for key in ("pick", "proper", "s1", "s2"))
    print(json.dumps({
        "metric": "bmv_align_paired pair kernel ms", "value": min(pair["ms_pair"]), "unit": "ms",
        "config": {"pairs": P, "candidates_per_mate": 3, "query_len": m, "text_len": n, "margin": margin, "frag_range": [1, 1000]},
        "ms_pair": pair["ms_pair"], "ms_pick_of_align_best": best["ms_pick"], "combinations": pst["combinations"],
        "proper_share": float(got["proper"].mean()), "pairs_with_a_second_combination": float((got["s2"] != verify.PAIR_NONE).mean()),
        "pick_is_not_the_own_winner": float((got["pick"] != got["winner"]).mean()),
        "align_best": best, "align_paired": {**pair, "n_realigned": st["n_realigned"], "n_seed": st["n_seed"]},
        **({"frag_auto": auto} if auto else {}),
        "checks": {"first_pairs_identical_to_select_pairs": bool(ok)}}), flush=True)


def split_main(args):
    """Verifier.split on --reads groups of five candidates: a read of --len bases is a chimera of two halves from unrelated
    places (the second half on the reverse strand for every other read); its candidates, in random order, are the two windows
    that hold the whole read laid around either half -- as the locator places a long read's window -- and three unrelated
    windows.  Every candidate is aligned in full (Verifier.align) once; then --repeat calls of split (ms_range, ms_pick) and,
    on the same batch in the same process, --repeat calls of the unchanged Verifier.clip (its kernel ms: the yardstick).  The
    first groups are held against verify.clip_range and verify.select_segments, every score against clip's.  One JSON line."""
    from bucket_map_amd import verify

    rng = np.random.default_rng(20261014)
    R, m = args.reads, args.len
    n = m + 1 + int(np.float32(args.indel_rate) * np.float32(m))
    h, lead = m // 2, (n - m) // 2
    bases = np.frombuffer(b"ACGT", np.uint8)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    genome = bases[rng.integers(0, 4, 64 << 20, dtype=np.uint8)]
    A = rng.integers(m + lead, len(genome) - 2 * n, R)
    B = rng.integers(m + lead, len(genome) - 2 * n, R)
    second_rc = np.arange(R) % 2 == 1
    reads = np.empty((R, m), np.uint8)
    for r0 in range(0, R, 4096):
        sl = slice(r0, min(R, r0 + 4096))
        reads[sl, :h] = genome[A[sl, None] + np.arange(h)]
        two = genome[B[sl, None] + np.arange(m - h)]
        reads[sl, h:] = np.where(second_rc[sl, None], comp[two][:, ::-1], two)
    hit = rng.random(reads.shape) < args.sub
    reads[hit] = bases[rng.integers(0, 4, int(hit.sum()))]
    # the window around the first half begins `lead` before it; around the second half: h + lead before it on the forward
    # strand, `lead` before it on the reverse strand (there the read's second half comes first)
    own = np.stack([A - lead, np.where(second_rc, B - lead, B - h - lead)], 1)
    cand = np.concatenate([own, rng.integers(0, len(genome) - n, (R, 3))], 1).astype(np.uint64)
    strand = np.concatenate([np.zeros((R, 1), np.uint8), second_rc[:, None].astype(np.uint8), rng.integers(0, 2, (R, 3)).astype(np.uint8)], 1)
    order = np.argsort(rng.random((R, 5)), axis=1)
    ts = np.take_along_axis(cand, order, axis=1).reshape(-1)
    rc = np.take_along_axis(strand, order, axis=1).reshape(-1)
    N = 5 * R
    tl, ql = np.full(N, n, np.uint32), np.full(N, m, np.uint32)
    qs = np.repeat(np.arange(R, dtype=np.uint64) * m, 5)
    groups = np.arange(R + 1, dtype=np.uint32) * 5
    reads = reads.reshape(-1)
    v = verify.Verifier()
    v.load_genome(genome)
    batch = (reads, ts, tl, rc, qs, ql)
    t0 = time.perf_counter()
    _, begin, off, cg = v.align(*batch)
    align_s = time.perf_counter() - t0
    split, clip = {"ms_range": [], "ms_pick": [], "wall_s": []}, {"ms_kernels": [], "wall_s": []}
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        got = v.split(*batch, begin, off, cg, groups)
        split["wall_s"].append(time.perf_counter() - t0)
        st = v.split_stats()
        split["ms_range"].append(st["ms_range"])
        split["ms_pick"].append(st["ms_pick"])
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        clipped = v.clip(*batch, begin, off, cg)
        clip["wall_s"].append(time.perf_counter() - t0)
        clip["ms_kernels"].append(v.clip_stats()["ms_kernels"])
    k = max(10, min(500, 200_000 // m, R))
    want = {key: [] for key in ("score", "q_lo", "q_hi", "g_lo", "g_hi")}
    for a in range(5 * k):
        c = verify.clip_range(genome[int(ts[a]): int(ts[a]) + n], reads[int(qs[a]): int(qs[a]) + m], int(rc[a]), int(begin[a]),
                              cg[int(off[a]): int(off[a + 1])])
        for key, x in (("score", c["score"]), ("q_lo", c["q_lo"]), ("q_hi", c["q_hi"]), ("g_lo", int(ts[a]) + c["g_off_lo"]),
                       ("g_hi", int(ts[a]) + c["g_off_hi"])):
            want[key].append(x)
    pick = verify.select_segments(want["score"], want["q_lo"], want["q_hi"], want["g_lo"], want["g_hi"], rc[: 5 * k], groups[: k + 1], 40, 500, 8)
    ok = all(got[key][: 5 * k].tolist() == want[key] for key in want) and all(np.array_equal(got[key][:k], pick[key]) for key in pick)
    print(json.dumps({
        "metric": "bmv_split range pass ms", "value": min(split["ms_range"]), "unit": "ms",
        "config": {"reads": R, "candidates_per_read": 5, "query_len": m, "text_len": n, "sub": args.sub, "min_score": 40,
                   "max_overlap_permille": 500, "max_segments": 8, "clip_scores": [1, 2]},
        "ms_range": split["ms_range"], "ms_pick": split["ms_pick"], "columns": st["columns"],
        "columns_per_s": st["columns"] / (min(split["ms_range"]) * 1e-3), "segments": st["n_segments"],
        "reads_with_two_segments": float((got["n_seg"] == 2).mean()),
        "ms_kernels_of_bmv_clip_same_batch": clip["ms_kernels"], "range_pass_over_clip": min(split["ms_range"]) / min(clip["ms_kernels"]),
        "split": split, "clip": clip, "align_wall_s": align_s,
        "checks": {"first_groups_identical_to_the_restatement": bool(ok),
                   "every_score_is_clips": bool(np.array_equal(got["score"], clipped["score"]))}}), flush=True)


def rescue_main(args):
    """Verifier.rescue on jobs of --rescue-len-base mates under the range 1,1000 and max_edits = 0.1 x len: the anchor at a random
    place of a random genome, on either strand, the mate sampled from the other end of a fragment of 2 x len .. 900 bases with
    substitutions at --sub.  Per job count of --rescue-jobs: the kernels' ms with the job cut into one part
    (BMV_RESCUE_PARTS=1) and into the host's own choice of parts, and beside them Verifier.align_bounded on the same views under
    the same bounds.  The results of the two rescue runs are held against each other and against align_bounded's scores.  One
    JSON line per job count."""
    from bucket_map_amd import verify

    rng = np.random.default_rng(20251106)
    m = args.rescue_len
    bases = np.frombuffer(b"ACGT", np.uint8)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    genome = bases[rng.integers(0, 4, 64 << 20, dtype=np.uint8)]
    v = verify.Verifier()
    v.load_genome(genome)
    for J in [int(x) for x in args.rescue_jobs.split(",")]:
        frag = rng.integers(2 * m, 901, J)
        left = rng.integers(2_000, len(genome) - 4_000, J)
        anchor_rc = (np.arange(J) % 2).astype(np.uint8)         # the anchor is the reverse read: the mate lies at the left end
        mate_at = np.where(anchor_rc != 0, left, left + frag - m)
        anchor_at = np.where(anchor_rc != 0, left + frag - m, left)
        reads = genome[mate_at[:, None] + np.arange(m)[None, :]]
        reads[anchor_rc == 0] = comp[reads[anchor_rc == 0]][:, ::-1]
        hit = rng.random(reads.shape) < args.sub
        reads[hit] = bases[rng.integers(0, 4, int(hit.sum()))]
        ats = (anchor_at - 3).astype(np.uint64)                 # the anchor's view: 3 bases of slack either side
        atl = np.full(J, m + 7, np.uint32)
        aend = np.where(anchor_rc != 0, m + 4, m + 3).astype(np.uint32)
        jobs = (reads.reshape(-1), ats, atl, anchor_rc, np.full(J, m, np.uint32), aend, np.zeros(J, np.uint64),
                np.full(J, len(genome), np.uint64), np.arange(J, dtype=np.uint64) * m, np.full(J, m, np.uint32),
                np.full(J, m // 10, np.uint32))
        runs = {}
        for name, forced in (("one_part", "1"), ("host_choice", None)):
            if forced is None:
                os.environ.pop("BMV_RESCUE_PARTS", None)
            else:
                os.environ["BMV_RESCUE_PARTS"] = forced
            ms, wall = [], []
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                got = v.rescue(*jobs, 1, 1000)
                wall.append(time.perf_counter() - t0)
                ms.append(v.rescue_stats()["ms_kernels"])
            runs[name] = {"ms_kernels": ms, "wall_s": wall, "parts": v.rescue_stats()["parts"], "cells": v.rescue_stats()["cells"], "got": got}
        os.environ.pop("BMV_RESCUE_PARTS", None)
        one, own = runs["one_part"].pop("got"), runs["host_choice"].pop("got")
        same = all(np.array_equal(one[k], own[k]) for k in one)
        views = (jobs[0], own["text_start"], own["text_len"], own["text_rc"], jobs[8], jobs[9])
        b_ms, b_wall = [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            score, _, _, _ = v.align_bounded(*views, jobs[10])
            b_wall.append(time.perf_counter() - t0)
            b_ms.append(v.stats()["ms_kernels"])
        d = np.where(score == verify.REJECTED, verify.BEYOND, -score.astype(np.int64)).astype(np.uint32)
        print(json.dumps({
            "metric": f"bmv_rescue kernels ms, {J} jobs", "value": min(runs["host_choice"]["ms_kernels"]), "unit": "ms",
            "config": {"jobs": J, "query_len": m, "max_edits": m // 10, "frag_range": [1, 1000], "mean_view_len": float(own["text_len"].mean())},
            "rescue_one_part": runs["one_part"], "rescue_host_choice": runs["host_choice"],
            "align_bounded_same_views": {"ms_kernels": b_ms, "wall_s": b_wall},
            "rescued_share": float((own["edits"] != verify.BEYOND).mean()), "proper_share": float(own["proper"].mean()),
            "checks": {"parts_do_not_change_the_results": bool(same), "edits_equal_align_bounded": bool(np.array_equal(d, own["edits"]))}}),
            flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rescue", action="store_true", help="Verifier.rescue beside Verifier.align_bounded on the same views (see rescue_main)")
    ap.add_argument("--rescue-jobs", default="500000,4000", help="--rescue: the job counts, one run each")
    ap.add_argument("--rescue-len", type=int, default=150, help="--rescue: the mates' length")
    ap.add_argument("--split", action="store_true", help="Verifier.split beside Verifier.clip on groups of five candidates (see split_main)")
    ap.add_argument("--paired", action="store_true", help="Verifier.align_paired beside Verifier.align_best (see paired_main)")
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--frag-auto", action="store_true", help="--paired: also paired_begin + paired_finish under the learned range")
    ap.add_argument("--frag-cap", type=int, default=10_000, help="--frag-auto: the cap (beyond 16 383 the histogram uses global atomics)")
    ap.add_argument("--best", action="store_true", help="Verifier.align_best on groups of five candidates (see best_main)")
    ap.add_argument("--groups", type=int, default=20_000)
    ap.add_argument("--text-len", type=int, default=0, help="--best: the window's length (default: as the tool computes it)")
    ap.add_argument("--margin-rate", type=float, default=0.05, help="--best: margin = max(1, rate x query length)")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=300)
    ap.add_argument("--indel-rate", type=float, default=0.02)
    ap.add_argument("--sub", type=float, default=0.002)
    ap.add_argument("--indels", type=float, default=0.0, metavar="F",
                    help="plant F x --len indel events of 1..3 bases in every read (half deletions, half insertions; default: "
                         "substitutions only): what --leftalign needs to have anything to move")
    ap.add_argument("--cpu-sample", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--mixed", type=int, default=0,
                    help="query lengths log-uniform in [MIXED, --len] (forward strand only): a batch of several length classes")
    ap.add_argument("--bounded", type=float, default=None, metavar="RATE",
                    help="also run Verifier.align_bounded on the same batch with max_edits = RATE * query length: kernels ms of "
                         "both (every repeat), the screen's ms and cells, the rejected share")
    ap.add_argument("--annotate", action="store_true",
                    help="also run Verifier.annotate on the batch's results: kernels ms of every repeat, bytes read (text + query, "
                         "each once), bytes / time, and the ratio to align's kernels ms on the same batch")
    ap.add_argument("--clip", action="store_true",
                    help="also run Verifier.clip (match 1, penalty 2) and Verifier.annotate on the batch's results: the clipping "
                         "pass's kernels ms of every repeat, the columns walked, and the ratios to annotate's and to align's "
                         "kernels ms on the same batch")
    ap.add_argument("--realign", action="store_true",
                    help="also run Verifier.realign (scores 1,4,6,1, band 16) on the batch's results: the pass's kernels ms of every "
                         "repeat with forward and traceback apart (the library's BMV_LOG_CLASSES line), band cells / time, and the "
                         "ratio to align's kernels ms on the same batch")
    ap.add_argument("--leftalign", action="store_true",
                    help="also run Verifier.leftalign and Verifier.annotate on the batch's results: the normalisation pass's "
                         "kernels ms of every repeat, the columns compared, the alignments changed, the merges and dropped bases, "
                         "and the ratio to annotate's kernels ms on the same batch")
    ap.add_argument("--decoys", type=float, default=0.0, metavar="F",
                    help="this share of the alignments takes its text window from an unrelated place (a wrong locus)")
    ap.add_argument("--long", action="store_true", help="Verifier.align_long on reads beyond 65 536 bases (see above)")
    ap.add_argument("--long-reads", type=int, default=1000)
    ap.add_argument("--long-len", type=int, default=100_000)
    args = ap.parse_args()

    import torch  # noqa: F401  (HIP runtime first, as in bench.py)
    from bucket_map_amd import verify
    if args.long:
        return long_main(args)
    if args.best:
        return best_main(args)
    if args.paired:
        return paired_main(args)
    if args.rescue:
        return rescue_main(args)
    if args.split:
        return split_main(args)

    rng = np.random.default_rng(20240003)
    m = args.len
    width = m + 1 + int(np.float32(args.indel_rate) * np.float32(m))
    genome = rng.integers(0, 4, 64 << 20, dtype=np.uint8)
    genome = np.frombuffer(b"ACGT", np.uint8)[genome]
    start = rng.integers(0, len(genome) - width - 8, args.reads).astype(np.uint64)
    rc = rng.integers(0, 2, args.reads).astype(np.uint8) * (0 if args.mixed else 1)
    # reads: the window's bases from offset 1 (so begin = 1), substitutions only + strand flips, built vectorised
    idx = start[:, None] + 1 + np.arange(m, dtype=np.uint64)[None, :]
    inserted = None
    if args.indels > 0:                                # --indels: events of 1..3 bases, half deletions, half insertions
        k = max(1, int(round(args.indels * m)))
        at = rng.integers(0, m, (args.reads, k))
        size = rng.integers(1, 4, (args.reads, k))
        dele = rng.random((args.reads, k)) < 0.5
        row = np.broadcast_to(np.arange(args.reads)[:, None], at.shape)
        shift = np.zeros((args.reads, m + 4), np.int32)  # a deletion skips window bases from its place on, an insertion lags behind
        np.add.at(shift, (row[dele], at[dele]), size[dele].astype(np.int32))
        np.add.at(shift, (row[~dele], at[~dele] + size[~dele]), -size[~dele].astype(np.int32))
        shift = np.cumsum(shift[:, :m], axis=1)
        inserted = np.zeros((args.reads, m + 4), bool)
        for d in range(3):
            sel = ~dele & (size > d)
            inserted[row[sel], at[sel] + d] = True
        inserted = inserted[:, :m]
        idx = start[:, None] + np.clip(1 + np.arange(m, dtype=np.int64)[None, :] + shift, 0, width - 1).astype(np.uint64)
    reads = genome[idx]
    if inserted is not None:
        reads[inserted] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(inserted.sum()))]
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    flip = rc.astype(bool)
    reads[flip] = comp[reads[flip]][:, ::-1]
    subs = rng.random(reads.shape) < args.sub
    reads[subs] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(subs.sum()))]
    reads = np.ascontiguousarray(reads).reshape(-1)
    qs = (np.arange(args.reads, dtype=np.uint64) * m)
    ql = np.full(args.reads, m, np.uint32)
    tl = np.full(args.reads, width, np.uint32)
    if args.mixed:                                     # each read keeps its first ql bases
        ql = np.exp(rng.uniform(np.log(args.mixed), np.log(m), args.reads)).astype(np.uint32)
        tl = (ql + 1 + (np.float32(args.indel_rate) * ql.astype(np.float32)).astype(np.uint32)).astype(np.uint32)

    if args.decoys > 0:                                # wrong loci: the read stays, its window moves
        decoy = rng.random(args.reads) < args.decoys
        start = np.where(decoy, rng.integers(0, len(genome) - width - 8, args.reads).astype(np.uint64), start)

    v = verify.Verifier()
    v.load_genome(genome)
    best_ms, best_wall, all_ms = None, None, []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        score, begin, off, cg = v.align(reads, start, tl, rc, qs, ql)
        wall = time.perf_counter() - t0
        st = v.stats()
        all_ms.append(st["ms_kernels"])
        if best_ms is None or st["ms_kernels"] < best_ms:
            best_ms, best_wall = st["ms_kernels"], wall
    cells = st["cells"]
    bounded = None
    if args.bounded is not None:
        bound = (np.float32(args.bounded) * ql.astype(np.float32)).astype(np.uint32)
        b_ms, b_wall, b_screen = [], [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            bs, bb, bo, bc = v.align_bounded(reads, start, tl, rc, qs, ql, bound)
            b_wall.append(time.perf_counter() - t0)
            b_ms.append(v.stats()["ms_kernels"])
            bst = v.bounded_stats()
            b_screen.append(bst["ms_screen"])
        expect = -score.astype(np.int64) > bound
        acc = ~expect
        lens, lens_all = np.diff(bo.astype(np.int64)), np.diff(off.astype(np.int64))
        bounded = {"rate": args.bounded, "decoys": args.decoys, "ms_kernels_align": all_ms, "ms_kernels_bounded": b_ms,
                   "ms_screen": b_screen, "wall_s_bounded": b_wall, "screen_cells": bst["screen_cells"],
                   "screen_cells_share": bst["screen_cells"] / max(cells, 1), "rejected_share": bst["n_rejected"] / args.reads,
                   "bounded_over_align": min(b_ms) / min(all_ms),
                   "checks": {"rejected_set_is_score_beyond_bound": bool(np.array_equal(bs == verify.REJECTED, expect)),
                              "accepted_identical_to_align": bool(np.array_equal(bs[acc], score[acc]) and np.array_equal(bb[acc], begin[acc])
                                                                  and np.array_equal(lens[acc], lens_all[acc])
                                                                  and int(lens.sum()) == len(bc))}}

    annotate = None
    if args.annotate:
        a_ms, a_wall = [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            nm, pos, ref_len, xo, xc, ro, rb = v.annotate(reads, start, tl, rc, qs, ql, begin, off, cg)
            a_wall.append(time.perf_counter() - t0)
            a_ms.append(v.annotate_stats()["ms_kernels"])
        covered = np.diff(off.astype(np.int64)) > 0                    # (an empty CIGAR reads nothing)
        n_bytes = int(ref_len.sum()) + int(ql[covered].sum())
        annotate = {"ms_kernels_annotate": a_ms, "ms_kernels_align": all_ms, "wall_s_annotate": a_wall,
                    "columns": v.annotate_stats()["columns"], "bytes_read": n_bytes,
                    "bytes_per_s": n_bytes / (min(a_ms) * 1e-3), "spread": (max(a_ms) - min(a_ms)) / min(a_ms),
                    "annotate_over_align": min(a_ms) / min(all_ms), "xcigar_entries": int(len(xc)), "ref_bases": int(len(rb)),
                    "checks": {"nm_is_minus_score": bool(np.array_equal(nm.astype(np.int64), -score.astype(np.int64)))}}

    clip = None
    if args.clip:
        c_ms, c_wall, a_ms = [], [], []
        for _ in range(args.repeat):
            v.annotate(reads, start, tl, rc, qs, ql, begin, off, cg)
            a_ms.append(v.annotate_stats()["ms_kernels"])
            t0 = time.perf_counter()
            got = v.clip(reads, start, tl, rc, qs, ql, begin, off, cg)
            c_wall.append(time.perf_counter() - t0)
            c_ms.append(v.clip_stats()["ms_kernels"])
        by_op = lambda ops: int((got["xcigar"] >> 4)[np.isin(got["xcigar"] & 15, ops)].sum())     # entry lengths of these ops
        clip = {"ms_kernels_clip": c_ms, "ms_kernels_annotate": a_ms, "ms_kernels_align": all_ms, "wall_s_clip": c_wall,
                "columns": v.clip_stats()["columns"], "spread": (max(c_ms) - min(c_ms)) / min(c_ms),
                "clip_over_annotate": min(c_ms) / min(a_ms), "clip_over_align": min(c_ms) / min(all_ms),
                "xcigar_entries": int(len(got["xcigar"])), "clipped_bases": int(got["clip_left"].sum() + got["clip_right"].sum()),
                "checks": {"queries_are_covered": bool(by_op([4, 7, 8, 1]) == int(ql[np.diff(off.astype(np.int64)) > 0].sum())),
                           "scores_add_up": bool(int(got["score"].sum()) == by_op([7]) - 2 * int(got["nm"].sum()))}}

    realign = None
    if args.realign:
        import re
        import tempfile
        r_ms, r_wall, r_parts = [], [], []
        os.environ["BMV_LOG_CLASSES"] = "1"
        for _ in range(args.repeat):
            sys.stderr.flush()
            with tempfile.TemporaryFile() as log:              # the library's own line, written to file descriptor 2
                keep = os.dup(2)
                os.dup2(log.fileno(), 2)
                try:
                    t0 = time.perf_counter()
                    got = v.realign(reads, start, tl, rc, qs, ql, begin, off, cg)
                    r_wall.append(time.perf_counter() - t0)
                finally:
                    os.dup2(keep, 2)
                    os.close(keep)
                log.seek(0)
                line = log.read().decode(errors="replace")
            found = re.search(r"forward ([0-9.]+) ms, traceback ([0-9.]+) ms, scan and gather ([0-9.]+) ms", line)
            r_parts.append([float(x) for x in found.groups()] if found else None)
            rst = v.realign_stats()
            r_ms.append(rst["ms_kernels"])
        del os.environ["BMV_LOG_CLASSES"]
        lens = np.diff(got["cigar_offset"].astype(np.int64))
        realign = {"ms_kernels_realign": r_ms, "ms_forward_traceback_gather": r_parts, "ms_kernels_align": all_ms,
                   "wall_s_realign": r_wall, "band_cells": rst["cells"], "band_cells_per_s": rst["cells"] / (min(r_ms) * 1e-3),
                   "passed_through": rst["n_passed_through"], "spread": (max(r_ms) - min(r_ms)) / min(r_ms),
                   "realign_over_align": min(r_ms) / min(all_ms), "cigar_entries": int(len(got["cigar"])),
                   "changed_cigars": int((lens != np.diff(off.astype(np.int64))).sum()),
                   "checks": {"all_realigned": bool(got["realigned"].all() or rst["n_passed_through"] > 0),
                              "score_at_least_the_edit_bound": bool((got["score"].astype(np.int64) >= ql.astype(np.int64) + 12 * score.astype(np.int64)).all())}}

    leftalign = None
    if args.leftalign:
        l_ms, l_wall, a_ms = [], [], []
        for _ in range(args.repeat):
            nm = v.annotate(reads, start, tl, rc, qs, ql, begin, off, cg)[0]
            a_ms.append(v.annotate_stats()["ms_kernels"])
            t0 = time.perf_counter()
            got = v.leftalign(reads, start, tl, rc, qs, ql, begin, off, cg)
            l_wall.append(time.perf_counter() - t0)
            l_ms.append(v.leftalign_stats()["ms_kernels"])
        lst = v.leftalign_stats()
        nm2 = v.annotate(reads, start, tl, rc, qs, ql, got["begin"], got["cigar_offset"], got["cigar"])[0]
        again = v.leftalign(reads, start, tl, rc, qs, ql, got["begin"], got["cigar_offset"], got["cigar"])
        leftalign = {"ms_kernels_leftalign": l_ms, "ms_kernels_annotate": a_ms, "ms_kernels_align": all_ms, "wall_s_leftalign": l_wall,
                     "columns_compared": lst["compared"], "changed": lst["n_changed"], "merges": lst["merges"],
                     "dropped_bases": lst["dropped"], "gap_entries": int(((cg & 15) != 0).sum()),
                     "spread": (max(l_ms) - min(l_ms)) / min(l_ms), "leftalign_over_annotate": min(l_ms) / min(a_ms),
                     "checks": {"nm_is_nm_in_minus_dropped": bool(np.array_equal(nm2.astype(np.int64), nm.astype(np.int64) - got["dropped"])),
                                "idempotent": bool(not again["changed"].any() and np.array_equal(again["cigar"], got["cigar"])
                                                   and np.array_equal(again["begin"], got["begin"]))}}

    ns = min(args.cpu_sample, args.reads)
    same, cpu = None, None
    if ns > 0:                                         # (--cpu-sample 0: no oracle in the process at all -- bench.py's leg)
        from oracle import oracle_c as oc
        t0 = time.perf_counter()
        s_ref, b_ref, o_ref, c_ref = oc.align_batch(genome, reads, start[:ns], tl[:ns], rc[:ns], qs[:ns], ql[:ns])
        cpu_s = time.perf_counter() - t0
        same = bool(np.array_equal(score[:ns], s_ref) and np.array_equal(begin[:ns], b_ref) and
                    np.array_equal(off[: ns + 1], o_ref) and np.array_equal(cg[: int(o_ref[ns])], c_ref))
        cpu = {"value": ns / cpu_s, "unit": "alignments/s", "cores": 1, "kind": "port", "sample": f"first {ns} alignments"}
    print(json.dumps({
        "metric": "verified alignments/s (device kernels)", "value": args.reads / (best_ms * 1e-3), "unit": "alignments/s",
        "config": {"alignments": args.reads, "query_len": m, "text_len": width, "mixed_from": args.mixed},
        "ms_kernels": best_ms, "cell_updates_per_s": cells / (best_ms * 1e-3), "wall_s_host_buffers": best_wall,
        "mean_edits": float(-score.mean()), "cigar_entries": int(len(cg)),
        "cpu_baseline": cpu,
        "bounded": bounded,
        "annotate": annotate,
        "clip": clip,
        "realign": realign,
        "leftalign": leftalign,
        "checks": {"sample_identical_to_oracle": same},
    }))


if __name__ == "__main__":
    main()
