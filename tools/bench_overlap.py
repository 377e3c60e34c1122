#!/usr/bin/env python3
"""What the overlap pass costs on the device: bmv_overlap on a batch of 2 x 150 bp pairs on fragments of 200 to 400 bases, both
strands, about a million alignments with 1 % substitutions, every one a single 150M entry -- beside bmv_clip on the same batch
in the same process, which does three of the walks bmv_overlap does.  Prints one JSON line.

    python tools/bench_overlap.py [--pairs 500000] [--device 0] [--reps 5] [--genome 20000000]

ms_overlap is bmv_last_overlap_stats' kernel time under the scores 1 / 2 (range, span, decide, restrict, commit, count and
score passes, two prefix sums, write pass), ms_overlap_unscored the same with match = penalty = 0 (no range pass), ms_clip
bmv_last_clip_stats' (range, count, two prefix sums, write): HIP events, each the minimum over the repetitions after one
warm-up call of each.  call_ms_* are host clocks around the whole calls, uploads and downloads included."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))

READ, LEAD, TAIL = 150, 2, 2
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def batch(n_pairs, n_genome, seed=24):
    """The genome and the batch: alignment 2p is the fragment's left mate, 2p + 1 its right one; in odd pairs the left mate is
    the reverse read.  Windows of LEAD + 150 + TAIL bases, so begin is LEAD on the forward strand and TAIL on the other."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)
    genome = bases[rng.integers(0, 4, n_genome)]
    frag = rng.integers(200, 401, n_pairs)
    g0 = rng.integers(LEAD, n_genome - 400 - TAIL, n_pairs)
    n = 2 * n_pairs
    at = np.empty(n, np.int64)                                   # where each alignment's first column lies
    at[0::2] = g0
    at[1::2] = g0 + frag - READ
    rc = np.zeros(n, np.uint8)
    rc[1::2] = 1
    odd = np.arange(n_pairs) % 2 == 1
    rc[0::2][odd] = 1
    rc[1::2][odd] = 0
    reads = np.empty(n * READ, np.uint8)
    step = 100_000
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        fwd = genome[at[lo:hi, None] + np.arange(READ)]
        err = rng.random(fwd.shape) < 0.01
        fwd = np.where(err, bases[(np.searchsorted(bases, fwd) + 1 + rng.integers(0, 3, fwd.shape)) % 4], fwd)
        rev = COMP[fwd[:, ::-1]]
        reads[lo * READ: hi * READ] = np.where(rc[lo:hi, None] != 0, rev, fwd).ravel()
    ts = (at - LEAD).astype(np.uint64)
    tl = np.full(n, LEAD + READ + TAIL, np.uint32)
    qs = (np.arange(n, dtype=np.uint64) * READ)
    ql = np.full(n, READ, np.uint32)
    begin = np.where(rc != 0, TAIL, LEAD).astype(np.uint32)
    off = np.arange(n + 1, dtype=np.uint64)
    cg = np.full(n, READ << 4, np.uint32)
    mate = (np.arange(n, dtype=np.uint32) ^ 1).astype(np.uint32)
    return genome, (reads, ts, tl, rc, qs, ql, begin, off, cg), mate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from bucket_map_amd import verify

    genome, args, mate = batch(a.pairs, a.genome)
    v = verify.Verifier(device=a.device)
    v.load_genome(genome)
    res = {"alignments": 2 * a.pairs, "pairs": a.pairs, "read": READ, "reps": a.reps}
    runs = {"overlap": lambda: v.overlap(*args, mate, None, match=1, penalty=2),
            "overlap_unscored": lambda: v.overlap(*args, mate, None, match=0, penalty=0),
            "clip": lambda: v.clip(*args, match=1, penalty=2)}
    stats = {"overlap": v.overlap_stats, "overlap_unscored": v.overlap_stats, "clip": v.clip_stats}
    for name, run in runs.items():
        run()                                                    # warm-up: code objects, buffers grown
    ms = {k: [] for k in runs}
    call = {k: [] for k in runs}
    last = {}
    for _ in range(a.reps):
        for name, run in runs.items():                           # alternating, so that a busy moment hits all three
            t0 = time.perf_counter()
            last[name] = run()
            call[name].append((time.perf_counter() - t0) * 1e3)
            ms[name].append(stats[name]()["ms_kernels"])
    st = v.overlap_stats()
    v.close()
    for name in runs:
        res[f"ms_{name}"] = round(min(ms[name]), 3)
        res[f"ms_{name}_max"] = round(max(ms[name]), 3)
        res[f"call_ms_{name}"] = round(min(call[name]), 1)
    res["columns"] = st["columns"]
    res["pairs_cut"] = int(last["overlap"]["pairs_cut"])
    res["bases_cut"] = int(last["overlap"]["bases_cut"])
    res["pairs_cut_unscored"] = int(last["overlap_unscored"]["pairs_cut"])
    res["overlap_over_clip"] = round(res["ms_overlap"] / res["ms_clip"], 2)
    # without mates the pass is bmv_clip: the batch it was timed on is the batch bmv_clip was timed on
    untouched = last["overlap"]["cut"] == 0
    for k in ("score", "clip_left", "clip_right", "pos", "ref_len", "nm"):
        assert np.array_equal(last["overlap"][k][untouched], last["clip"][k][untouched]), k
    assert res["pairs_cut"] > 0
    print(json.dumps(res))


if __name__ == "__main__":
    main()
