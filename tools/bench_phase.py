#!/usr/bin/env python3
"""What the read-backed phaser costs on the device: bmk_begin / bmk_add / bmk_finish beside bmg_add on the same records in the
same process, on two record sets.  Prints one JSON line.

    python tools/bench_phase.py [--mb 256] [--long-mb 64] [--device 0] [--reps 5] [--positions 8000000] [--long-positions 2000000]

"short" is the record set of tools/bench_genotype.py (the BAM stream of synthetic 150-base reads, one 150= op each,
24 references, about 1 % mismatches), here drawn from TWO haplotypes that differ at one base in a thousand (every other record
from the second one), over fewer positions so that the depth makes het calls.  "long" is 10 000-base reads with an =/X CIGAR of
2 001 ops (an X every ten bases, about 10 % edits) from the same kind of pair of haplotypes.  In both the phase sites are the het
calls bmg makes at the sites bmp lists, as in the tools.

ms_add and ms_finish are the HIP-event times of bmk_last_stats (the add kernels summed; the pick, jump, mark and out kernels of
bmk_finish), bmg_ms_add that of bmg_last_stats; each is the minimum over the repetitions after one warm-up.  bmg's add reads every
base and issues one 64-bit atomic per counted base; bmk's add reads the CIGAR and, per site under the record, one quality byte and
one nibble, and issues one 32-bit atomic per pair of observed sites within reach."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pileup import CHUNK, N_REF, QUAL, READ, RECORD, SEQ  # noqa: E402

NIB = np.array([1, 2, 4, 8], np.uint8)
HET_EVERY = 1000
LONG_READ, LONG_X = 10_000, 1000                         # bases of a long read; its X ops (one in every ten bases)


def haplotypes(rng, n_ref, ref_len):
    """(genome of haplotype 0, of haplotype 1): they differ at base 500 of every thousand."""
    one = rng.integers(0, 4, n_ref * ref_len, dtype=np.uint8)
    two = one.copy()
    at = np.arange(HET_EVERY // 2, n_ref * ref_len, HET_EVERY)
    two[at] = (two[at] + rng.integers(1, 4, at.size, dtype=np.uint8)) & 3
    return one, two


def short_records(mb, positions):
    from bench_bgzf import bam_stream
    n = (mb << 20) // RECORD
    data = bam_stream(mb << 20, False)[: n * RECORD].copy()
    rec = data.reshape(n, RECORD)
    ref_len = positions // N_REF
    pos = rec[:, 8:12].copy().view("<i4").reshape(n) % (ref_len - READ + 1)
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    ref = rec[:, 4:8].copy().view("<i4").reshape(n).astype(np.int64)
    rng = np.random.default_rng(20240023)
    haps = haplotypes(rng, N_REF, ref_len)
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        at = (ref[lo:hi] * ref_len + pos[lo:hi])[:, None] + np.arange(READ)
        letters = np.where((np.arange(lo, hi) % 2 == 0)[:, None], haps[0][at], haps[1][at])
        wrong = rng.random(letters.shape) < 0.01
        letters[wrong] = (letters[wrong] + rng.integers(1, 4, int(wrong.sum()), dtype=np.uint8)) & 3
        codes = NIB[letters]
        rec[lo:hi, SEQ:QUAL] = codes[:, 0::2] << 4 | codes[:, 1::2]
    off = np.arange(n + 1, dtype=np.uint64) * RECORD
    return data, off, [ref_len] * N_REF, haps[0]


def long_records(mb, positions):
    """10 000-base reads, CIGAR (e=, 1X) x 1 000, e=: the X of every ten bases lies 1 .. 8 bases into them."""
    n_ops = 2 * LONG_X + 1
    size = 36 + 2 + 4 * n_ops + LONG_READ // 2 + LONG_READ
    n = max(1, (mb << 20) // size)
    rng = np.random.default_rng(20240024)
    haps = haplotypes(rng, 1, positions)
    pos = rng.integers(0, positions - LONG_READ + 1, n)
    x_at = 1 + 10 * np.arange(LONG_X)[None, :] + rng.integers(0, 8, (n, LONG_X))
    eq = np.empty((n, LONG_X + 1), np.int64)
    eq[:, 0], eq[:, 1:-1], eq[:, -1] = x_at[:, 0], x_at[:, 1:] - x_at[:, :-1] - 1, LONG_READ - 1 - x_at[:, -1]
    ops = np.empty((n, n_ops), "<u4")
    ops[:, 0::2], ops[:, 1::2] = eq << 4 | 7, 1 << 4 | 8
    rec = np.zeros((n, size), np.uint8)
    head = np.zeros(n, np.dtype([("block_size", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"),
                                 ("flag", "<u2"), ("l_seq", "<u4"), ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4")]))
    head["block_size"], head["pos"], head["l_name"], head["mapq"], head["bin"] = size - 4, pos, 2, 60, 4680
    head["n_cigar"], head["l_seq"], head["next_ref"], head["next_pos"] = n_ops, LONG_READ, -1, -1
    head["flag"] = 16 * (np.arange(n) % 4 // 2)
    rec[:, :36] = head.view(np.uint8).reshape(n, 36)
    rec[:, 36] = ord("r")
    rec[:, 38: 38 + 4 * n_ops] = ops.view(np.uint8).reshape(n, 4 * n_ops)
    seq_at = 38 + 4 * n_ops
    for lo in range(0, n, 256):
        hi = min(n, lo + 256)
        at = pos[lo:hi, None] + np.arange(LONG_READ)
        letters = np.where((np.arange(lo, hi) % 2 == 0)[:, None], haps[0][at], haps[1][at])
        rows = np.arange(hi - lo)[:, None]
        letters[rows, x_at[lo:hi]] = (letters[rows, x_at[lo:hi]] + rng.integers(1, 4, (hi - lo, LONG_X), dtype=np.uint8)) & 3
        codes = NIB[letters]
        rec[lo:hi, seq_at: seq_at + LONG_READ // 2] = codes[:, 0::2] << 4 | codes[:, 1::2]
    rec[:, seq_at + LONG_READ // 2:] = 30
    off = np.arange(n + 1, dtype=np.uint64) * size
    return rec.reshape(-1), off, [positions], haps[0]


def measure(name, data, off, lens, genome, device, reps):
    from bucket_map_amd import genotype, phase, pileup
    bases = [np.frombuffer(b"ACGT", np.uint8)[genome[sum(lens[:r]): sum(lens[: r + 1])]] for r in range(len(lens))]
    res = {"payload_bytes": int(data.size), "records": int(off.size - 1), "references": len(lens), "positions": int(sum(lens))}
    p = pileup.Pileup(device)
    p.begin(lens, bases)
    p.add(data, off)
    n_sites, _ = p.finish()
    sites = p.sites()
    p.close()
    g = genotype.Genotype(device)
    warm = min(off.size - 1, 1000)
    g.begin(lens)
    g.add(data[: int(off[warm])], off[: warm + 1])
    g_add = []
    for _ in range(reps):
        g.begin(lens)
        g.add(data, off)
        calls = g.call(sites)
        g_add.append(g.ms_add)
    g.close()
    k = phase.Phase(device)
    k.begin(lens, calls)
    k.add(data[: int(off[warm])], off[: warm + 1])
    k.finish()
    t_add, t_finish = [], []
    for _ in range(reps):
        H = k.begin(lens, calls)
        k.add(data, off)
        stats = k.finish()
        t_add.append(k.ms_add)
        t_finish.append(k.ms_finish)
    words = k.phase()
    k.close()
    phased = (words[:, phase.W_FLAGS] & phase.PHASED) != 0
    longest = int((calls[words[phased, phase.W_CALL], 1].astype(np.int64) - words[phased, phase.W_ROOT_POS] + 1).max(initial=0))
    res.update(pileup_sites=int(n_sites), phase_sites=int(H), phased=int(stats[1]), blocks=int(stats[2]), observations=int(stats[3]), longest_block_bases=longest,
               bmg_ms_add=round(min(g_add), 3), bmg_ms_add_max=round(max(g_add), 3), ms_add=round(min(t_add), 3), ms_add_max=round(max(t_add), 3),
               ms_finish=round(min(t_finish), 4), ms_finish_max=round(max(t_finish), 4))
    res["add_over_bmg_add"] = round(res["ms_add"] / res["bmg_ms_add"], 3)
    res["observations_per_ns"] = round(res["observations"] / (res["ms_add"] * 1e6), 3)
    return {name: res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--long-mb", type=int, default=64)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--positions", type=int, default=8_000_000)
    ap.add_argument("--long-positions", type=int, default=2_000_000)
    a = ap.parse_args()
    from bucket_map_amd import phase
    out = {"params": phase.DEFAULTS}
    out.update(measure("short", *short_records(a.mb, a.positions), a.device, a.reps))
    out.update(measure("long", *long_records(a.long_mb, a.long_positions), a.device, a.reps))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
