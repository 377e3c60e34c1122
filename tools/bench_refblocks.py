#!/usr/bin/env python3
"""What the reference-block pass costs on the device: bmr_run over the cells bmg_add has filled from the record set of
tools/bench_genotype.py (synthetic 150-base reads over 24 references, about 130 M positions), with the default bands and the
positions of bmg's variant calls as the excluded intervals, as the tools pass them.  Prints one JSON line.

    python tools/bench_refblocks.py [--mb 256] [--device 0] [--reps 5] [--positions 130000000] [--no-host]

ms_kernels is the HIP-event time of bmr_last_stats (the kernels alone: without the upload of the reference bases and the
intervals, and without the read of the block count between the two halves), the minimum over the repetitions after one
warm-up; run_wall_ms is bmr_run as the caller sees it.  bytes_moved is what the kernels read and write by their own arithmetic:
conf 32 + 1 in and 8 out per position, heads 4 in and 4 out, the scan 8 in and 4 out, blocks 16 in per position and 64 per
block (the fill and the record), exclude 4 out per excluded position.  Without --no-host the blocks are computed again with
numpy on the host and must equal the device's."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pileup import CHUNK, HBM_PEAK, N_REF, QUAL, READ, RECORD, SEQ  # noqa: E402

GENOTYPES = [(a, b) for b in range(4) for a in range(b + 1)]


def host_blocks(cell, R, excluded, ref_len, bands):
    """The rule of include/bmr.h with numpy over equal references of ref_len positions: cell is (positions, 4) uint64, R the
    reference alleles (4 for none), excluded a bool per position.  Returns the (n_blocks, 8) uint32 array."""
    positions = len(R)
    gq = np.zeros(positions, np.uint8)
    dp = np.zeros(positions, np.uint32)
    step = 1 << 22
    for lo in range(0, positions, step):
        c = cell[lo: lo + step]
        n, Q = (c >> np.uint64(32)).astype(np.int64), (c & np.uint64(0xFFFFFFFF)).astype(np.int64)
        dp[lo: lo + step] = np.minimum(n.sum(axis=1), 2 ** 32 - 1)
        M, T = 100 * Q + 477 * n, 301 * n
        total = M.sum(axis=1)
        L = np.stack([total - M[:, a] if a == b else T[:, a] + T[:, b] + total - M[:, a] - M[:, b] for a, b in GENOTYPES], axis=1)
        r = R[lo: lo + step]
        k_rr = np.array([0, 2, 5, 9, 0])[r]
        rows = np.arange(len(r))
        l_rr = L[rows, k_rr]
        L[rows, k_rr] = np.iinfo(np.int64).max
        h = L.min(axis=1)
        gq[lo: lo + step] = np.where((l_rr <= h) & (r < 4), np.minimum(99, (h - l_rr) // 100), 0)
    band = np.zeros(positions, np.uint8)
    for bound in bands:
        band += gq >= bound
    inside = (R < 4) & ~excluded
    key = np.where(inside, band.astype(np.int16), -1)
    head = inside.copy()
    head[1:] &= key[1:] != key[:-1]
    head[::ref_len] = inside[::ref_len]
    start = np.flatnonzero(head)
    last = inside.copy()                                  # the last position of a block: the next is a head or outside
    last[:-1] &= head[1:] | ~inside[1:]
    end = np.flatnonzero(last) + 1
    assert len(start) == len(end)
    out = np.zeros((len(start), 8), np.uint32)
    if len(start):
        # reduceat over [start, next start): what lies between a block's end and the next start is outside and made neutral
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = start // ref_len, start % ref_len, (end - 1) % ref_len + 1, band[start]
        out[:, 4] = np.minimum.reduceat(np.where(inside, gq, 255), start)
        out[:, 5] = np.minimum.reduceat(np.where(inside, dp, 2 ** 32 - 1).astype(np.uint32), start)
        total = np.add.reduceat(np.where(inside, dp, 0).astype(np.uint64), start)
        out[:, 6], out[:, 7] = (total & np.uint64(0xFFFFFFFF)).astype(np.uint32), (total >> np.uint64(32)).astype(np.uint32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--positions", type=int, default=130_000_000)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    from bench_bgzf import bam_stream
    from bucket_map_amd import genotype, pileup, refblocks

    # the record set of bench_genotype.py, made the same way
    n = (a.mb << 20) // RECORD
    data = bam_stream(a.mb << 20, False)[: n * RECORD].copy()
    rec = data.reshape(n, RECORD)
    ref_len = a.positions // N_REF
    pos = rec[:, 8:12].copy().view("<i4").reshape(n) % (ref_len - READ + 1)
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    ref = rec[:, 4:8].copy().view("<i4").reshape(n).astype(np.int64)
    rng = np.random.default_rng(20240021)
    genome = rng.integers(0, 4, N_REF * ref_len, dtype=np.uint8)
    nib = np.array([1, 2, 4, 8], np.uint8)
    for lo in range(0, n, CHUNK):
        hi = min(n, lo + CHUNK)
        at = (ref[lo:hi] * ref_len + pos[lo:hi])[:, None] + np.arange(READ)
        letters = genome[at]
        wrong = rng.random(letters.shape) < 0.01
        letters[wrong] = (letters[wrong] + rng.integers(1, 4, int(wrong.sum()), dtype=np.uint8)) & 3
        codes = nib[letters]
        rec[lo:hi, SEQ:QUAL] = codes[:, 0::2] << 4 | codes[:, 1::2]
    lens = [ref_len] * N_REF
    bases = [np.frombuffer(b"ACGT", np.uint8)[genome[r * ref_len: (r + 1) * ref_len]] for r in range(N_REF)]
    off = np.arange(n + 1, dtype=np.uint64) * RECORD
    positions = N_REF * ref_len
    res = {"payload_bytes": int(data.size), "records": n, "references": N_REF, "positions": positions, "bands": list(refblocks.DEFAULT_BANDS)}

    p = pileup.Pileup(a.device)
    p.begin(lens, bases)
    p.add(data, off)
    p.finish()
    sites = p.sites()
    p.close()
    g = genotype.Genotype(a.device)
    g.begin(lens)
    g.add(data, off)
    calls = g.call(sites)
    res["ms_add"] = round(g.ms_add, 3)                    # bmg's add kernels over the same records, for scale
    variant = calls[(calls[:, 3] & 2) != 0]
    exclude = np.stack([variant[:, 0], variant[:, 1], variant[:, 1] + 1], axis=1).astype(np.uint32)
    res["excluded_intervals"] = int(len(exclude))

    c = refblocks.RefBlocks(a.device)
    c.run(g, bases, refblocks.DEFAULT_BANDS, exclude)     # the warm-up: it grows the buffers
    t_kernels, t_wall = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        n_blocks = c.run(g, bases, refblocks.DEFAULT_BANDS, exclude)
        t_wall.append((time.perf_counter() - t0) * 1e3)
        t_kernels.append(c.ms_kernels)
    res.update(blocks=int(n_blocks), ms_kernels=round(min(t_kernels), 3), ms_kernels_max=round(max(t_kernels), 3), run_wall_ms=round(min(t_wall), 2),
               bytes_state=int(c.bytes_state))
    res["bytes_moved"] = (33 + 8 + 8 + 12 + 16) * positions + 64 * int(n_blocks) + 4 * int(len(exclude))
    res["bytes_one_read_of_the_cells"] = 32 * positions
    res["GBps"] = round(res["bytes_moved"] / res["ms_kernels"] / 1e6, 1)
    res["share_of_hbm_peak"] = round(res["bytes_moved"] / (res["ms_kernels"] * 1e-3) / HBM_PEAK, 3)
    res["reads_of_the_cells_at_79_percent"] = round(res["ms_kernels"] * 1e-3 / (32 * positions / (0.79 * HBM_PEAK)), 2)
    blocks = c.blocks()
    lengths = (blocks[:, 2] - blocks[:, 1]).astype(np.int64)
    res.update(bases_in_blocks=int(lengths.sum()), longest_block=int(lengths.max(initial=0)), blocks_of_one_base=int((lengths == 1).sum()))

    if not a.no_host:
        cell = np.concatenate([g.cells_at(r, 0, ref_len) for r in range(N_REF)])
        t0 = time.perf_counter()
        excluded = np.zeros(positions, bool)
        excluded[exclude[:, 0].astype(np.int64) * ref_len + exclude[:, 1]] = True
        want = host_blocks(cell, genome.astype(np.int64), excluded, ref_len, refblocks.DEFAULT_BANDS)
        res["host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert want.shape == blocks.shape and np.array_equal(want, blocks), "the host's blocks are the device's"
        res["host_over_device"] = round(res["host_numpy_ms"] / res["ms_kernels"], 1)
    c.close()
    g.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
