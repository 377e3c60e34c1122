#!/usr/bin/env python3
"""What the genotype caller costs on the device: bmg_begin / bmg_add / bmg_call on the record set of tools/bench_pileup.py (the BAM
stream of synthetic 150-base reads, one 150= op each, 24 references, sequences drawn from a synthetic reference at about 1 %
mismatches), beside bmp_add / bmp_finish on the same stream in the same process; the calls are made at the sites bmp lists.
Prints one JSON line.

    python tools/bench_genotype.py [--mb 256] [--device 0] [--reps 5] [--positions 130000000] [--no-host]

ms_add and ms_call are the HIP-event times of bmg_last_stats (the add kernels summed; the call kernel alone, without the upload
of the sites and the download of the calls), bmp_ms_add and bmp_ms_finish those of bmp_last_stats; begin_ms is the wall time of
bmg_begin on the grown context (it zeroes 32 bytes per position and waits); call_wall_ms is bmg_call as the caller sees it.  Each
is the minimum over the repetitions after one warm-up.  Both add kernels issue one atomic per counted base: bmp a 32-bit add
into one of eight counters of a position's 32-byte sector, bmg a 64-bit add into one of four cells of it.  Without --no-host
the cells of the first 100 000 positions and every call are compared with numpy on the host."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--positions", type=int, default=130_000_000)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    from bench_bgzf import bam_stream
    from bucket_map_amd import genotype, pileup

    # the record set of bench_pileup.kernels, made the same way
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
    res = {"payload_bytes": int(data.size), "records": n, "references": N_REF, "positions": positions, "params": genotype.DEFAULTS,
           "pileup_thresholds": pileup.DEFAULTS}

    p = pileup.Pileup(a.device)
    p.begin(lens, bases)
    p.add(data[: 1000 * RECORD], off[:1001])
    p.finish()
    p_add, p_finish = [], []
    for _ in range(a.reps):
        p.begin(lens, bases)
        p.add(data, off)
        n_sites, stats = p.finish()
        p_add.append(p.ms_add)
        p_finish.append(p.ms_finish)
    sites = p.sites()
    some_counts = p.counts_at(0, 0, min(ref_len, 100000))
    p.close()
    res.update(sites=int(n_sites), bmp_ms_add=round(min(p_add), 3), bmp_ms_add_max=round(max(p_add), 3), bmp_ms_finish=round(min(p_finish), 3))

    g = genotype.Genotype(a.device)
    g.begin(lens)
    g.add(data[: 1000 * RECORD], off[:1001])
    g.call(sites[:1000])
    t_begin, t_add, t_call, w_call = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        g.begin(lens)
        t1 = time.perf_counter()
        g.add(data, off)
        t_add.append(g.ms_add)
        t2 = time.perf_counter()
        calls = g.call(sites)
        w_call.append((time.perf_counter() - t2) * 1e3)
        t_call.append(g.ms_call)
        t_begin.append((t1 - t0) * 1e3)
    some = g.cells_at(0, 0, min(ref_len, 100000))
    g.close()
    counted = int((calls[:, 22]).sum())
    res.update(begin_ms=round(min(t_begin), 3), ms_add=round(min(t_add), 3), ms_add_max=round(max(t_add), 3), ms_call=round(min(t_call), 4),
               call_wall_ms=round(min(w_call), 2))
    res["variants"] = int(((calls[:, 3] & 2) != 0).sum())
    res["het"] = int((((calls[:, 3] & 2) != 0) & (calls[:, 4] != calls[:, 5])).sum())
    res["atomic_adds"] = int(stats[:, 3].sum())                      # every counted base of a letter: the pileup's n_bases (no N in the reads)
    res["atomic_adds_per_ns"] = round(res["atomic_adds"] / (res["ms_add"] * 1e6), 2)
    res["add_stream_GBps"] = round(int(data.size) / res["ms_add"] / 1e6, 1)
    res["add_over_bmp_add"] = round(res["ms_add"] / res["bmp_ms_add"], 2)
    res["bytes_begin"], res["bytes_call"] = 32 * positions, (48 + 32 + 96) * int(n_sites)
    res["begin_share_of_hbm_peak"] = round(res["bytes_begin"] / (res["begin_ms"] * 1e-3) / HBM_PEAK, 3)
    res["depth_at_sites"] = counted
    assert np.array_equal((some >> np.uint64(32)).astype(np.uint32), some_counts[:, :4]), "bmg's counts are bmp's"

    if not a.no_host:
        letter_of = np.full(16, 4, np.int64)
        letter_of[[1, 2, 4, 8]] = [0, 1, 2, 3]
        d = genotype.DEFAULTS
        t0 = time.perf_counter()
        cell = np.zeros(positions * 4, np.uint64)
        for lo in range(0, n, CHUNK):
            hi = min(n, lo + CHUNK)
            packed = rec[lo:hi, SEQ:QUAL]
            letter = letter_of[np.stack([packed >> 4, packed & 15], axis=2).reshape(hi - lo, READ)]
            q = rec[lo:hi, QUAL: QUAL + READ].astype(np.uint64)
            keep = ((q == 255) | (q >= d["min_bq"])) & (letter < 4)
            q_eff = np.where(q == 255, d["q_absent"], np.minimum(q, d["q_cap"])).astype(np.uint64)
            at = (ref[lo:hi] * ref_len + pos[lo:hi])[:, None] + np.arange(READ)
            np.add.at(cell, (at * 4 + letter)[keep], (np.uint64(1) << np.uint64(32)) + q_eff[keep])
        res["host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)   # the cells alone
        assert np.array_equal(cell[: some.size].reshape(-1, 4), some), "the host's cells are the device's"
        by_site = cell.reshape(-1, 4)[sites[:, 0].astype(np.int64) * ref_len + sites[:, 1]]
        assert np.array_equal((by_site >> np.uint64(32)).astype(np.uint32), calls[:, 8:12]), "the calls carry the host's counts"
        # the ten costs of every site, vectorised: the rule of include/bmg.h
        nn, Q = (by_site >> np.uint64(32)).astype(np.int64), (by_site & np.uint64(0xFFFFFFFF)).astype(np.int64)
        M, T = 100 * Q + 477 * nn, 301 * nn
        R = sites[:, 2].astype(np.int64)
        cost = np.zeros((len(sites), 10), np.int64)
        k = 0
        for b in range(4):
            for x in range(b + 1):
                like = M.sum(axis=1) - M[:, x] if x == b else T[:, x] + T[:, b] + M.sum(axis=1) - M[:, x] - M[:, b]
                cost[:, k] = like + d["prior"] * ((R != x).astype(np.int64) + ((R != b) & (b != x)).astype(np.int64))
                k += 1
        snv = ((sites[:, 11] & 1) != 0) & (R < 4) & (nn.sum(axis=1) > 0)
        pl = cost - cost.min(axis=1)[:, None]
        assert np.array_equal(pl[snv], calls[snv, 12:22].astype(np.int64)) and not calls[~snv, 3:8].any(), "the calls' PL are the host's"
        res["host_over_device_add"] = round(res["host_numpy_ms"] / res["ms_add"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
