#!/usr/bin/env python3
"""What the indel caller costs on the device: bmn_begin / bmn_add / bmn_finish on a record set in the style of
tools/bench_pileup.py (the BAM stream of synthetic 150-base reads on 24 references), here with three CIGAR ops per record: a
fraction --indel-rate of the records carries one insertion (72= kI rest=) or one deletion (74= kD 76=) of 1 .. 4 bases, whose kind,
length and bases are a function of the read's position, so that reads of one position agree; the others are 70= 40= 40=.  bmp_add runs on the
same stream in the same process.  Prints one JSON line.

    python tools/bench_indel.py [--mb 256] [--device 0] [--reps 5] [--positions 130000000] [--indel-rate 0.1] [--no-host]

ms_add and ms_finish are the HIP-event times of bmn_last_stats (the two passes of every add with the scan and the host's read of
the event count between them; the sorts, scans and passes of finish with the host's reads), bmp_ms_add that of bmp_last_stats.
Each is the minimum over the repetitions after one warm-up.  Without --no-host the alleles, the calls, the sums and the cover
of the first reference are compared with numpy on the host."""
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

from bench_pileup import N_REF, READ  # noqa: E402

OLD, RECORD = 287, 295                     # bench_bgzf.bam_stream's record and the same with two more CIGAR ops
CIGAR, SEQ = 47, 59                        # where a record's CIGAR and its packed sequence start


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--positions", type=int, default=130_000_000)
    ap.add_argument("--indel-rate", type=float, default=0.1)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()

    from bench_bgzf import bam_stream
    from bucket_map_amd import indel, pileup

    n = (a.mb << 20) // RECORD
    old = bam_stream(n * OLD, False)[: n * OLD].reshape(n, OLD)
    rec = np.zeros((n, RECORD), np.uint8)
    rec[:, :CIGAR] = old[:, :CIGAR]
    rec[:, SEQ:] = old[:, CIGAR + 4:]
    rec[:, 0:4] = np.frombuffer(np.array([RECORD - 4], "<u4").tobytes(), np.uint8)
    rec[:, 16:18] = np.frombuffer(np.array([3], "<u2").tobytes(), np.uint8)
    ref_len = a.positions // N_REF
    pos = old[:, 8:12].copy().view("<i4").reshape(n).astype(np.int64) % (ref_len - READ - 8)
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    ref = old[:, 4:8].copy().view("<i4").reshape(n).astype(np.int64)
    rng = np.random.default_rng(20240023)
    has = rng.random(n) < a.indel_rate
    # kind, length and bases by the read's place: a multiplicative hash of the slot behind its first 71 bases
    lead = np.where(has, 72, 70)
    h = (((ref * ref_len + pos + 71) * 2654435761) >> 7) & 0xFFFF
    is_ins = (h & 1) == 1
    lead = np.where(has & ~is_ins, 74, lead)
    size = 1 + ((h >> 1) & 3)
    ops = np.zeros((n, 3), np.int64)
    ops[:, 0] = lead << 4 | 7
    ops[:, 1] = np.where(has, np.where(is_ins, size << 4 | 1, size << 4 | 2), 40 << 4 | 7)
    ops[:, 2] = np.where(has, np.where(is_ins, (READ - 72 - size) << 4 | 7, (READ - 74) << 4 | 7), 40 << 4 | 7)
    rec[:, CIGAR:SEQ] = ops.astype("<u4").view(np.uint8).reshape(n, 12)
    # the inserted bases of an anchor agree: the 2-bit letters of the hash, written over the read's own
    ins_rows = np.flatnonzero(has & is_ins)
    nib = np.array([1, 2, 4, 8], np.uint8)
    packed = rec[:, SEQ: SEQ + READ // 2]
    codes = np.stack([packed >> 4, packed & 15], axis=2).reshape(n, READ)
    for j in range(4):
        rows = ins_rows[size[ins_rows] > j]
        codes[rows, 72 + j] = nib[(h[rows] >> (3 + 2 * j)) & 3]
    rec[:, SEQ: SEQ + READ // 2] = codes[:, 0::2] << 4 | codes[:, 1::2]
    data = rec.reshape(-1)
    lens = [ref_len] * N_REF
    off = np.arange(n + 1, dtype=np.uint64) * RECORD
    positions = N_REF * ref_len
    res = {"payload_bytes": int(data.size), "records": n, "references": N_REF, "positions": positions, "indel_rate": a.indel_rate,
           "params": indel.DEFAULTS}

    p = pileup.Pileup(a.device)
    bases = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ref_len)] for _ in range(N_REF)]
    p.begin(lens, bases)
    p.add(data[: 1000 * RECORD], off[:1001])
    p.finish()
    p_add = []
    for _ in range(a.reps):
        p.begin(lens, bases)
        p.add(data, off)
        _, p_stats = p.finish()
        p_add.append(p.ms_add)
    p.close()
    res.update(bmp_ms_add=round(min(p_add), 3), bmp_ms_add_max=round(max(p_add), 3))

    c = indel.Indel(a.device)
    c.begin(lens)
    c.add(data[: 1000 * RECORD], off[:1001])
    c.finish()
    t_begin, t_add, t_finish, w_finish = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        c.begin(lens)
        t1 = time.perf_counter()
        c.add(data, off)
        t2 = time.perf_counter()
        stats = c.finish()
        w_finish.append((time.perf_counter() - t2) * 1e3)
        t_begin.append((t1 - t0) * 1e3), t_add.append(c.ms_add), t_finish.append(c.ms_finish)
    alleles, calls = c.alleles(), c.calls()
    cover0 = c.cover_at(0, 0, ref_len)
    res.update(begin_ms=round(min(t_begin), 3), ms_add=round(min(t_add), 3), ms_add_max=round(max(t_add), 3), ms_finish=round(min(t_finish), 3),
               ms_finish_max=round(max(t_finish), 3), finish_wall_ms=round(min(w_finish), 2), events=c.n_events, alleles=c.n_alleles, calls=c.n_calls)
    res["variants"] = int(((calls[:, 5] & 2) != 0).sum())
    res["events_per_s"] = round(c.n_events / (res["ms_add"] * 1e-3))
    res["add_stream_GBps"] = round(int(data.size) / res["ms_add"] / 1e6, 1)
    res["add_over_bmp_add"] = round(res["ms_add"] / res["bmp_ms_add"], 3)
    c.close()
    assert np.array_equal(stats, p_stats[:, :3]), "bmn's sums are bmp's"

    if not a.no_host:
        d = indel.DEFAULTS
        t0 = time.perf_counter()
        rows = np.flatnonzero(has)
        slot = ref[rows] * ref_len + pos[rows] + lead[rows] - 1
        w1 = size[rows] | np.where(is_ins[rows], 1 << 31, 0)
        seq = np.zeros(rows.size, np.int64)
        for j in range(4):
            two = np.log2(codes[rows, 72 + j]).astype(np.int64)
            seq |= np.where(is_ins[rows] & (size[rows] > j), two << (2 * j), 0)
        keys = np.stack([slot, w1, seq], axis=1)
        uniq, count = np.unique(keys, axis=0, return_counts=True)        # rows ascending by (slot, w1, seq)
        want = np.zeros((len(uniq), 8), np.int64)
        want[:, 0], want[:, 1], want[:, 2], want[:, 3], want[:, 5] = uniq[:, 0] // ref_len, uniq[:, 0] % ref_len, uniq[:, 1], uniq[:, 2], count
        assert rows.size == res["events"] and np.array_equal(want, alleles.astype(np.int64)), "the host's alleles are the device's"
        end = pos + READ + np.where(has, np.where(is_ins, -size, size), 0)
        diff = np.zeros(positions + 1, np.int64)
        np.add.at(diff, ref * ref_len + pos, 1)
        np.add.at(diff, ref * ref_len + end - 1, -1)
        cover = np.cumsum(diff[:-1])
        assert np.array_equal(cover[:ref_len], cover0.astype(np.int64)), "the host's cover is the device's"
        # per anchor: E, the first allele of the largest n (none is `other` here), the site test and the three costs
        anchor, first, group = np.unique(uniq[:, 0], return_index=True, return_inverse=True)
        E = np.bincount(group, weights=count).astype(np.int64)
        best = np.lexsort((np.arange(len(uniq)), -count, group))[first]
        n_alt, D = count[best], cover[anchor]
        site = (D > 0) & (n_alt >= d["min_alt"]) & (n_alt * 1000000 >= d["min_frac_ppm"] * D)
        n_ref = np.maximum(D - E, 0)
        cost = np.stack([100 * d["q_indel"] * n_alt, 301 * (n_ref + n_alt) + d["prior"], 100 * d["q_indel"] * n_ref + d["prior"]], axis=1)[site]
        g = np.argmin(cost, axis=1)                                      # the first of the smallest: RR, then RA
        got = calls.astype(np.int64)
        assert len(got) == int(site.sum()) and np.array_equal(got[:, 6], g) and np.array_equal(got[:, 13:16], cost - cost.min(axis=1)[:, None])
        assert np.array_equal(got[:, [9, 10, 11, 12]], np.stack([n_ref, n_alt, E - n_alt, D], axis=1)[site]) and np.array_equal(got[:, :5], want[best][site][:, :5])
        res["host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
