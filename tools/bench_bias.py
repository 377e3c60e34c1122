#!/usr/bin/env python3
"""What the strand-bias and mapping-quality annotator costs on the device: bmb_begin / bmb_add / bmb_annotate on the record set of
tools/bench_genotype.py (the BAM stream of synthetic 150-base reads, one 150= op each, 24 references, sequences
drawn from a synthetic reference at about 1 % mismatches; here every other record is put on the reverse strand), beside bmg_add /
bmg_call on the same stream in the same process; the annotations are made for the calls bmg makes at the sites bmp lists.
Prints one JSON line.

    python tools/bench_bias.py [--mb 256] [--device 0] [--reps 5] [--positions 130000000]

ms_add and ms_annotate are the HIP-event times of bmb_last_stats (the add kernels summed; the annotate kernel alone, without the
upload of the calls and the download of the annotations), bmg_ms_add and bmg_ms_call those of bmg_last_stats; begin_ms is the
wall time of bmb_begin on the grown context (it zeroes 40 bytes per position and waits).  Each is the minimum over the
repetitions after one warm-up.  bmg's add kernel issues one 64-bit atomic per counted base, bmb's two: one into the four strand
cells of the position's 32-byte sector, one into its mapq cell.  The strand cells of the first 100 000 positions are compared
with bmg's counts, the mapq cells' n with their sum.

"kernels" is the resource table of the two kernels as hipcc reports it for gfx950 (-Rpass-analysis=kernel-resource-usage on
csrc/bmb_api.hip); it is a record of the build, not a measurement of this run."""
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

from bench_pileup import CHUNK, N_REF, QUAL, READ, RECORD, SEQ  # noqa: E402

KERNELS = {"bmb::add_kernel": dict(vgprs=98, sgprs=70, scratch=0, lds=0, waves_per_simd=4),
           "bmb::annotate_kernel": dict(vgprs=50, sgprs=25, scratch=0, lds=0, waves_per_simd=8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--positions", type=int, default=130_000_000)
    a = ap.parse_args()

    from bench_bgzf import bam_stream
    from bucket_map_amd import bias, genotype, pileup

    # the record set of bench_genotype, made the same way; then every other record on the reverse strand
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
    rec[1::2, 18] |= 0x10
    lens = [ref_len] * N_REF
    bases = [np.frombuffer(b"ACGT", np.uint8)[genome[r * ref_len: (r + 1) * ref_len]] for r in range(N_REF)]
    off = np.arange(n + 1, dtype=np.uint64) * RECORD
    positions = N_REF * ref_len
    res = {"payload_bytes": int(data.size), "records": n, "references": N_REF, "positions": positions, "params": bias.DEFAULTS, "kernels": KERNELS}

    p = pileup.Pileup(a.device)
    p.begin(lens, bases)
    p.add(data, off)
    n_sites, stats = p.finish()
    sites = p.sites()
    p.close()

    g = genotype.Genotype(a.device)
    g.begin(lens)
    g.add(data[: 1000 * RECORD], off[:1001])
    g_add, g_call = [], []
    for _ in range(a.reps):
        g.begin(lens)
        g.add(data, off)
        calls = g.call(sites)
        g_add.append(g.ms_add)
        g_call.append(g.ms_call)
    some_g = g.cells_at(0, 0, min(ref_len, 100000))
    g.close()
    res.update(sites=int(n_sites), bmg_ms_add=round(min(g_add), 3), bmg_ms_add_max=round(max(g_add), 3), bmg_ms_call=round(min(g_call), 4))

    b = bias.Bias(a.device)
    b.begin(lens)
    b.add(data[: 1000 * RECORD], off[:1001])
    b.annotate(calls[:1000])
    t_begin, t_add, t_note, w_note = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        b.begin(lens)
        t1 = time.perf_counter()
        b.add(data, off)
        t_add.append(b.ms_add)
        t2 = time.perf_counter()
        notes = b.annotate(calls)
        w_note.append((time.perf_counter() - t2) * 1e3)
        t_note.append(b.ms_annotate)
        t_begin.append((t1 - t0) * 1e3)
    strand, mapq = b.cells_at(0, 0, min(ref_len, 100000))
    b.close()
    both = (strand >> np.uint64(32)) + (strand & np.uint64(0xFFFFFFFF))
    assert np.array_equal(both, some_g >> np.uint64(32)), "fwd + rev of bmb's strand cells is bmg's n"
    assert np.array_equal(mapq >> np.uint64(40), both.sum(axis=1)), "n of the mapq cell is the sum of the strand cells"
    done = (notes[:, bias.W_FLAGS] & bias.ANNOTATED) != 0
    assert np.array_equal(done, (calls[:, 3] & 2) != 0), "every variant call is annotated, no other"
    res.update(begin_ms=round(min(t_begin), 3), ms_add=round(min(t_add), 3), ms_add_max=round(max(t_add), 3), ms_annotate=round(min(t_note), 4),
               annotate_wall_ms=round(min(w_note), 2))
    res["annotated"] = int(done.sum())
    res["without_fs"] = int(((notes[:, bias.W_FLAGS] & bias.NO_FS) != 0).sum())
    res["fs_at_cap"] = int((done & (notes[:, bias.W_FS] == bias.FS_CAP)).sum())
    res["counted_bases"] = int(stats[:, 3].sum())                    # every counted base of a letter: the pileup's n_bases (no N in the reads)
    res["atomic_adds"] = 2 * res["counted_bases"]
    res["atomic_adds_per_ns"] = round(res["atomic_adds"] / (res["ms_add"] * 1e6), 2)
    res["add_over_bmg_add"] = round(res["ms_add"] / res["bmg_ms_add"], 2)
    res["bytes_begin"] = 40 * positions
    print(json.dumps(res))


if __name__ == "__main__":
    main()
