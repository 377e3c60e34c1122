#!/usr/bin/env python3
"""Throughput of bmz_deflate against zlib on 16 host threads, on the same payload: the BAM stream of synthetic 150-base
reads (bm_synth-style: uniform bases, qualities around Q36 with low-quality tails, positions over a 3 Gbp genome), cut
every 65 280 bytes.  Prints one JSON line.

    python tools/bench_bgzf.py [--mb 256] [--device 0] [--reps 3] [--constant-quals]

`call` times are PCIe-inclusive (the whole bmz_deflate call: upload from ordinary host memory, kernels, download);
`kernels` are the HIP-event times of bmz_last_stats.  The comparison is host zlib, never the kernel against itself."""
import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))


def bam_stream(n_bytes, constant_quals, seed=20240001):
    """Fixed-size records of 150-base reads: 36 bytes of fields, an 11-byte name, one CIGAR op, 75 bytes of bases, 150 of
    qualities, NM:C and MD:Z."""
    rng = np.random.default_rng(seed)
    l_seq, name_len = 150, 11
    tags = np.frombuffer(b"NMC\0MDZ150\0", np.uint8)
    size = 36 + name_len + 4 + 75 + l_seq + tags.size
    n = n_bytes // size + 1
    rec = np.zeros((n, size), np.uint8)
    fixed = np.zeros(n, dtype=[("block_size", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                               ("n_cigar", "<u2"), ("flag", "<u2"), ("l_seq", "<u4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")])
    fixed["block_size"], fixed["l_name"], fixed["n_cigar"], fixed["l_seq"] = size - 4, name_len, 1, l_seq
    fixed["ref"] = rng.integers(0, 24, n)
    fixed["pos"] = rng.integers(0, 130_000_000, n)
    fixed["mapq"] = np.minimum(60, rng.integers(0, 90, n))
    fixed["bin"] = 4681 + (fixed["pos"] >> 14)
    fixed["flag"] = rng.choice([0, 16], n)
    fixed["nref"], fixed["npos"] = -1, -1
    rec[:, :36] = fixed.view(np.uint8).reshape(n, 36)
    k = np.arange(n, dtype=np.int64)
    rec[:, 36] = ord("r")
    for j in range(9):
        rec[:, 37 + j] = 48 + (k // 10 ** (8 - j)) % 10
    rec[:, 47:51] = np.frombuffer(np.array([l_seq << 4 | 7], "<u4").tobytes(), np.uint8)
    nib = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, (n, l_seq))]
    rec[:, 51:126] = nib[:, 0::2] << 4 | nib[:, 1::2]
    if constant_quals:
        rec[:, 126:276] = 40
    else:
        q = np.clip(rng.normal(36, 4, (n, l_seq)) - np.maximum(0, np.arange(l_seq) - 110) * rng.random((n, 1)) * 0.4, 2, 41)
        rec[:, 126:276] = q.astype(np.uint8)
    rec[:, 276:] = tags
    rec[:, 279] = rng.integers(0, 4, n)
    return rec.reshape(-1)[:n_bytes].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--constant-quals", action="store_true")
    a = ap.parse_args()
    from bucket_map_amd import bgzf

    data = bam_stream(a.mb << 20, a.constant_quals)
    view = memoryview(data)
    blocks = [view[at: at + bgzf.BLOCK_MAX] for at in range(0, data.size, bgzf.BLOCK_MAX)]
    z = bgzf.Compressor(a.device)
    z.deflate(data[: 4 * bgzf.BLOCK_MAX])                                  # code objects, first allocations
    call_ms, kernel_ms = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out, offsets, forms = z.deflate(data)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        kernel_ms.append(z.ms_kernels)
    z.close()
    res = {"payload_bytes": int(data.size), "blocks": len(blocks), "quals": "constant" if a.constant_quals else "varied",
           "bmz_bytes": len(out), "forms_stored_fixed_dynamic": forms,
           "bmz_call_ms": round(min(call_ms), 2), "bmz_call_GBps": round(data.size / min(call_ms) / 1e6, 2),
           "bmz_kernels_ms": round(min(kernel_ms), 2), "bmz_kernels_GBps": round(data.size / min(kernel_ms) / 1e6, 2)}
    with ThreadPoolExecutor(16) as pool:
        for level in (1, 6):
            best = None
            for _ in range(a.reps if level == 1 else 1):
                t0 = time.perf_counter()
                total = sum(pool.map(lambda b: len(zlib.compress(b, level)) + 20, blocks))   # the zlib wrapper (6) swapped for BGZF's (26)
                ms = (time.perf_counter() - t0) * 1e3
                best = ms if best is None else min(best, ms)
            res[f"zlib{level}_bytes"] = total
            res[f"zlib{level}_16_threads_ms"] = round(best, 2)
            res[f"zlib{level}_16_threads_GBps"] = round(data.size / best / 1e6, 2)
    res["bmz_over_zlib1_bytes"] = round(len(out) / res["zlib1_bytes"], 4)
    res["bmz_over_zlib6_bytes"] = round(len(out) / res["zlib6_bytes"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
