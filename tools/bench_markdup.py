#!/usr/bin/env python3
"""What duplicate marking on the device adds to the sorted BAM path: bmd_mark_sort_deflate by stage and as a whole call
against bms_sort_deflate of the same bytes (the path with --sort alone), in the same session, on the payload of
tools/bench_bamsort.py made paired: records 2p and 2p + 1 share a name and carry 0x41 / 0x81, and one pair in ten takes the
places and strands of the pair before it, so that the sorts have real runs of equal keys.  Prints one JSON line.

    python tools/bench_markdup.py [--mb 256] [--device 0] [--reps 5] [--dup-every 10]

`call` times are PCIe-inclusive (upload from ordinary host memory, kernels, downloads); stage times are the HIP-event times
of bmd_last_stats / bmd_last_sort_stats / bms_last_stats; each figure is the minimum over the repetitions after one warm-up
call.  `ends` holds the quality sums, the CIGAR ends and the kinds; the quality sums read the bytes, so stream bytes over
`ends` is a lower bound of that kernel's rate, set beside the gather's (which reads and writes every byte)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RECORD = 287          # bench_bgzf.bam_stream's record size


def paired_stream(n_bytes, dup_every):
    from bench_bgzf import bam_stream
    n = n_bytes // RECORD // 2 * 2
    rec = bam_stream(n_bytes, False)[: n * RECORD].reshape(n, RECORD).copy()
    assert int(rec[0, :4].view("<u4")[0]) == RECORD - 4
    rec[1::2, 36:47] = rec[0::2, 36:47]                            # mates share their name
    rec[0::2, 18] = (rec[0::2, 18] & 0x10) | 0x41
    rec[1::2, 18] = (rec[1::2, 18] & 0x10) | 0x81
    p = np.arange(dup_every - 1, n // 2, dup_every)                # these pairs lie where the pair before them lies
    for mate in (0, 1):
        rec[2 * p + mate, 4:12] = rec[2 * (p - 1) + mate, 4:12]
        rec[2 * p + mate, 18] = rec[2 * (p - 1) + mate, 18]
    return rec.reshape(-1), n, int(p.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dup-every", type=int, default=10)
    a = ap.parse_args()
    from bucket_map_amd import bamsort, markdup

    data, n, n_copies = paired_stream(a.mb << 20, a.dup_every)
    off = np.arange(n + 1, dtype=np.uint64) * RECORD
    res = {"payload_bytes": int(data.size), "records": n, "pairs_duplicated": n_copies}

    s = bamsort.Sorter(a.device)
    s.sort_deflate(data[: 1000 * RECORD], off[:1001])
    call, stage = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        s.sort_deflate(data, off)
        call.append((time.perf_counter() - t0) * 1e3)
        stage.append((s.ms_sort, s.ms_gather, s.ms_deflate))
    s.close()
    res["bms_call_ms"] = round(min(call), 2)
    for k, name in enumerate(("keys_sort", "gather", "deflate")):
        res[f"bms_{name}_ms"] = round(min(x[k] for x in stage), 3)

    m = markdup.Marker(a.device)
    m.mark_sort_deflate(data[: 1000 * RECORD], off[:1001])
    call, stage = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out, perm, so, dup, counts = m.mark_sort_deflate(data, off)
        call.append((time.perf_counter() - t0) * 1e3)
        stage.append((m.ms_ends, m.ms_mark, m.ms_sort, m.ms_gather, m.ms_deflate))
    res["bmd_call_ms"] = round(min(call), 2)
    for k, name in enumerate(("ends", "mark", "keys_sort", "gather", "deflate")):
        res[f"bmd_{name}_ms"] = round(min(x[k] for x in stage), 3)
    res["mark_radix_passes"], res["sort_radix_passes"] = m.n_passes, m.n_sort_passes
    res["counts"] = counts
    assert counts[0] == n // 2 and counts[2] >= 2 * n_copies, counts
    end, score, kind = m.ends(data, off)
    res["bmd_ends_alone_ms"] = round(m.ms_ends, 3)
    m.mark(end, score, kind)
    res["bmd_mark_alone_ms"] = round(m.ms_mark, 3)
    m.close()
    res["bmd_call_over_bms_call"] = round(res["bmd_call_ms"] / res["bms_call_ms"], 3)
    res["ends_and_mark_over_deflate_kernels"] = round((res["bmd_ends_ms"] + res["bmd_mark_ms"]) / res["bmd_deflate_ms"], 3)
    res["ends_GBps_read"] = round(data.size / res["bmd_ends_ms"] / 1e6, 1)
    res["gather_GBps_read_plus_write"] = round(2 * data.size / res["bmd_gather_ms"] / 1e6, 1)
    res["marked_bam_bytes"] = len(out)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
