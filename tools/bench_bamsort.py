#!/usr/bin/env python3
"""What coordinate-sorting on the device adds to the BAM path: bms_sort_deflate by stage and as a whole call against
bmz_deflate of the same unsorted bytes (the path without --sort), on the payload of tools/bench_bgzf.py (the BAM stream of
synthetic 150-base reads, varied qualities, 24 references, positions uniform over 130 M).  The host comparison is a stable
sort of the keys (numpy's, standing in for std::stable_sort), the copy of the records, and zlib level 1 on 16 threads.  The
gather's bytes per second stand beside a device-to-device hipMemcpy of the same bytes.  Prints one JSON line.

    python tools/bench_bamsort.py [--mb 256] [--device 0] [--reps 5]

`call` times are PCIe-inclusive (upload from ordinary host memory, kernels, downloads); stage times are the HIP-event times
of bms_last_stats / bmz_last_stats; each figure is the minimum over the repetitions after one warm-up call."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RECORD = 287          # bench_bgzf.bam_stream's record size


def d2d_copy(n_bytes, device, reps):
    """hipMemcpy device to device between two buffers of n_bytes, timed by HIP events on the null stream."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipSetDevice(device))
    ok(hip.hipMalloc(C.byref(src), n_bytes))
    ok(hip.hipMalloc(C.byref(dst), n_bytes))
    ok(hip.hipMemset(src, 1, n_bytes))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    best = None
    for _ in range(reps + 1):                                  # the first is the warm-up
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpy(dst, src, n_bytes, 3))                # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float(0)
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        if _ > 0:
            best = ms.value if best is None else min(best, ms.value)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    hip.hipFree(src)
    hip.hipFree(dst)
    return {"d2d_copy_ms": round(best, 3), "d2d_copy_GBps_read_plus_write": round(2 * n_bytes / best / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from bench_bgzf import bam_stream
    from bucket_map_amd import bamsort, bgzf

    n = (a.mb << 20) // RECORD
    data = bam_stream(a.mb << 20, False)[: n * RECORD].copy()
    assert int(data[:4].view("<u4")[0]) == RECORD - 4
    off = np.arange(n + 1, dtype=np.uint64) * RECORD
    res = {"payload_bytes": int(data.size), "records": n}

    z = bgzf.Compressor(a.device)
    z.deflate(data[: 4 * bgzf.BLOCK_MAX])
    call, kern = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        z.deflate(data)
        call.append((time.perf_counter() - t0) * 1e3)
        kern.append(z.ms_kernels)
    z.close()
    res["bmz_call_ms"], res["bmz_kernels_ms"] = round(min(call), 2), round(min(kern), 2)

    s = bamsort.Sorter(a.device)
    s.sort_deflate(data[: 1000 * RECORD], off[:1001])
    call, stage = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out, perm, so = s.sort_deflate(data, off)
        call.append((time.perf_counter() - t0) * 1e3)
        stage.append((s.ms_sort, s.ms_gather, s.ms_deflate))
    res["radix_passes"] = s.n_passes
    s.close()
    res["bms_call_ms"] = round(min(call), 2)
    for k, name in enumerate(("keys_sort", "gather", "deflate")):
        res[f"bms_{name}_ms"] = round(min(x[k] for x in stage), 3)
    res["bms_call_over_bmz_call"] = round(res["bms_call_ms"] / res["bmz_call_ms"], 3)
    res["sort_and_gather_over_deflate_kernels"] = round((res["bms_keys_sort_ms"] + res["bms_gather_ms"]) / res["bms_deflate_ms"], 3)
    res["gather_GBps_read_plus_write"] = round(2 * data.size / res["bms_gather_ms"] / 1e6, 1)
    res["sorted_bam_bytes"] = len(out)

    res.update(d2d_copy(data.size, a.device, a.reps))          # a device-to-device copy of the same bytes, for scale

    rec = data.reshape(n, RECORD)
    best_sort = best_copy = None
    for _ in range(max(1, a.reps // 2)):
        t0 = time.perf_counter()
        key = rec[:, 4:8].copy().view("<u4").reshape(n).astype(np.uint64) << np.uint64(32) | (rec[:, 8:12].copy().view("<u4").reshape(n) + np.uint32(1)).astype(np.uint64)
        order = np.argsort(key, kind="stable")
        t1 = time.perf_counter()
        host_sorted = rec[order]
        t2 = time.perf_counter()
        best_sort = (t1 - t0) * 1e3 if best_sort is None else min(best_sort, (t1 - t0) * 1e3)
        best_copy = (t2 - t1) * 1e3 if best_copy is None else min(best_copy, (t2 - t1) * 1e3)
    assert np.array_equal(order.astype(np.uint32), perm), "the host's stable order differs from the device's"
    flat = memoryview(host_sorted.reshape(-1))
    blocks = [flat[at: at + bgzf.BLOCK_MAX] for at in range(0, data.size, bgzf.BLOCK_MAX)]
    best = None
    with ThreadPoolExecutor(16) as pool:
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            sum(pool.map(lambda b: len(zlib.compress(b, 1)), blocks))
            ms = (time.perf_counter() - t0) * 1e3
            best = ms if best is None else min(best, ms)
    res["host_stable_sort_ms"], res["host_copy_ms"], res["host_zlib1_16_threads_ms"] = round(best_sort, 1), round(best_copy, 1), round(best, 1)
    res["host_total_ms"] = round(best_sort + best_copy + best, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
