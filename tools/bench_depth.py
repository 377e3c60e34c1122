#!/usr/bin/env python3
"""What the coverage counter costs on the device: bmc_begin / bmc_add / bmc_finish on the payload of tools/bench_bamsort.py
(the BAM stream of synthetic 150-base reads, one 150= op each, 24 references), the bytes each pass has to move and the share
of the HBM peak that gives, and the same work in numpy on the host (np.add.at on a difference array plus cumsum) on the same
machine.  Prints one JSON line.

    python tools/bench_depth.py [--mb 256] [--device 0] [--reps 5] [--positions 130000000] [--no-host]
    python tools/bench_depth.py --tools [--reads 100000] [--parent-exe PATH] [--dir /tmp/bm_depth]

--positions is the number of reference positions in all: the stream's positions are folded into 24 references of
positions / 24 bases each.  --positions 0 leaves them as they are: 24 references of 130 000 150 bases, 3.1 Gbp and 25 GB of
state.  ms_add and ms_finish are the HIP-event times of bmc_last_stats; begin_ms is the wall time of bmc_begin on the grown
context (it zeroes the differences and waits); each is the minimum over the repetitions after one warm-up.  Bytes: begin
writes 4 per slot, the scan reads the differences twice and writes the depths (12), the tile pass and the emit pass read the
depths once each (8, and 16 per run written).

--tools measures the wall time of bucketmap_align on the `mini` workload of bench.py: -o x.bam --sort three times, the same with
--depth --coverage three times, and -- where --parent-exe names a build of the commit before -- its --sort run three times,
interleaved in one session; best of three and the spread (max - min)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RECORD, N_REF, READ = 287, 24, 150   # bench_bgzf.bam_stream's record size, references and read length
HBM_PEAK = 8.0e12                    # bytes per second, MI355X


def kernels(a):
    from bench_bgzf import bam_stream
    from bucket_map_amd import depth

    n = (a.mb << 20) // RECORD
    data = bam_stream(a.mb << 20, False)[: n * RECORD].copy()
    rec = data.reshape(n, RECORD)
    if a.positions:
        ref_len = a.positions // N_REF
        pos = rec[:, 8:12].copy().view("<i4").reshape(n) % (ref_len - READ + 1)
        rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    else:
        ref_len = 130_000_000 + READ
    lens = [ref_len] * N_REF
    off = np.arange(n + 1, dtype=np.uint64) * RECORD
    slots = sum(lens) + N_REF
    res = {"payload_bytes": int(data.size), "records": n, "references": N_REF, "positions": sum(lens)}

    c = depth.Depth(a.device)
    c.begin(lens)
    c.add(data[: 1000 * RECORD], off[:1001])
    c.finish()
    t_begin, t_add, t_finish, call = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        c.begin(lens)
        t1 = time.perf_counter()
        c.add(data, off)
        n_runs, stats = c.finish()
        call.append((time.perf_counter() - t0) * 1e3)
        t_begin.append((t1 - t0) * 1e3)
        t_add.append(c.ms_add)
        t_finish.append(c.ms_finish)
    runs = c.runs()
    c.close()
    res.update(runs=int(n_runs), begin_ms=round(min(t_begin), 3), ms_add=round(min(t_add), 3), ms_finish=round(min(t_finish), 3),
               call_ms=round(min(call), 2))
    moved = {"begin": 4 * slots, "add": int(data.size), "finish": 20 * slots + 16 * int(n_runs)}
    res["bytes_begin"], res["bytes_add_stream"], res["bytes_finish"] = moved["begin"], moved["add"], moved["finish"]
    res["begin_share_of_hbm_peak"] = round(moved["begin"] / (res["begin_ms"] * 1e-3) / HBM_PEAK, 3)
    res["finish_share_of_hbm_peak"] = round(moved["finish"] / (res["ms_finish"] * 1e-3) / HBM_PEAK, 3)
    res["add_stream_GBps"] = round(moved["add"] / res["ms_add"] / 1e6, 1)
    assert int(stats[:, 0].sum()) == n and int(stats[:, 2].sum()) == n * READ, "every record is counted with all its bases"

    if not a.no_host:
        ref = rec[:, 4:8].copy().view("<i4").reshape(n).astype(np.int64)
        pos = rec[:, 8:12].copy().view("<i4").reshape(n).astype(np.int64)
        best = None
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            d = np.zeros(slots, np.int32)
            at = ref * (ref_len + 1) + pos
            np.add.at(d, at, 1)
            np.add.at(d, at + READ, -1)
            np.cumsum(d, out=d)
            ms = (time.perf_counter() - t0) * 1e3
            best = ms if best is None else min(best, ms)
        res["host_numpy_ms"] = round(best, 1)
        total = int(d.sum(dtype=np.int64))
        assert total == n * READ
        r0 = runs[0]
        assert int(d[int(r0[0]) * (ref_len + 1) + int(r0[1])]) == int(r0[3])
        res["host_over_device"] = round(best / (res["begin_ms"] + res["ms_add"] + res["ms_finish"]), 1)
    print(json.dumps(res))


def tools(a):
    import bench
    from bucket_map_amd import host

    total_bp, bucket_len, read_len, _ = bench.WORKLOADS["mini"]
    os.makedirs(a.dir, exist_ok=True)
    g = host.Genome.synth(20240001, bench.workload_record_lengths("mini", total_bp), 16, profile="uniform")
    g.write_fasta(os.path.join(a.dir, "g.fa"))
    rd = host.Reads(g, bucket_len, read_len, read_len, a.reads, seed=20240003, threads=16)
    rd.write_fastq(os.path.join(a.dir, "reads"))
    exe = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    common = ["-i", "idx", "--genome", "g.fa", "--bucket-len", str(bucket_len), "-r", str(read_len), "-f", "1"]
    r = subprocess.run([exe, "-x", *common], cwd=a.dir, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    variants = {"sort": (exe, ["--sort"]), "sort_depth_coverage": (exe, ["--depth", "out.bedgraph", "--coverage", "out.cov"])}
    if a.parent_exe:
        variants["parent_sort"] = (os.path.abspath(a.parent_exe), ["--sort"])
    wall = {k: [] for k in variants}
    line = ""
    for rep in range(3):
        for name, (tool, extra) in variants.items():
            for f in ("out.bam", "out.bam.bai", "out.bedgraph", "out.cov"):
                if os.path.exists(os.path.join(a.dir, f)):
                    os.remove(os.path.join(a.dir, f))
            t0 = time.perf_counter()
            r = subprocess.run([tool, *common, "-q", "reads.fastq", "-o", "out.bam", *extra], cwd=a.dir, capture_output=True, text=True, timeout=300)
            wall[name].append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr[-2000:]
            line = next((l for l in r.stderr.splitlines() if "Coverage:" in l), line)
    res = {"workload": "mini", "reads": rd.n, "coverage_line": line.strip()}
    for name, w in wall.items():
        res[f"{name}_best_s"], res[f"{name}_spread_s"] = round(min(w), 3), round(max(w) - min(w), 3)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--positions", type=int, default=130_000_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--tools", action="store_true")
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--parent-exe", default="")
    ap.add_argument("--dir", default="/tmp/bm_depth")
    a = ap.parse_args()
    (tools if a.tools else kernels)(a)


if __name__ == "__main__":
    main()
