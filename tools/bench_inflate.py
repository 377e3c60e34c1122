#!/usr/bin/env python3
"""Throughput of bmu_inflate against zlib on 16 host threads, on the same blocks, and the tools' wall time on compressed
against plain inputs (GPU box).  Prints one JSON line per measurement.

    python tools/bench_inflate.py [--workload egu] [--reads 1000000] [--read-len 300] [--reps 3] [--dir /tmp/bm_inflate]
                                  [--no-e2e] [--parent-dir DIR]

Payloads: the FASTQ of the end-to-end leg (tools/e2e_cli.py: --reads reads of --read-len bases) and the workload's FASTA,
each compressed at zlib level 6 into 65 280-byte BGZF blocks.  `call` times are PCIe-inclusive (the whole bmu_inflate call:
layout, upload from ordinary host memory, kernel, download); `kernels` are the HIP-event times of bmu_last_stats.  The
comparison is the host's zlib.decompress of the same blocks on 16 threads, never the kernel against itself.

End to end: `bucketmap` and `bucketmap_align` on (reads.fastq, g.fa) and on (reads.fastq.gz, g.fa.gz), wall time of the
map run, --reps each, interleaved.  --parent-dir names a folder with the parent commit's libbmf.so / bucketmap /
bucketmap_align: their plain-input runs are timed in the same session, so the plain path can be compared with its own
run-to-run spread."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))
import bench  # noqa: E402
from bucket_map_amd import host, inflate  # noqa: E402

HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK = 65280


def bgzf_block(piece):
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = z.compress(piece) + z.flush()
    return HEAD + (len(raw) + 25).to_bytes(2, "little") + raw + zlib.crc32(piece).to_bytes(4, "little") + len(piece).to_bytes(4, "little")


def compress_file(path, pool):
    data = memoryview(open(path, "rb").read())
    blocks = list(pool.map(bgzf_block, [data[at: at + BLOCK] for at in range(0, len(data), BLOCK)]))
    with open(path + ".gz", "wb") as f:
        for b in blocks:
            f.write(b)
        f.write(EOF)
    return len(data), blocks


def measure(name, path, pool, u, reps):
    n, blocks = compress_file(path, pool)
    blob = np.frombuffer(b"".join(blocks) + EOF, np.uint8)
    u.inflate(blob[: sum(map(len, blocks[:4]))])                          # code objects, first allocations
    call_ms, kernel_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = u.inflate(blob)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        kernel_ms.append(u.ms_kernels)
    assert len(out) == n
    payloads = [(bytes(b[18:-8]), int.from_bytes(b[-4:], "little")) for b in blocks]
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        total = sum(pool.map(lambda p: len(zlib.decompress(p[0], -15, p[1])), payloads))
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    assert total == n
    res = {"payload": name, "text_bytes": n, "compressed_bytes": int(blob.size), "blocks": len(blocks) + 1,
           "deflate_blocks_stored_fixed_dynamic": [u.n_stored, u.n_fixed, u.n_dynamic],
           "bmu_call_ms": round(min(call_ms), 2), "bmu_call_GBps": round(n / min(call_ms) / 1e6, 2),
           "bmu_kernels_ms": round(min(kernel_ms), 2), "bmu_kernels_GBps": round(n / min(kernel_ms) / 1e6, 2),
           "zlib_16_threads_ms": round(best, 2), "zlib_16_threads_GBps": round(n / best / 1e6, 2)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="egu")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dir", default="/tmp/bm_inflate")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--parent-dir", default="")
    a = ap.parse_args()

    total_bp, bucket_len, _, _ = bench.WORKLOADS[a.workload]
    os.makedirs(a.dir, exist_ok=True)
    lens = [total_bp] if a.workload == "mini" else bench.workload_record_lengths(a.workload, total_bp)
    g = host.Genome.synth(20240001, lens, 16)
    g.write_fasta(os.path.join(a.dir, "g.fa"))
    rd = host.Reads(g, bucket_len, a.read_len, a.read_len, a.reads, seed=20240003, threads=16)
    rd.write_fastq(os.path.join(a.dir, "reads"))
    u = inflate.Inflater(a.device)
    with ThreadPoolExecutor(16) as pool:
        measure("fastq", os.path.join(a.dir, "reads.fastq"), pool, u, a.reps)
        measure("fasta", os.path.join(a.dir, "g.fa"), pool, u, a.reps)
    u.close()
    if a.no_e2e:
        return

    common = ["-i", "idx", "--bucket-len", str(bucket_len), "-r", str(a.read_len), "-f", "1"]
    product = os.path.join(ROOT, "bucket-map_amd")
    subprocess.run([os.path.join(product, "bucketmap"), "-x", *common, "--genome", "g.fa"], cwd=a.dir, capture_output=True, check=True, timeout=600)
    legs = [("this", product, "reads.fastq", "g.fa"), ("this", product, "reads.fastq.gz", "g.fa.gz")]
    if a.parent_dir:
        legs.append(("parent", os.path.abspath(a.parent_dir), "reads.fastq", "g.fa"))
    for tool in ("bucketmap", "bucketmap_align"):
        walls = {leg: [] for leg in legs}
        for _ in range(a.reps):
            for leg in legs:
                out = os.path.join(a.dir, "out.sam")
                if os.path.exists(out):
                    os.remove(out)
                t0 = time.perf_counter()
                r = subprocess.run([os.path.join(leg[1], tool), *common, "--genome", leg[3], "-q", leg[2], "-o", "out.sam"], cwd=a.dir,
                                   capture_output=True, text=True, timeout=600)
                walls[leg].append(round(time.perf_counter() - t0, 3))
                if r.returncode:
                    raise SystemExit(f"{tool} {leg}: exit {r.returncode}\n{r.stderr[-2000:]}")
        for leg in legs:
            print(json.dumps({"tool": tool, "build": leg[0], "reads": leg[2], "genome": leg[3], "wall_s": walls[leg],
                              "best_s": min(walls[leg]), "spread_s": round(max(walls[leg]) - min(walls[leg]), 3)}), flush=True)


if __name__ == "__main__":
    main()
