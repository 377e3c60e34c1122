#!/usr/bin/env python3
"""What the pileup counter costs on the device: bmp_begin / bmp_add / bmp_finish on the payload of tools/bench_depth.py (the BAM
stream of synthetic 150-base reads, one 150= op each, 24 references), with the reads' sequences drawn from a synthetic
reference at about 1 % mismatches; beside it bmc_add / bmc_finish on the same stream in the same session, the atomic adds and
the bytes each pass has to move, and the same counting in numpy on the host (np.add.at over [position][8]) on the same machine.
Prints one JSON line.

    python tools/bench_pileup.py [--mb 256] [--device 0] [--reps 5] [--positions 130000000] [--no-host]
    python tools/bench_pileup.py --tools [--reads 100000] [--parent-exe PATH] [--dir /tmp/bm_pileup]

--positions is the number of reference positions in all, folded into 24 references of positions / 24 bases each; the state is
33 bytes a position.  ms_add and ms_finish are the HIP-event times of bmp_last_stats (bmc_last_stats for the coverage counter);
begin_ms is the wall time of bmp_begin on the grown context (it zeroes the counters, uploads the reference bases and waits); each
is the minimum over the repetitions after one warm-up.  Bytes: begin writes 33 per position, add reads the stream and issues one
32-bit atomic per base, the site pass reads 33 per position, the emit pass reads them again and writes 48 per site.

--tools measures the wall time of bucketmap_align on the `mini` workload of bench.py: -o x.bam --sort three times, the same with
--pileup three times, and -- where --parent-exe names a build of the commit before -- its --sort run three times, interleaved in
one session; best of three and the spread (max - min)."""
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
SEQ, QUAL = 51, 126                  # where a record's packed sequence and its qualities start
HBM_PEAK = 8.0e12                    # bytes per second, MI355X
CHUNK = 100_000                      # records handled at a time on the host


def kernels(a):
    from bench_bgzf import bam_stream
    from bucket_map_amd import depth, pileup

    n = (a.mb << 20) // RECORD
    data = bam_stream(a.mb << 20, False)[: n * RECORD].copy()
    rec = data.reshape(n, RECORD)
    ref_len = a.positions // N_REF
    pos = rec[:, 8:12].copy().view("<i4").reshape(n) % (ref_len - READ + 1)
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    ref = rec[:, 4:8].copy().view("<i4").reshape(n).astype(np.int64)
    # the reads say what the reference says, but for one base in a hundred
    rng = np.random.default_rng(20240021)
    genome = rng.integers(0, 4, N_REF * ref_len, dtype=np.uint8)         # 0 .. 3 for A C G T, the references back to back
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
    res = {"payload_bytes": int(data.size), "records": n, "references": N_REF, "positions": positions, "thresholds": pileup.DEFAULTS}

    c = pileup.Pileup(a.device)
    c.begin(lens, bases)
    c.add(data[: 1000 * RECORD], off[:1001])
    c.finish()
    t_begin, t_add, t_finish, call = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        c.begin(lens, bases)
        t1 = time.perf_counter()
        c.add(data, off)
        n_sites, stats = c.finish()
        call.append((time.perf_counter() - t0) * 1e3)
        t_begin.append((t1 - t0) * 1e3)
        t_add.append(c.ms_add)
        t_finish.append(c.ms_finish)
    sites = c.sites()
    some = c.counts_at(0, 0, min(ref_len, 100000))
    c.close()
    counted = int(stats[:, 3].sum() + stats[:, 4].sum())
    assert int(stats[:, 0].sum()) == n and counted == n * READ, "every record is counted with all its bases"
    res.update(sites=int(n_sites), n_lowq=int(stats[:, 4].sum()), begin_ms=round(min(t_begin), 3), ms_add=round(min(t_add), 3),
               ms_finish=round(min(t_finish), 3), call_ms=round(min(call), 2))
    res["atomic_adds"] = counted
    res["atomic_adds_per_ns"] = round(counted / (res["ms_add"] * 1e6), 2)
    res["add_stream_GBps"] = round(int(data.size) / res["ms_add"] / 1e6, 1)
    res["bytes_begin"], res["bytes_finish"] = 33 * positions, 66 * positions + 48 * int(n_sites)
    res["begin_share_of_hbm_peak"] = round(res["bytes_begin"] / (res["begin_ms"] * 1e-3) / HBM_PEAK, 3)
    res["finish_share_of_hbm_peak"] = round(res["bytes_finish"] / (res["ms_finish"] * 1e-3) / HBM_PEAK, 3)

    d = depth.Depth(a.device)                            # the coverage counter on the same stream, in the same session
    d.begin(lens)
    d.add(data[: 1000 * RECORD], off[:1001])
    d.finish()
    d_add, d_finish = [], []
    for _ in range(a.reps):
        d.begin(lens)
        d.add(data, off)
        d.finish()
        d_add.append(d.ms_add)
        d_finish.append(d.ms_finish)
    d.close()
    res["bmc_ms_add"], res["bmc_ms_finish"] = round(min(d_add), 3), round(min(d_finish), 3)
    res["add_over_bmc_add"] = round(res["ms_add"] / res["bmc_ms_add"], 1)
    res["finish_over_bmc_finish"] = round(res["ms_finish"] / res["bmc_ms_finish"], 1)

    if not a.no_host:
        which_of = np.full(16, 4, np.int64)
        which_of[[1, 2, 4, 8]] = [0, 1, 2, 3]
        t0 = time.perf_counter()
        cnt = np.zeros(positions * 8, np.uint32)
        for lo in range(0, n, CHUNK):
            hi = min(n, lo + CHUNK)
            packed = rec[lo:hi, SEQ:QUAL]
            code = np.stack([packed >> 4, packed & 15], axis=2).reshape(hi - lo, READ)
            q = rec[lo:hi, QUAL: QUAL + READ]
            which = np.where((q != 255) & (q < pileup.DEFAULTS["min_bq"]), 7, which_of[code])
            at = (ref[lo:hi] * ref_len + pos[lo:hi])[:, None] + np.arange(READ)
            np.add.at(cnt, (at * 8 + which).reshape(-1), 1)
        res["host_numpy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)   # the counters alone: no site pass
        assert np.array_equal(cnt[: some.size].reshape(-1, 8), some), "the host's counters are the device's"
        by_site = cnt.reshape(-1, 8)[sites[:, 0].astype(np.int64) * ref_len + sites[:, 1]]
        assert np.array_equal(by_site, sites[:, 3:11]), "the listed sites carry the host's counters"
        res["host_over_device"] = round(res["host_numpy_ms"] / (res["begin_ms"] + res["ms_add"] + res["ms_finish"]), 1)
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
    variants = {"sort": (exe, ["--sort"]), "sort_annotate": (exe, ["--sort", "--annotate"]), "sort_pileup": (exe, ["--pileup", "out.pileup"])}
    if a.parent_exe:
        variants["parent_sort"] = (os.path.abspath(a.parent_exe), ["--sort"])
    wall = {k: [] for k in variants}
    line = ""
    for rep in range(3):
        for name, (tool, extra) in variants.items():
            for f in ("out.bam", "out.bam.bai", "out.pileup"):
                if os.path.exists(os.path.join(a.dir, f)):
                    os.remove(os.path.join(a.dir, f))
            t0 = time.perf_counter()
            r = subprocess.run([tool, *common, "-q", "reads.fastq", "-o", "out.bam", *extra], cwd=a.dir, capture_output=True, text=True, timeout=300)
            wall[name].append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr[-2000:]
            line = next((l for l in r.stderr.splitlines() if "Pileup:" in l), line)
    res = {"workload": "mini", "reads": rd.n, "pileup_line": line.strip()}
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
    ap.add_argument("--dir", default="/tmp/bm_pileup")
    a = ap.parse_args()
    (tools if a.tools else kernels)(a)


if __name__ == "__main__":
    main()
