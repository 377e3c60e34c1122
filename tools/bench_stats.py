#!/usr/bin/env python3
"""What the mapping statistics cost on the device: bmq_add with the default LDS window and with BMQ_LDS_CYCLES=0 (every cell by
global atomics) beside bmp_add on the same records in the same process, on two record sets.  Prints one JSON line.

    python tools/bench_stats.py [--records 1000000] [--long-records 20000] [--device 0] [--reps 5] [--positions 130000000] [--long-positions 2000000]

"short" is the record set of tools/bench_pileup.py (the BAM stream of synthetic 150-base reads, one 150= op each, 24 references,
about 1 % mismatches; the sequences as tools/bench_phase.py draws them); "long" is tools/bench_phase.py's 10 000-base reads with
an =/X CIGAR of 2 001 ops.

ms_add is the HIP-event time of bmq_last_stats (both kernels of every bmq_add), bmp_ms_add that of bmp_last_stats; each is the
minimum over the repetitions after one warm-up, the maximum beside it.  bmq's add reads every base, every quality and every op
and issues two LDS atomics (BC, QC) and one more per aligned base (MC); bmp's reads the same and issues one global atomic per
base."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bucket-map_amd", "python"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_phase import LONG_READ, LONG_X, long_records, short_records  # noqa: E402
from bench_pileup import READ, RECORD  # noqa: E402


def context(stats, device, window):
    """A bmq context made under BMQ_LDS_CYCLES=window (None: unset)."""
    before = os.environ.pop("BMQ_LDS_CYCLES", None)
    try:
        if window is not None:
            os.environ["BMQ_LDS_CYCLES"] = str(window)
        return stats.Stats(device)
    finally:
        os.environ.pop("BMQ_LDS_CYCLES", None)
        if before is not None:
            os.environ["BMQ_LDS_CYCLES"] = before


def measure(name, data, off, lens, genome, device, reps, max_cycle):
    from bucket_map_amd import pileup, stats
    n = int(off.size - 1)
    warm = min(n, 1000)
    res = {"payload_bytes": int(data.size), "records": n, "max_cycle": max_cycle}
    seen = []
    for key, window in (("lds", None), ("global", 0)):
        q = context(stats, device, window)
        q.begin(max_cycle=max_cycle)
        q.add(data[: int(off[warm])], off[: warm + 1])
        q.finish()
        times = []
        for _ in range(reps):
            q.begin(max_cycle=max_cycle)
            q.add(data, off)
            t = q.finish()
            times.append(q.ms_add)
        seen.append((t.tolist(), [q.table(k).tobytes() for k in range(stats.N_TABLES)]))
        q.close()
        res[f"ms_add_{key}"], res[f"ms_add_{key}_max"] = round(min(times), 3), round(max(times), 3)
    assert seen[0] == seen[1], "the window changes no output"
    t = seen[0][0]
    assert t[0] == n and t[31] == t[18], "every record and every quality counted"
    res.update(bases=int(t[18]), bases_eq=int(t[23]), bases_x=int(t[24]))
    bases = [np.frombuffer(b"ACGT", np.uint8)[genome[sum(lens[:r]): sum(lens[: r + 1])]] for r in range(len(lens))]
    p = pileup.Pileup(device)
    p.begin(lens, bases)
    p.add(data[: int(off[warm])], off[: warm + 1])
    p.finish()
    times = []
    for _ in range(reps):
        p.begin(lens, bases)
        p.add(data, off)
        p.finish()
        times.append(p.ms_add)
    p.close()
    res["bmp_ms_add"], res["bmp_ms_add_max"] = round(min(times), 3), round(max(times), 3)
    res["lds_over_global"] = round(res["ms_add_lds"] / res["ms_add_global"], 3)
    res["add_over_bmp_add"] = round(res["ms_add_lds"] / res["bmp_ms_add"], 3)
    res["bases_per_ns"] = round(res["bases"] / (res["ms_add_lds"] * 1e6), 2)
    return {name: res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--long-records", type=int, default=20_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--positions", type=int, default=130_000_000)
    ap.add_argument("--long-positions", type=int, default=2_000_000)
    a = ap.parse_args()
    long_size = 36 + 2 + 4 * (2 * LONG_X + 1) + LONG_READ // 2 + LONG_READ
    out = {}
    out.update(measure("short", *short_records((a.records * RECORD >> 20) + 1, a.positions), a.device, a.reps, 1024))
    assert out["short"]["bases"] == out["short"]["records"] * READ
    out.update(measure("long", *long_records((a.long_records * long_size >> 20) + 1, a.long_positions), a.device, a.reps, 16384))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
