"""bench.py --dump-outputs without a GPU: dump_outputs on arrays shaped as bmf_batch_download returns them."""
import os

import numpy as np


def _batch(n, mc, nb, seed=1):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, mc + 1, (n, 2)).astype(np.uint32)
    buckets = rng.integers(0, 1 << 32, (n, 2, mc), dtype=np.uint64).astype(np.uint32)   # undefined past the counts
    valid = np.arange(mc)[None, None, :] < counts[:, :, None]
    buckets[valid] = rng.integers(0, nb, int(valid.sum()))
    return counts, buckets, valid


def _load(d):
    return [np.load(os.path.join(d, f"{name}.npy")) for name in ("windows", "counts", "buckets")]


def test_whole_batch_within_the_budget(tmp_path):
    import bench
    counts, buckets, valid = _batch(5000, 30, 70_000)
    size = bench.dump_outputs(str(tmp_path), counts, buckets, 70_000)
    w, c, b = _load(tmp_path)
    assert size == sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= bench.DUMP_BYTES
    assert (w.dtype, c.dtype, b.dtype) == (np.float64, np.float32, np.float32)
    assert np.array_equal(w, np.arange(5000)) and np.array_equal(c, counts)
    assert np.array_equal(b[valid], buckets[valid]) and (b[~valid] == -1).all()


def test_over_the_budget_a_fixed_sample(tmp_path):
    import bench
    counts, buckets, valid = _batch(5000, 30, 70_000)
    budget = 300 * (16 + 2 * 30 * 4) + 4096
    sizes = [bench.dump_outputs(str(tmp_path / d), counts, buckets, 70_000, budget=budget) for d in ("a", "b")]
    (wa, ca, ba), (wb, cb, bb) = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert max(sizes) <= budget and len(wa) == 300
    assert np.array_equal(wa, wb) and np.array_equal(ba, bb)                     # same windows on every run
    assert (np.diff(wa) > 0).all()
    idx = wa.astype(np.int64)
    assert np.array_equal(ca, counts[idx]) and np.array_equal(cb, counts[idx])
    assert np.array_equal(ba[valid[idx]], buckets[idx][valid[idx]]) and (ba[~valid[idx]] == -1).all()


def test_ids_past_float32_stay_exact(tmp_path):
    import bench
    nb = (1 << 24) + 5
    counts, buckets, valid = _batch(200, 30, nb)
    buckets[valid] = nb - 1 - (buckets[valid] & 1)                                # odd ids float32 would round
    bench.dump_outputs(str(tmp_path), counts, buckets, nb)
    _, _, b = _load(tmp_path)
    assert b.dtype == np.float64 and np.array_equal(b[valid], buckets[valid])
