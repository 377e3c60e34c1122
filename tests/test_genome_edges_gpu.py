"""The two kernels that read the genome itself -- bmi_presence_kernel (GPU index build) and bml_scan_kernel (locator
scan) -- where they can go wrong: buckets that start at any byte (they load aligned 16-byte chunks and address base j at
stream position (start & 15) + j), letters other than upper-case ACGT (dna4_pack4's byte-wise path), buckets that go
through LDS in overlapping segments, and degenerate views (empty, shorter than q, first / last byte of the buffer).

The index build is compared with brute_rows, a numpy restatement that takes arbitrary (start, length) views; two CPU
tests tie it to the host indexer and its letter table to the oracle's.  The scan is compared with the locator oracle.
Every comparison is exact.
"""
import numpy as np
import pytest

import test_locator as tl
from oracle import oracle_c as oc

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ the reference

def _rank_table():
    """host/bm_common.h::dna4_rank: C Y S B -> 1, G K -> 2, T U -> 3, either case, everything else 0."""
    t = np.zeros(256, np.uint8)
    for letters, r in ((b"CYSB", 1), (b"GK", 2), (b"TU", 3)):
        for c in letters + letters.lower():
            t[c] = r
    return t


RANK = _rank_table()


def qgram_hashes(flat, q):
    """Hash of the q-gram that starts at every byte of flat (first base in the high bits); len(flat) - q + 1 of them."""
    r = RANK[np.asarray(flat, np.uint8)].astype(np.int64)
    n = max(len(r) - q + 1, 0)
    h = np.zeros(n, np.int64)
    for t in range(q):
        h = h * 4 + r[t:t + n]
    return h


def brute_rows(flat, bstart, blen, k2i, nb, q):
    """The q-gram x bucket index in the .qgram layout (n_rows x ceil(nb/8) bytes, bucket b = bit b & 7 of byte b >> 3):
    bit b of row k2i[h] is set iff q-gram h starts somewhere in bucket b and FracMinHash kept it (k2i[h] >= 0)."""
    k2i = np.asarray(k2i, np.int64)
    h = qgram_hashes(flat, q)
    rows = np.zeros((int((k2i >= 0).sum()), (nb + 7) // 8), np.uint8)
    for b, (s, n) in enumerate(zip(np.asarray(bstart, np.int64), np.asarray(blen, np.int64))):
        if n < q:
            continue
        present = np.zeros(4 ** q, bool)
        present[h[s:s + n - q + 1]] = True
        idx = k2i[present]
        rows[idx[idx >= 0], b >> 3] |= np.uint8(1 << (b & 7))
    return rows


# ------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("kmer_frac", [1.0, 0.25])
def test_brute_rows_equal_the_host_indexer(kmer_frac):
    from bucket_map_amd import host
    bucket_len, read_len, q = 1024, 120, 7
    g = host.Genome.synth(20240001, [150_001, 9_003, 707, 41_005])
    nb = g.awk_bucket_num(bucket_len)
    index = host.Index(g, nb, bucket_len, read_len, q=q, kmer_frac=kmer_frac)
    flat, _ = g.flat()
    bstart, blen = g.bucket_views(bucket_len, read_len)
    assert len(set(int(s) % 16 for s in bstart)) == 4              # the odd record lengths really move the bucket starts
    k2i = index.kmer_to_index()
    assert ((k2i >= 0).sum() == 4 ** q) == (kmer_frac == 1.0)
    rows = brute_rows(flat, bstart, blen, k2i, nb, q)
    assert rows.shape == index.rows().shape and rows.any()
    assert np.array_equal(rows, index.rows())


def test_rank_table_equals_the_oracle():
    L = oc.lib()
    assert [int(L.bmo_dna4_rank(c)) for c in range(256)] == RANK.tolist()
    assert sorted(np.nonzero(RANK)[0].tolist()) == sorted(b"CYSBGKTUcysbgktu")


# ------------------------------------------------------------------------------------------ index build, GPU

def gpu_rows(flat, bstart, blen, k2i, nb, q, keep=False):
    """bmf_build_index over the views, and the rows it built (and the filter itself with keep)."""
    import bucket_map_amd as bma
    flt = bma.Filter(bma.Params(num_buckets=nb, q=q, k=q + 2, min_base_quality=25 * (q + 2), read_len=100))
    flt.build_index(flat, np.asarray(bstart, np.uint64), np.asarray(blen, np.uint32), k2i)
    rows = flt.index_download()
    if keep:
        return rows, flt
    flt.close()
    return rows


def assert_rows(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size:
        r = int(bad[0])
        bits = np.nonzero(np.unpackbits(got[r] ^ want[r], bitorder="little"))[0]
        raise AssertionError(f"{what}: {bad.size} of {len(want)} rows differ; row {r} differs at buckets {bits[:8].tolist()}")


def letters(rng, n):
    return tl.LETTERS[rng.integers(0, 4, n)]


@gpu
@pytest.mark.parametrize("q", [3, 7, 10])
def test_build_at_every_shift_and_every_short_length(q):
    from bucket_map_amd import host
    rng = np.random.default_rng(100 + q)
    n = 40_003                                                     # the last byte is not the last of a 16-byte chunk
    flat = letters(rng, n)
    lengths = (0, q - 1, q, q + 1, 15, 16, 17, 31, 33)
    views = [(0, 777)]                                             # the buffer's first byte
    for s in range(16):
        for length in lengths + (1000 + s,):
            views.append((16 * int(rng.integers(0, (n - length) // 16 - 1)) + s, length))
    ends = [(n - 300 - 16 * s) // 16 * 16 + s for s in range(16)]  # ... and its last
    views += [(start, n - start) for start in ends] + [(n, 0)]     # (and an empty view at the very end)
    bstart, blen = np.array(views, np.int64).T
    assert all(sorted(bstart[blen == length] % 16) == list(range(16)) for length in lengths if length)
    assert [e % 16 for e in ends] == list(range(16)) and (bstart + blen <= n).all() and (bstart >= 0).all()
    nb = len(views) + 3                                            # padding bits past the kept buckets: zero
    k2i = host.select_qgrams(q, 0.25) if q == 7 else host.select_qgrams(q)
    assert (k2i >= 0).all() == (q != 7)
    want = brute_rows(flat, bstart, blen, k2i, nb, q)
    assert want.any() and not np.unpackbits(want, axis=1, bitorder="little")[:, len(views):].any()
    assert_rows(gpu_rows(flat, bstart, blen, k2i, nb, q), want, f"q={q}")


def every_byte_buffer(rng):
    """Every byte value at every position of a 4-byte word whose other bytes are plain A/C/G/T (either case), every
    position of a 16-byte chunk hit, then runs of N longer than a chunk at odd places, plain letters in between."""
    plain = np.frombuffer(b"ACGTacgt", np.uint8)
    words = plain[rng.integers(0, 8, (1024, 4))]
    odd_at = np.zeros(len(words) * 4, bool)
    for v in range(256):
        for slot in range(4):
            p = (slot + v) % 4                                     # word v * 4 + slot sits at bytes 4 * slot .. of its chunk
            words[v * 4 + slot, p] = v
            odd_at[(v * 4 + slot) * 4 + p] = True
    parts = [words.ravel(), plain[rng.integers(0, 8, 37)], np.full(40, ord("N"), np.uint8), plain[rng.integers(0, 8, 3)],
             np.full(17, ord("n"), np.uint8), plain[rng.integers(0, 8, 50)], np.frombuffer(b"N" * 33 + b"-", np.uint8),
             plain[rng.integers(0, 8, 300)]]
    return np.concatenate(parts), odd_at


@gpu
def test_build_with_every_byte_value():
    from bucket_map_amd import host
    q = 5
    flat, odd_at = every_byte_buffer(np.random.default_rng(55))
    # the buffer is what the docstring says
    at = np.nonzero(odd_at)[0]
    assert sorted(set(zip(flat[at].tolist(), (at % 4).tolist()))) == [(v, p) for v in range(256) for p in range(4)]
    for v in (0x00, 0x40, 0x5B, 0x60, 0x7B, 0x80, 0xC3, 0xE3, 0xFF, ord("N"), ord("U"), ord("y")):
        assert sorted(set(at[flat[at] == v] % 4)) == [0, 1, 2, 3]
    assert sorted(set(at % 16)) == list(range(16))
    plain = np.isin(flat, np.frombuffer(b"ACGTacgt", np.uint8))
    assert all(plain[w * 4: w * 4 + 4].sum() >= 3 for w in range(1024))
    bstart = np.arange(0, len(flat) - 300, 97)                     # 97 = 6 * 16 + 1: every shift in turn
    bstart = np.concatenate([bstart, [len(flat) - 300]])
    blen = np.full(len(bstart), 300)
    assert set(bstart % 16) == set(range(16)) and bstart[-1] + 300 == len(flat)
    nb = len(bstart) + 3
    k2i = host.select_qgrams(q)
    want = brute_rows(flat, bstart, blen, k2i, nb, q)
    got = gpu_rows(flat, bstart, blen, k2i, nb, q)
    assert_rows(got, want, "every byte value")
    respelled = tl.LETTERS[RANK[flat]]                             # the same ranks in plain upper-case letters
    assert (respelled != flat).sum() > 2000
    assert_rows(gpu_rows(respelled, bstart, blen, k2i, nb, q), got, "respelled")


def segment_capacity(q):
    """bmf_build_index: bases of a bucket that fit in 159 KiB of LDS beside the 4^q-bit presence bitmap, at most 2^20:
    126 912 at q = 10, 520 128 at q = 9, 643 008 at q = 7 (the LDS binds at every q; 2^20 never does).  Restated only to
    aim at the seams: the test below holds whatever the budget is."""
    room = 159 * 1024 - 4 ** q // 8
    return min((room // 4 - 4) * 16, 1 << 20)


@gpu
@pytest.mark.parametrize("q,n,far,more", [(10, 400_000, 300_000, ()), (9, 1_200_000, 700_000, ()),
                                          (7, 2_200_000, 1_500_000, (((1 << 20) - 1, 15), (1 << 20, 1), ((1 << 20) + 1, 8)))])
def test_build_buckets_that_go_through_lds_in_segments(q, n, far, more):
    """Lengths around one and two full segments (segments overlap by q - 1) and one far from any seam, each at shifts
    0, 1, 8, 15 (at q = 7 lengths around 2^20, the cap on a segment whatever the LDS, too), and a 50-base bucket in the
    same launch.  In every bucket longer than a segment, the q - 1 q-grams that straddle the first seam occur nowhere
    else in the bucket: a seam that loses one clears exactly their bits."""
    from bucket_map_amd import host
    rng = np.random.default_rng(q)
    cap = segment_capacity(q)
    # random bases without "TT"; a planted TT then marks q-grams that nothing else in the buffer can equal
    codes = rng.integers(0, 4, n).astype(np.uint8)
    again = np.nonzero((codes[1:] == 3) & (codes[:-1] == 3))[0] + 1
    codes[again] = rng.integers(0, 3, len(again))
    assert not ((codes[1:] == 3) & (codes[:-1] == 3)).any() and (codes == 3).mean() > 0.15
    views = [(500, 50)]
    cases = [(ln, s) for ln in (cap - 1, cap, cap + 1, 2 * cap - (q - 1), 2 * cap - (q - 1) + 1, far) for s in (0, 1, 8, 15)]
    for i, (length, shift) in enumerate(cases + list(more)):
        views.append((1024 * (i + 1) + shift, length))
    bstart, blen = np.array(views, np.int64).T
    assert (bstart + blen <= n).all() and far % cap > 1000 and cap - far % cap > 1000
    # the plants: at bucket offsets cap - 1 and cap, TT between flanks that spell the bucket's number in base 3 (lowest
    # digit next to the TT on both sides, no T): the q-grams around two plants differ wherever the TT sits in them
    d = q - 2
    seams = [b for b in range(len(views)) if blen[b] > cap]
    for b in seams:
        digits = np.array([b // 3 ** t % 3 for t in range(d)], np.uint8)
        at = int(bstart[b]) + cap - 1
        codes[at - d: at] = digits[::-1]
        codes[at: at + 2] = 3
        codes[at + 2: at + 2 + d] = digits
    flat = tl.LETTERS[codes]
    h = qgram_hashes(flat, q)
    planted = []                                                   # (bucket, q-gram): it starts before the seam and ends after it
    for b in seams:
        mine = h[bstart[b]: bstart[b] + blen[b] - q + 1]
        for j in range(cap - q + 1, min(cap, int(blen[b]) - q + 1)):
            assert (mine == mine[j]).sum() == 1, (b, j)
            planted.append((b, int(mine[j])))
    assert len(planted) == 4 * (1 + 3 * (q - 1)) + len(more) * (q - 1)   # cap + 1 has one such q-gram, the longer ones all
    nb = len(views) + 3
    k2i = host.select_qgrams(q)
    got = gpu_rows(flat, bstart, blen, k2i, nb, q)
    lost = [(b, g) for b, g in planted if not (got[k2i[g], b >> 3] >> (b & 7)) & 1]
    assert not lost, f"q-grams across the first seam are missing: (bucket, q-gram) {lost[:6]}"
    assert_rows(got, brute_rows(flat, bstart, blen, k2i, nb, q), f"q={q}")


@gpu
def test_build_fewer_buckets_than_nb():
    from bucket_map_amd import host
    q, nb = 7, 200
    rng = np.random.default_rng(5)
    flat = letters(rng, 9_001)
    bstart, blen = np.array([3, 1500, 2999, 4242, 7000]), np.array([1400, 1501, 777, 2000, 2001])
    k2i = host.select_qgrams(q)
    want = brute_rows(flat, bstart, blen, k2i, nb, q)
    assert want[:, 0].any() and not want[:, 1:].any()
    rows, flt = gpu_rows(flat, bstart, blen, k2i, nb, q, keep=True)
    assert_rows(rows, want, "5 buckets, NB = 200")
    assert np.array_equal(flt.zeros(), nb - np.unpackbits(want, axis=1).sum(axis=1))
    flt.close()


@gpu
def test_build_no_buckets_at_all():
    from bucket_map_amd import host
    q, nb = 7, 200
    rng = np.random.default_rng(6)
    flat = letters(rng, 5_000)
    k2i = host.select_qgrams(q)
    rows, flt = gpu_rows(flat, np.zeros(0, np.uint64), np.zeros(0, np.uint32), k2i, nb, q, keep=True)
    assert rows.shape == (4 ** q, nb // 8) and not rows.any()
    assert (flt.zeros() == nb).all()
    # ... and the filter answers: no bucket holds anything, so no read has a candidate
    n_reads, read_len = 8, 100
    ws = np.arange(n_reads, dtype=np.uint64) * read_len
    wl = np.full(n_reads, read_len, np.uint32)
    counts, _ = flt.map_windows(flat[: n_reads * read_len], np.full(n_reads * read_len, ord("I"), np.uint8), ws, wl)
    assert counts.shape == (n_reads, 2) and not counts.any()
    flt.close()


# ------------------------------------------------------------------------------------------ locator scan, GPU

def assert_scan(case, want, what, **how):
    o_got, v_got, st = tl.gpu_scan(case, **how)
    bad = np.nonzero((want[0] != o_got) | (want[1] != v_got))[0]
    assert bad.size == 0, (f"{what}: {bad.size} candidates differ, first {bad[:5]}: ref {want[0][bad[:5]]}/{want[1][bad[:5]]} "
                           f"got {o_got[bad[:5]]}/{v_got[bad[:5]]}")
    return st


SMALL = dict(n_buckets=3, bucket_len=2048, read_len=100, n_reads=60, k=12, p=10)


@gpu
def test_scan_at_every_shift():
    for lead in range(1, 16):
        case = tl.make_case(np.random.default_rng(300 + lead), lead=lead, **SMALL)
        assert [int(s) % 16 for s in case["bstart"]] == [lead] * 3
        want = tl.oracle(case)
        assert (want[0] >= 0).sum() >= 50                          # the reads are found: the comparison is not of -1s
        assert_scan(case, want, f"lead={lead}")


@gpu
def test_scan_at_every_shift_in_repeats():
    for lead in range(1, 16):
        case = tl.make_case(np.random.default_rng(400 + lead), lead=lead, motif=53, **SMALL)
        want = tl.oracle(case)
        assert (want[0] >= 0).sum() >= 50
        st = assert_scan(case, want, f"lead={lead}, motif")
        assert st["heavy_candidates"] > 0 and st["occurrences"] > 20 * len(case["pb"])


@gpu
@pytest.mark.parametrize("k,p", [(16, 10), (6, 5)])
def test_scan_tight_fit(k, p):
    """Every bucket has exactly max_bucket_bases bases (a multiple of 16: the stream then takes one word more than the
    bucket alone) and starts at shift 15; the last one ends at the buffer's last byte; k = 16 shifts the two-word
    extraction by its extremes."""
    case = tl.make_case(np.random.default_rng(500 + k), n_buckets=3, bucket_len=2048, read_len=96, n_reads=80, k=k, p=p, lead=15)
    assert case["blen"].tolist() == [2144] * 3 and [int(s) % 16 for s in case["bstart"]] == [15] * 3
    assert int(case["bstart"][-1]) + 2144 == len(case["genome"])
    want = tl.oracle(case)
    assert (want[0] >= 0).sum() >= 40
    assert_scan(case, want, f"k={k}")
    # reads that end at the last bucket's (and the buffer's) last base are found there
    text, n = case["genome"], len(case["genome"])
    hs = oc.kmer_hashes(text[n - 96:], k)
    pos = [int(i) for i in oc.sample_positions(p, len(hs) - 1)]
    from bucket_map_amd import locate
    s = locate.LocatorScan(k, p, 0, 0, 2144)
    s.load_genome(text, case["bstart"], case["blen"])
    off, votes = s.locate([[int(hs[j]) for j in pos]], [pos], [96], [2], [0], [0])
    s.close()
    o_ref, v_ref = oc.locate(k, p, 0, 0, text, case["bstart"], case["blen"], [[int(hs[j]) for j in pos]], [pos], [96], [2], [0], [0])
    assert (int(off[0]), int(votes[0])) == (int(o_ref[0]), int(v_ref[0]))
    if k == 16:
        assert (int(off[0]), int(votes[0])) == (2144 - 96, p)


@gpu
@pytest.mark.parametrize("motif", [None, 53])
def test_scan_of_a_respelled_genome(motif):
    """IUPAC letters, lower case, U, N and '-' in the genome: the scan folds them like the oracle (and the host) do, so
    offsets and votes are those of the plain genome -- uploaded as one string or as records cut at odd places."""
    from bucket_map_amd import locate
    plain = tl.make_case(np.random.default_rng(600), lead=5, motif=motif, **SMALL)
    case = tl.make_case(np.random.default_rng(600), lead=5, motif=motif, spelling=np.random.default_rng(601), **SMALL)
    assert np.array_equal(RANK[case["genome"]], RANK[plain["genome"]]) and len(set(case["genome"].tolist())) == 35
    for name in ("sh", "sp", "pb", "pw", "pr", "bstart", "blen"):
        assert np.array_equal(case[name], plain[name]), name
    want = tl.oracle(plain)
    got = tl.oracle(case)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and (want[0] >= 0).sum() >= 50
    assert_scan(case, want, "respelled, one string")
    records = np.split(case["genome"], [1, 1, 18, 2053, 2054, 4099, 6000])     # an empty one among them
    s = locate.LocatorScan(case["k"], case["p"], 4, 6, int(case["blen"].max()))
    s.load_genome_records(records, case["bstart"], case["blen"])
    off, votes = s.locate(case["sh"], case["sp"], case["sl"], case["pb"], case["pw"], case["pr"])
    s.close()
    assert np.array_equal(want[0], off) and np.array_equal(want[1], votes)
