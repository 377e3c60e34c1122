"""The affine-gap realignment pass on the GPU (bmv_realign, include/bmv.h): score, begin, the realigned flag and the CIGAR
for what bmv_align returns over a grid of query lengths, strands, bands and scores, for hand-planted CIGARs at the band's
borders, for one long alignment whose batch is taken in pieces, and for a batch that mixes realigned, passed-through and empty
alignments; what the call leaves untouched; that bmv_annotate and bmv_clip take its output; the refusals; and
`bucketmap_align --affine` against the oracle-backed tool, byte for byte.

Expected values come from test_realign.restate_realign, the plain-Python restatement held against a second formulation and
hand-worked cases there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_annotate import D, EQ, I, M, X, pack
from test_annotate_gpu import _Batch, _plant, _planted_specs, _revcomp, _unpack, _verifier, genome  # noqa: F401  (a fixture)
from test_realign import ARGS, DEFAULT, TOOLS, indel_job, path_score, restate_realign  # noqa: F401  (a fixture)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 300, 1000)
BASES = np.frombuffer(b"ACGT", np.uint8)


def _packed(cigars):
    off = np.concatenate([[0], np.cumsum([len(c) for c in cigars])]).astype(np.uint64)
    cg = np.concatenate([pack(c) for c in cigars] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return off, cg


def _views(genome, batch, a):
    reads, ts, tl, trc, qs, ql = batch
    return (bytes(genome[int(ts[a]): int(ts[a]) + int(tl[a])]), int(trc[a]), bytes(reads[int(qs[a]): int(qs[a]) + int(ql[a])]))


def _assert_realigned(got, genome, batch, begins, cigars, scores, band, what):
    """got: Verifier.realign's dict.  Every output of every alignment is the restatement's, and the contract's invariants
    hold.  Returns the restatement's dicts."""
    n = len(cigars)
    off = got["cigar_offset"]
    assert len(got["score"]) == len(got["begin"]) == len(got["realigned"]) == n and len(off) == n + 1
    assert off[0] == 0 and off[n] == len(got["cigar"]), f"{what}: the total is not the offsets' end"
    want = []
    for a in range(n):
        window, rc, query = _views(genome, batch, a)
        w = restate_realign(window, rc, query, int(begins[a]), cigars[a], scores, band)
        ops = _unpack(got["cigar"][int(off[a]): int(off[a + 1])])
        g = dict(score=int(got["score"][a]), begin=int(got["begin"][a]), realigned=int(got["realigned"][a]), cigar=ops)
        assert g == w, f"{what}: alignment {a} (m = {len(query)}, rc = {rc}, given {cigars[a]}) differs from the restatement"
        assert not cigars[a] or g["score"] >= path_score(window, rc, query, int(begins[a]), cigars[a], scores), f"{what}: {a}"
        if ops:
            assert sum(k for op, k in ops if op != D) == len(query), f"{what}: alignment {a} loses query bases"
            assert all(x[0] != y[0] for x, y in zip(ops, ops[1:])), f"{what}: alignment {a} has adjacent entries of one op"
        assert g["begin"] + sum(k for op, k in ops if op != I) <= len(window), f"{what}: alignment {a} leaves its window"
        want.append(w)
    return want


def _edited(rng, src, longest_del):
    """src with planted edits at least 12 bases apart, at most one per 10 bases: substitutions, insertions of 1-3 bases,
    deletions of 1 .. longest_del bases."""
    out, at, budget = [], 0, len(src) // 10
    while at < len(src):
        step = int(rng.integers(12, 40))
        out.append(src[at: at + step])
        at += step
        if at >= len(src) or budget <= 0:
            continue
        kind = int(rng.integers(0, 3))
        size = 1 if kind == 0 else int(rng.integers(1, 4)) if kind == 1 else int(rng.integers(1, longest_del + 1))
        size = min(size, budget)
        budget -= size
        if kind == 0:
            out.append(BASES[(np.searchsorted(BASES, src[at: at + 1]) + 1) % 4])
            at += 1
        elif kind == 1:
            out.append(BASES[rng.integers(0, 4, size)])
        else:
            at += size
    return np.concatenate(out).astype(np.uint8)


def _grid_batch(rng, plain, band):
    """Two reads of every length on either strand with <= 10 % planted edits (deletions of at most min(8, the band's cap)
    bases), then three alignments with a hand-planted D entry one base over the cap."""
    cap = 63 - 2 * band
    b = _Batch()
    for m in LENGTHS:
        for rc in (0, 1):
            for _ in range(2):
                start = int(rng.integers(0, len(plain) - 2 * m - 64))
                q = _edited(rng, plain[start + 6: start + 6 + m + m // 8 + 8], min(8, cap))[:m]
                b.add(_revcomp(q) if rc else q, start, m + m // 8 + 20, rc)
    return b, cap


@pytest.fixture(scope="module")
def plain():
    return np.random.default_rng(20250901).choice(list(b"ACGT"), 300_000).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("scores", [DEFAULT, (3, 2, 5, 3)], ids=["1-4-6-1", "3-2-5-3"])
@pytest.mark.parametrize("band", [1, 8, 16, 31])
def test_after_the_aligner(plain, band, scores):
    """The grid of lengths and strands: bmv_align's CIGARs realigned.  The pass-through count is the number of deliberately
    planted over-long D entries: an unexpected pass-through fails the test."""
    rng = np.random.default_rng(100 + band)
    b, cap = _grid_batch(rng, plain, band)
    n_sim = len(b.ts)
    planted = []
    for rc in (0, 1, 0):
        planted.append(_plant(rng, plain, b, [(EQ, 20), (D, cap + 1), (EQ, 25)], rc, exact=True))
    batch = b.args()
    v = _verifier()
    v.load_genome(plain)
    score, begin, off, cg = v.align(*batch)
    begins = [int(x) for x in begin]
    cigars = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in range(len(begins))]
    assert (score[:n_sim] < 0).sum() > n_sim // 3 and {M, I, D} <= {op for c in cigars[:n_sim] for op, _ in c}
    for k, (bg, c) in enumerate(planted):
        begins[n_sim + k], cigars[n_sim + k] = bg, c
    o2, c2 = _packed(cigars)
    got = v.realign(*batch, begins, o2, c2, *scores, band)
    st = v.realign_stats()
    v.close()
    assert st["n_passed_through"] == len(planted) == int((got["realigned"] == 0).sum()), "an unexpected pass-through"
    assert st["ms_kernels"] > 0 and st["cells"] == 64 * int(batch[5][:n_sim].sum())
    want = _assert_realigned(got, plain, batch, begins, cigars, scores, band, f"band {band}, scores {scores}")
    assert [w["realigned"] for w in want[n_sim:]] == [0, 0, 0]
    assert any(w["cigar"] != c for w, c in zip(want[:n_sim], cigars)), "no path changed: the grid shows little"


def _border_batch(rng, genome, band):
    cap = 63 - 2 * band
    b, begins, cigars = _Batch(), [], []

    def plant(spec, rc, **kw):
        bg, cg = _plant(rng, genome, b, spec, rc, **kw)
        begins.append(bg)
        cigars.append(cg)

    def empty(qlen):
        b.add(rng.choice(list(b"ACGT"), qlen).astype(np.uint8), int(rng.integers(0, 100_000)), 40, int(rng.integers(0, 2)))
        begins.append(int(rng.integers(0, 5)))
        cigars.append([])

    specs = [
        [(EQ, 40), (X, 1), (EQ, 40)],
        [(I, 3), (EQ, 30)], [(EQ, 30), (I, 3)],                              # row shift 0 at either end
        [(EQ, 30), (I, band + 5), (EQ, 30)],                                 # an I run longer than the band
        [(EQ, 30), (D, cap), (EQ, 30)], [(EQ, 30), (D, cap + 1), (EQ, 30)],  # a D entry at the cap and one over it
        [(EQ, 5), (D, 1), (EQ, 2), (D, 2), (EQ, 1), (D, 1), (X, 1), (D, 2), (EQ, 40)],   # row shifts 1 + L, close together
        [(D, 3), (EQ, 20), (D, 3)], [(D, min(5, cap))], [(D, 2), (I, 2), (EQ, 20)], [(EQ, 20), (I, 2), (D, 2), (EQ, 20)],
        [(I, 70)], [(EQ, 1)], [(X, 1)], [(I, 1)],
        [(EQ, 64), (I, 1), (EQ, 64), (D, 1), (EQ, 64)], [(EQ, 63), (D, 2), (EQ, 65), (I, 2), (EQ, 130)],
    ]
    for spec in specs:
        for rc in (0, 1):
            plant(spec, rc)
            plant(spec, rc, begin=0, end_slack=0)                            # begin < w and begin + R > n - w
    for spec in _planted_specs(rng):
        plant(spec, int(rng.integers(0, 2)))
    empty(30)
    for rc in (0, 1):
        plant([(EQ, 100), (X, 1)], rc, start=len(genome) - 120, begin=19, end_slack=0)       # the genome's last base
        plant([(EQ, 5), (X, 10), (D, 10), (EQ, 5)], rc, start=49_990, begin=5, end_slack=5)   # the stretch of N
        empty(0)
    return b, begins, cigars


@pytest.mark.gpu
@pytest.mark.parametrize("band", [16, 3])
def test_planted_cigars_at_the_borders(genome, band):
    """Hand-planted, deliberately poor paths on both strands over a genome with N, IUPAC letters and lower case (the queries
    spell their ranks with such letters too): the band cut at either end of the text, row shifts of 0, 1 and 1 + L, an I run
    longer than the band, D entries at the cap and over it, empty CIGARs in between -- one batch that mixes realigned,
    passed-through and empty alignments."""
    rng = np.random.default_rng(200 + band)
    b, begins, cigars = _border_batch(rng, genome, band)
    batch = b.args()
    off, cg = _packed(cigars)
    v = _verifier()
    v.load_genome(genome)
    got = v.realign(*batch, begins, off, cg, band=band)
    want = _assert_realigned(got, genome, batch, begins, cigars, DEFAULT, band, f"borders, band {band}")
    over = sum(1 for c in cigars if not c or any(op == D and k > 63 - 2 * band for op, k in c))
    assert v.realign_stats()["n_passed_through"] == over and 0 < over < len(cigars) - 40
    assert sum(1 for c in cigars if not c) == 3 and any(w["begin"] != bg for w, bg in zip(want, begins))
    # a share of the batch, with offsets that do not start at 0
    part = slice(30, 90)
    share = tuple(x[part] for x in batch)[1:]
    again = v.realign(batch[0], *share, begins[part], off[30:91], cg, band=band)
    v.close()
    _assert_realigned(again, genome, (batch[0], *share), begins[part], cigars[part], DEFAULT, band, "a share of the batch")


@pytest.mark.gpu
def test_a_long_alignment_in_pieces(plain, monkeypatch, capfd):
    """One alignment of 20 000 rows after a short one and before one of 10 000 rows with the scratch forced down to 2 MB: its
    direction codes and entries take 1.44 MB, the last one's 0.72 MB, so the batch is taken in two pieces; under 1 MB the call
    refuses the long one by name before anything runs.  (The CIGARs come from a context with the default scratch.)"""
    from bucket_map_amd import verify
    rng = np.random.default_rng(300)
    b = _Batch()
    for m in (300, 20_000, 10_000):
        start = int(rng.integers(0, len(plain) - 2 * m - 64))
        b.add(_edited(rng, plain[start + 6: start + 6 + m + m // 8 + 8], 8)[:m], start, m + m // 8 + 20, 0)
    batch = b.args()
    v = _verifier()
    v.load_genome(plain)
    score, begin, off, cg = v.align(*batch)
    v.close()
    monkeypatch.setenv("BMV_SCRATCH_MB", "2")
    monkeypatch.setenv("BMV_LOG_CLASSES", "1")
    v = _verifier()
    v.load_genome(plain)
    cigars = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in range(3)]
    capfd.readouterr()
    got = v.realign(*batch, begin, off, cg)
    log = capfd.readouterr().err
    v.close()
    assert "[bmv] realign: 3 alignments (0 passed through) in 2 pieces" in log, log
    _assert_realigned(got, plain, batch, begin, cigars, DEFAULT, 16, "in pieces")
    monkeypatch.setenv("BMV_SCRATCH_MB", "1")
    v = _verifier()
    v.load_genome(plain)
    with pytest.raises(verify.BmvError) as e:
        v.realign(*batch, begin, off, cg)
    assert e.value.code == 5 and "alignment 1" in str(e.value) and "BMV_SCRATCH_MB" in str(e.value)
    short = tuple(x[:1] for x in batch[1:])
    one = v.realign(batch[0], *short, begin[:1], off[:2], cg)                # the context stays usable
    v.close()
    _assert_realigned(one, plain, (batch[0], *short), begin[:1], cigars[:1], DEFAULT, 16, "after the refusal")


def _snapshot(v, n, n_cigar, n_x, n_r, n_cx, n_cr):
    """What bmv_results, bmv_annotations and bmv_clipped return, read through the ABI."""
    from bucket_map_amd import verify
    L = verify.lib()
    u32, u64 = (lambda k: np.zeros(max(k, 1), np.uint32)), (lambda k: np.zeros(max(k, 1), np.uint64))
    res = [np.zeros(n, np.int32), u32(n), u64(n + 1), u32(n_cigar)]
    ann = [u32(n), u32(n), u32(n), u64(n + 1), u32(n_x), u64(n + 1), np.zeros(max(n_r, 1), np.uint8)]
    cl = [np.zeros(n, np.int64), u32(n), u32(n), u32(n), u32(n), u32(n), u64(n + 1), u32(n_cx), u64(n + 1), np.zeros(max(n_cr, 1), np.uint8)]
    for name, arrs in (("bmv_results", res), ("bmv_annotations", ann), ("bmv_clipped", cl)):
        types = verify.SYMBOLS[name][1][1:]
        assert getattr(L, name)(v._h, *(x.ctypes.data_as(t) for x, t in zip(arrs, types))) == 0
    return [x.copy() for x in res + ann + cl] + [v.stats(), v.annotate_stats(), v.clip_stats()]


@pytest.mark.gpu
def test_other_results_stay_and_the_output_feeds_annotate_and_clip(plain):
    from test_annotate_gpu import _assert_annotations
    from test_annotate_gpu import _expected as expected_annotations
    from test_clip_gpu import _assert_clipped
    from test_clip_gpu import _expected as expected_clipped
    rng = np.random.default_rng(400)
    b, _ = _grid_batch(rng, plain, 16)
    batch = b.args()
    n = len(b.ts)
    v = _verifier()
    v.load_genome(plain)
    score, begin, off, cg = v.align(*batch)
    ann = v.annotate(*batch, begin, off, cg)
    cl = v.clip(*batch, begin, off, cg)
    sizes = (n, len(cg), len(ann[4]), len(ann[6]), len(cl["xcigar"]), len(cl["ref_bases"]))
    before = _snapshot(v, *sizes)
    got = v.realign(*batch, begin, off, cg)
    after = _snapshot(v, *sizes)
    assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(before, after)), \
        "bmv_realign changed what another result or stats call returns"
    assert got["realigned"].all() and (got["score"].astype(np.int64) <= batch[5].astype(np.int64)).all()
    # its output is bmv_results' shape: straight into the two other post-passes
    ann2 = v.annotate(*batch, got["begin"], got["cigar_offset"], got["cigar"])
    _assert_annotations(ann2, expected_annotations(plain, batch, got["begin"], got["cigar_offset"], got["cigar"]), "annotate after realign")
    cl2 = v.clip(*batch, got["begin"], got["cigar_offset"], got["cigar"])
    v.close()
    _assert_clipped(cl2, expected_clipped(plain, batch, got["begin"], got["cigar_offset"], got["cigar"], 1, 2), batch, "clip after realign")
    # the affine score is that of the annotated columns
    for a in range(n):
        xc = _unpack(ann2[4][int(ann2[3][a]): int(ann2[3][a + 1])])
        s = sum(k if op == EQ else -4 * k if op == X else -6 - k for op, k in xc)
        assert s == int(got["score"][a]), a


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(plain):
    from bucket_map_amd import verify
    rng = np.random.default_rng(500)
    b = _Batch()
    for _ in range(3):
        start = int(rng.integers(0, 100_000))
        b.add(_edited(rng, plain[start + 6: start + 400], 8)[:300], start, 320, 0)
    batch = b.args()
    with pytest.raises(verify.BmvError) as e:
        verify.Verifier().realign(*batch, np.zeros(3, np.uint32), np.zeros(4, np.uint64), np.zeros(0, np.uint32))
    assert e.value.code == 3                                     # BMV_ERR_STATE: no genome yet
    v = _verifier()
    v.load_genome(plain)
    score, begin, off, cg = v.align(*batch)
    cigars = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in range(3)]
    good = v.realign(*batch, begin, off, cg)
    for kw in (dict(match=0), dict(match=1025), dict(mismatch=0), dict(gap_open=0), dict(gap_open=1025), dict(gap_extend=0),
               dict(gap_extend=1025), dict(band=0), dict(band=32)):
        with pytest.raises(verify.BmvError) as e:
            v.realign(*batch, begin, off, cg, **kw)
        assert e.value.code == 1 and "bmv_realign" in str(e.value), kw
    bad_cigars = {
        "consumes query_len - 1": [(M, 299)],
        "runs past the window": [(M, 300), (D, 21)],
        "a zero-length entry": [(M, 150), (I, 0), (M, 150)],
        "adjacent equal ops": [(M, 150), (M, 150)],
        "an op code of 3": [(M, 150), (3, 2), (M, 150)],
    }
    for what, bad in bad_cigars.items():
        o, c = _packed(cigars[:2] + [bad])
        with pytest.raises(verify.BmvError) as e:
            v.realign(*batch, [begin[0], begin[1], 0], o, c)
        assert e.value.code == 1 and "alignment 2" in str(e.value), (what, str(e.value))
    again = v.realign(*batch, begin, off, cg)
    assert all(np.array_equal(good[k], again[k]) for k in good), "a refusal changed what the next call returns"
    _assert_realigned(again, plain, batch, begin, cigars, DEFAULT, 16, "after the refusals")
    empty = v.realign(np.zeros(0, np.uint8), [], [], [], [], [], [], [0], [])                # n == 0 is fine
    assert empty["cigar_offset"].tolist() == [0] and len(empty["score"]) == 0
    v.close()
    # scores that leave 32 bits: (10 + 1 048 576) x 1024 + 6 >= 2^30
    big = np.full(1_100_000, ord("A"), np.uint8)
    v = _verifier()
    v.load_genome(big)
    args = (np.full(20, ord("A"), np.uint8), [0, 0], [64, 1_048_576], [0, 0], [0, 10], [10, 10], [0, 0], [0, 1, 2], pack([(M, 10), (M, 10)]))
    with pytest.raises(verify.BmvError) as e:
        v.realign(*args, match=1024)
    assert e.value.code == 5 and "alignment 1" in str(e.value)
    ok = v.realign(*args)
    v.close()
    assert ok["score"].tolist() == [10, 10] and ok["realigned"].tolist() == [1, 1]


def _run(exe, d, out, *extra):
    env = dict(os.environ, BM_VERIFY_BLOCK_READS="37")
    r = subprocess.run([exe, *ARGS, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@pytest.mark.gpu
def test_the_tool_against_the_oracle_backed_tool(indel_job):
    """bucketmap_align --affine writes, byte for byte, what the oracle-backed tool writes through the host restatement
    (host/affine_realign.h) -- alone, under --best with other scores and a narrow band, and from two contexts."""
    d = indel_job
    gpu = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    for k, extra in enumerate((["--affine"], ["--best", "--affine-scores", "2,3,5,2", "--affine-band", "4"])):
        _run(TOOLS["bucketmap_align"], d, f"cpu{k}.sam", *extra)
        err = _run(gpu, d, f"gpu{k}.sam", *extra)
        assert "GPU affine realignment" in err
        assert (d / f"gpu{k}.sam").read_bytes() == (d / f"cpu{k}.sam").read_bytes(), extra
        assert b"AS:i:" in (d / f"gpu{k}.sam").read_bytes()
    _run(gpu, d, "gpu_two.sam", "--affine", "--gpus", "0,0")
    assert (d / "gpu_two.sam").read_bytes() == (d / "gpu0.sam").read_bytes()
    err = _run(gpu, d, "gpu_plain.sam", "--annotate")
    assert "GPU affine realignment" not in err and b"AS:i:" not in (d / "gpu_plain.sam").read_bytes()


@pytest.mark.gpu
def test_the_tool_with_pairs_and_rescue(tmp_path):
    """--rescue --affine: the picks and the rescued mates realigned on the device, byte for byte the oracle-backed tool's
    records; with --clip on top the tool still writes clip's own AS:i."""
    from test_pair import ARGS as PAIR_ARGS
    from test_rescue import N_LOST, make_rescue_fixture
    make_rescue_fixture(tmp_path)
    gpu = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")

    def tool(exe, out, *extra):
        env = dict(os.environ, BM_VERIFY_BLOCK_READS="6")
        r = subprocess.run([exe, *PAIR_ARGS, "-q", "lost.fastq", "-o", out, "--rescue", *extra], cwd=str(tmp_path), capture_output=True,
                           text=True, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        return (tmp_path / out).read_bytes(), r.stderr
    cpu, _ = tool(TOOLS["bucketmap_align"], "cpu.sam", "--affine")
    got, err = tool(gpu, "gpu.sam", "--affine")
    assert "GPU affine realignment" in err and "GPU mate rescue" in err
    assert got == cpu and got.count(b"XR:i:1") >= N_LOST and got.count(b"AS:i:") == got.count(b"NM:i:") > 0
    clipped, _ = tool(gpu, "clip.sam", "--affine", "--clip")
    assert clipped.count(b"AS:i:") == clipped.count(b"NM:i:") > 0
