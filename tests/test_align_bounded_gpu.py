"""Edit-bounded verification on the GPU (bmv_align_bounded, include/bmv.h): an alignment is accepted iff its semi-global
edit distance is within its bound, accepted ones are bit-identical to bmv_align's, rejected ones carry BMV_REJECTED and
no CIGAR, and the screen's cut-off really leaves most of a wrong locus's matrix alone.

Expected scores come from the C oracle (oracle/bm_align_oracle.c through oracle_c.align_batch / check_alignments), the
bit identity from Verifier.align / align_long on the same batch."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle_c as oc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMP = bytes.maketrans(b"ACGT", b"TGCA")
# kClassUpTo of bmv_align (csrc/bmv_api.hip), in 64-row words: the length classes' upper ends
CLASS_UP_TO = (8, 16, 20, 24, 32)


def _revcomp(a):
    return np.frombuffer(bytes(a).translate(COMP)[::-1], np.uint8)


def _mutate(rng, seq, sub, ins, dele):
    seq = np.asarray(seq, np.uint8)
    r = rng.random(len(seq))
    keep = r >= dele
    insert = (r >= dele) & (r < dele + ins)
    bases = np.frombuffer(b"ACGT", np.uint8)
    out = np.where(rng.random(len(seq)) < sub, bases[rng.integers(0, 4, len(seq))], seq)
    ins_b = bases[rng.integers(0, 4, len(seq))]
    pair = np.stack([np.where(insert, ins_b, 0), np.where(keep, out, 0)], 1).ravel()
    return pair[pair != 0].astype(np.uint8)


class _Batch:
    def __init__(self):
        self.reads, self.ts, self.tl, self.trc, self.qs, self.ql, self.at = [], [], [], [], [], [], 0

    def add(self, q, start, width, rc):
        q = np.asarray(q, np.uint8)
        self.reads.append(q)
        self.ts.append(start); self.tl.append(width); self.trc.append(rc); self.qs.append(self.at); self.ql.append(len(q))
        self.at += len(q)

    def args(self):
        reads = np.concatenate(self.reads) if self.at else np.zeros(0, np.uint8)
        return (reads, np.array(self.ts, np.uint64), np.array(self.tl, np.uint32), np.array(self.trc, np.uint8),
                np.array(self.qs, np.uint64), np.array(self.ql, np.uint32))


def _verifier(scratch_mb=None):
    from bucket_map_amd import verify
    old = os.environ.get("BMV_SCRATCH_MB")
    if scratch_mb is not None:
        os.environ["BMV_SCRATCH_MB"] = str(scratch_mb)
    try:
        return verify.Verifier()
    finally:
        if scratch_mb is not None:
            if old is None:
                del os.environ["BMV_SCRATCH_MB"]
            else:
                os.environ["BMV_SCRATCH_MB"] = old


def _assert_contract(got, want, bounds, oracle_score, what):
    """got: align_bounded's result; want: the unbounded result of the same batch; oracle_score: the oracle's scores."""
    from bucket_map_amd import verify
    s, b, o, c = got
    s2, b2, o2, c2 = want
    n = len(s)
    assert len(o) == n + 1 and o[0] == 0 and o[n] == len(c), f"{what}: total_cigar is not the sum of the accepted CIGARs"
    expect_reject = -oracle_score.astype(np.int64) > np.asarray(bounds, np.int64)
    rejected = s == verify.REJECTED
    wrong = np.flatnonzero(rejected != expect_reject)
    assert wrong.size == 0, (f"{what}: rejected set differs from the oracle's at {wrong[:10]}: oracle scores "
                             f"{oracle_score[wrong[:10]]}, bounds {np.asarray(bounds)[wrong[:10]]}")
    lens = np.diff(o.astype(np.int64))
    assert (lens[rejected] == 0).all() and (b[rejected] == 0).all(), f"{what}: a rejected alignment has a begin or a CIGAR"
    acc = np.flatnonzero(~rejected)
    assert np.array_equal(s[acc], s2[acc]) and np.array_equal(s[acc], oracle_score[acc]), f"{what}: accepted scores differ"
    assert np.array_equal(b[acc], b2[acc]), f"{what}: accepted begins differ"
    assert np.array_equal(lens[acc], np.diff(o2.astype(np.int64))[acc]), f"{what}: accepted CIGAR lengths differ"
    for a in acc:
        assert np.array_equal(c[o[a]: o[a + 1]], c2[o2[a]: o2[a + 1]]), f"{what}: CIGAR of alignment {a} differs"
    return int(rejected.sum())


@pytest.fixture(scope="module")
def genome():
    return np.random.default_rng(20241101).choice(list(b"ACGT"), 1_600_000).astype(np.uint8)


def _unrelated_start(rng, genome, width, start):
    """A window start whose text shares no base with the window at `start`, nor with the read's source inside it (a plain
    random draw lands within a window's length of the source once in some hundred 10-kbp draws, and such a "decoy" is within
    the bound)."""
    while True:
        other = int(rng.integers(0, len(genome) - width - 1))
        if abs(other - start) > 2 * width:
            return other


def _true_and_decoy(rng, genome, b, m, rc, err=(0.03, 0.025, 0.025), slack=None):
    width = m + 1 + (m // 10 if slack is None else slack)
    start = int(rng.integers(0, len(genome) - width - 1))
    src = genome[start + 1: start + 1 + m]
    q = _mutate(rng, _revcomp(src) if rc else src, *err)[:m]
    if len(q) < m:
        q = np.concatenate([q, rng.choice(list(b"ACGT"), m - len(q)).astype(np.uint8)])
    b.add(q, start, width, rc)
    b.add(q, _unrelated_start(rng, genome, width, start), width, rc)          # the same read at an unrelated place


@pytest.mark.gpu
def test_exact_accept_and_reject_at_the_boundary(genome):
    """Bounds -s - 1, -s, -s + 1, 0 and query_len around every word, lane-kernel and class boundary: reject, accept,
    accept, accept iff s = 0, accept -- and every accepted result is Verifier.align's."""
    rng = np.random.default_rng(21)
    lengths = [1, 2, 3, 10, 63, 64, 65, 100, 127, 128, 129, 300, 511, 512, 513, 700, 1999, 2000]
    for w in CLASS_UP_TO:
        lengths += [64 * w - 1, 64 * w, 64 * w + 1]
    lengths += [int(x) for x in rng.integers(1, 2001, 40)]
    b = _Batch()
    for m in lengths:
        _true_and_decoy(rng, genome, b, m, int(rng.integers(0, 2)))
    for m in (64, 150, 512, 600):                            # exact copies: s = 0
        start = int(rng.integers(0, len(genome) - 2 * m))
        b.add(genome[start + 3: start + 3 + m], start, m + 7, 0)
        b.add(_revcomp(genome[start + 3: start + 3 + m]), start, m + 7, 1)
    batch = b.args()
    ql = batch[5].astype(np.int64)
    ora = oc.align_batch(genome, *batch)
    s = ora[0].astype(np.int64)
    assert (s == 0).any() and (-s > ql // 3).any()
    v = _verifier()
    v.load_genome(genome)
    want = v.align(*batch)
    for name, bounds in (("-s - 1", -s - 1), ("-s", -s), ("-s + 1", -s + 1), ("0", np.zeros_like(s)), ("query_len", ql)):
        ok = bounds >= 0                                     # (-s - 1 does not exist for s = 0: those take bound 0)
        bounds = np.where(ok, bounds, 0)
        got = v.align_bounded(*batch, bounds.astype(np.uint32))
        n_rej = _assert_contract(got, want, bounds, ora[0], f"bound {name}")
        assert v.bounded_stats()["n_rejected"] == n_rej
        if name == "-s - 1":
            assert n_rej == int(ok.sum())
        if name in ("-s", "-s + 1", "query_len"):
            assert n_rej == 0
        if name == "query_len":
            assert v.bounded_stats()["screen_cells"] == 0    # nothing to reject: the screen is skipped
    v.close()


def _short_mixed(rng, genome, count):
    b = _Batch()
    for a in range(count):
        m, width = 300, 307
        rc = int(rng.integers(0, 2))
        start = int(rng.integers(0, len(genome) - width - 1))
        src = genome[start + 3: start + 3 + m]
        q = _mutate(rng, _revcomp(src) if rc else src, 0.02, 0.01, 0.01)[:m]
        if len(q) < m:
            q = np.concatenate([q, rng.choice(list(b"ACGT"), m - len(q)).astype(np.uint8)])
        if a % 5:                                            # 80 % decoys: the text from an unrelated place
            start = _unrelated_start(rng, genome, width, start)
        b.add(q, start, width, rc)
    q = rng.choice(list(b"ACGTN"), 300).astype(np.uint8)     # N bases
    b.add(q, 1000, 307, 0)
    q = genome[5003:5303].copy()
    q[::37] = ord("N")
    b.add(q, 5000, 307, 0)
    b.add(_revcomp(q), 5000, 307, 1)
    b.add(genome[9000:9300], 9000, 100, 0)                   # texts shorter than the query, an empty one
    b.add(genome[9000:9300], 9100, 3, 1)
    b.add(genome[12000:12300], 12000, 0, 0)
    b.add(np.zeros(0, np.uint8), 13000, 307, 0)              # empty queries
    b.add(np.zeros(0, np.uint8), 13000, 0, 1)
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("scratch_mb", [None, 24])
def test_mixed_batch_of_short_reads(genome, scratch_mb):
    """20 000 alignments of 300 x 307, four of five at unrelated places, rate 0.1; once with a scratch that forces pieces."""
    rng = np.random.default_rng(22)
    batch = _short_mixed(rng, genome, 20_000).args()
    bounds = (0.1 * batch[5]).astype(np.uint32)
    ora = oc.align_batch(genome, *batch)
    v = _verifier(scratch_mb)
    v.load_genome(genome)
    want = v.align(*batch)
    got = v.align_bounded(*batch, bounds)
    st, all_st = v.bounded_stats(), v.stats()
    v.close()
    n_rej = _assert_contract(got, want, bounds, ora[0], "short mixed batch")
    assert st["n_rejected"] == n_rej and 0.7 * len(bounds) < n_rej < 0.9 * len(bounds)
    cells = int((batch[5].astype(np.int64) * batch[2]).sum())
    assert all_st["cells"] == cells
    assert 0 < st["screen_cells"] < cells, st
    assert all_st["ms_kernels"] >= st["ms_screen"] > 0


@pytest.mark.gpu
def test_mixed_batch_of_long_reads(genome):
    """400 alignments of 10 000 x 11 001 with ONT-like errors, four of five at unrelated places, rate 0.15.  The scores the
    rejected set is derived from are Verifier.align's, each confirmed optimal by the two-row checker (O(n) memory)."""
    rng = np.random.default_rng(23)
    b = _Batch()
    for a in range(400):
        m, width = 10_000, 11_001
        rc = int(rng.integers(0, 2))
        start = int(rng.integers(0, len(genome) - width - 1))
        src = genome[start + 1: start + 1 + m]
        q = _mutate(rng, _revcomp(src) if rc else src, 0.03, 0.025, 0.025)[:m]
        if len(q) < m:
            q = np.concatenate([q, rng.choice(list(b"ACGT"), m - len(q)).astype(np.uint8)])
        if a % 5:
            start = _unrelated_start(rng, genome, width, start)
        b.add(q, start, width, rc)
    batch = b.args()
    bounds = (0.15 * batch[5]).astype(np.uint32)
    v = _verifier()
    v.load_genome(genome)
    want = v.align(*batch)
    got = v.align_bounded(*batch, bounds)
    st = v.bounded_stats()
    v.close()
    bad = oc.check_alignments(genome, *batch, *want)
    assert not bad.any(), (np.flatnonzero(bad)[:5], bad[bad != 0][:5])
    n_rej = _assert_contract(got, want, bounds, want[0], "long mixed batch")
    assert n_rej == 320 == st["n_rejected"]
    cells = int((batch[5].astype(np.int64) * batch[2]).sum())
    assert 0 < st["screen_cells"] < cells, st


@pytest.mark.gpu
def test_batch_that_mixes_length_classes(genome):
    """100 .. 12 000 bases in one call, true and unrelated places, bounds of 5 .. 25 %."""
    rng = np.random.default_rng(24)
    b = _Batch()
    for a in range(150):
        m = int(rng.choice([100, 300, 512, 513, 900, 1500, 2500, 4000, 6000, 12_000]))
        _true_and_decoy(rng, genome, b, m, int(rng.integers(0, 2)))
    batch = b.args()
    bounds = (rng.uniform(0.05, 0.25, len(batch[5])) * batch[5]).astype(np.uint32)
    v = _verifier()
    v.load_genome(genome)
    want = v.align(*batch)
    got = v.align_bounded(*batch, bounds)
    st = v.bounded_stats()
    v.close()
    bad = oc.check_alignments(genome, *batch, *want)
    assert not bad.any(), (np.flatnonzero(bad)[:5], bad[bad != 0][:5])
    n_rej = _assert_contract(got, want, bounds, want[0], "mixed length classes")
    assert n_rej >= 150 and st["screen_cells"] < int((batch[5].astype(np.int64) * batch[2]).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,cap", [(300, 307, 15, 19_328), (10_000, 11_001, 500, 938_880)])
def test_the_cut_off_really_cuts(m, n, k, cap):
    """A query of all A against a text of all C: D[i][j] = i, so the last row within k is k in every column; the screen
    needs ceil(k / 64) words until column n - m + k + 1.  The cap allows one word and 128 columns more:
    64 (ceil(k / 64) + 1) (n - m + k + 1 + 128)."""
    assert cap == 64 * (-(-k // 64) + 1) * (n - m + k + 1 + 128)
    genome = np.full(n + 100, ord("C"), np.uint8)
    q = np.full(m, ord("A"), np.uint8)
    v = _verifier()
    v.load_genome(genome)
    score, begin, off, cg = v.align_bounded(q, [10], [n], [0], [0], [m], [k])
    st = v.bounded_stats()
    v.close()
    from bucket_map_amd import verify
    assert score[0] == verify.REJECTED and begin[0] == 0 and off[1] == 0 and len(cg) == 0
    assert st["n_rejected"] == 1
    print(f"screen_cells {st['screen_cells']} of {m * n}, cap {cap}")
    assert 0 < st["screen_cells"] <= cap < m * n, st


@pytest.mark.gpu
def test_beyond_the_limits(genome, monkeypatch):
    """A 70 000-base read at its place and at an unrelated one: no screen, the contract all the same; the context then
    serves a normal bounded batch."""
    from bucket_map_amd import verify
    monkeypatch.delenv("BMV_LONG_FROM", raising=False)
    rng = np.random.default_rng(25)
    b = _Batch()
    _true_and_decoy(rng, genome, b, 70_000, 1)
    batch = b.args()
    bounds = np.array([10_500, 10_500], np.uint32)
    v = _verifier()
    v.load_genome(genome)
    want = v.align_long(*batch)
    got = v.align_bounded(*batch, bounds)
    assert v.bounded_stats() == {"n_rejected": 1, "screen_cells": 0, "ms_screen": 0.0}
    bad = oc.check_alignments(genome, *batch, *want)
    assert not bad.any()
    _assert_contract(got, want, bounds, want[0], "beyond the limits")
    assert got[0][0] == want[0][0] > -10_500 and got[0][1] == verify.REJECTED
    small = _short_mixed(rng, genome, 500).args()
    sb = (0.1 * small[5]).astype(np.uint32)
    _assert_contract(v.align_bounded(*small, sb), v.align(*small), sb, oc.align_batch(genome, *small)[0], "afterwards")
    v.close()


# ------------------------------------------------------------------------------------------------ the tool

def _tool(args, cwd, env=None):
    exe = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    r = subprocess.run([exe, *args], cwd=str(cwd), capture_output=True, text=True, env={**os.environ, **(env or {})})
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


@pytest.mark.gpu
def test_bucketmap_align_with_max_edit_rate(tmp_path):
    """Short reads and ONT-like 6-kbp reads: the bounded SAM is the unbounded one without exactly the records whose dumped
    score is below -(uint32)(R * read length); two contexts write the same file; without the option nothing changes.
    The long reads all lie at their true places with 3 % substitutions and 2.5 % each of insertions and deletions, so their
    edit rates spread around 0.075: R = 5/64 (exact in float32) has alignments on both sides."""
    from bucket_map_amd import host
    from test_align_bounded import bounded_sam_is_unbounded_minus_rejections
    g = host.Genome.synth(33, [900_000, 300_000])
    g.write_fasta(str(tmp_path / "g.fa"))
    cases = [("short", ["--bucket-len", "8192", "-r", "150", "-f", "1", "-u", "0"], 0.0625,
              host.Reads(g, 8192, 150, 150, 3000, sub=0.03, seed=6)),
             ("long", ["--bucket-len", "262144", "-f", "1", "-s", "30", "-e", "0.9", "-n", "0.1", "-l", "12", "-p", "20", "-u", "5"], 0.078125,
              host.Reads(g, 262144, 300, 6000, 150, sub=0.03, ins=0.025, dele=0.025, seed=8))]
    for name, flags, rate, rd in cases:
        rd.write_fastq(str(tmp_path / name))
        common = ["-i", f"idx_{name}", "--genome", "g.fa", *flags, "-q", f"{name}.fastq"]
        u = int(flags[flags.index("-u") + 1])
        _tool([*common, "-o", f"{name}_all.sam"], tmp_path, env={"BM_DUMP_ALIGNMENTS": str(tmp_path / f"{name}_all.txt")})
        err = _tool([*common, "-o", f"{name}_b.sam", "--max-edit-rate", str(rate)], tmp_path,
                    env={"BM_DUMP_ALIGNMENTS": str(tmp_path / f"{name}_b.txt")})
        assert "rejected by the edit bound" in err and "screen cells" in err
        _tool([*common, "-o", f"{name}_b2.sam", f"--max-edit-rate={rate}", "--gpus", "0,0"], tmp_path)
        _tool([*common, "-o", f"{name}_all2.sam"], tmp_path)
        read = lambda f: open(tmp_path / f).read().split("\n")
        n_over, n_gone = bounded_sam_is_unbounded_minus_rejections(read(f"{name}_all.sam"), read(f"{name}_all.txt"), read(f"{name}_b.sam"),
                                                                   read(f"{name}_b.txt"), rate, u)
        assert n_over > 0 and n_gone > 0, (name, n_over, n_gone)
        assert (tmp_path / f"{name}_b2.sam").read_bytes() == (tmp_path / f"{name}_b.sam").read_bytes()
        md5 = lambda f: hashlib.md5((tmp_path / f).read_bytes()).hexdigest()
        assert md5(f"{name}_all2.sam") == md5(f"{name}_all.sam")


@pytest.mark.gpu
def test_unset_option_leaves_the_golden_sam_alone(tmp_path):
    """tests/golden/sam_small.json through the product tool: --max-edit-rate=1 can reject nothing there and the records
    are the fixture's; with a bound, the records are the fixture's minus those beyond it."""
    from test_align_bounded import _inputs, _run, TOOLS
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "sam_small.json")))
    _inputs(golden, tmp_path)
    TOOLS["gpu_align"] = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    recs = lambda lines: [l.split("\t") for l in lines if l and not l.startswith("@")]
    want = golden["bucketmap_align"]["sam"]
    plain = recs(_run(golden, "gpu_align", tmp_path, "p.sam"))
    loose = recs(_run(golden, "gpu_align", tmp_path, "l.sam", extra=["--max-edit-rate=1"]))
    assert plain == loose and len(plain) == len(want)
    for f, w in zip(plain, want):
        assert [f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[9], f[10]] == w
    tight = recs(_run(golden, "gpu_align", tmp_path, "t.sam", extra=["--max-edit-rate=0.125"]))
    oracle = recs(_run(golden, "bucketmap_align", tmp_path, "o.sam", extra=["--max-edit-rate=0.125"]))
    assert tight == oracle and 0 < len(tight) < len(plain)
