"""Alignments beyond the verifier's limits (bmv_align_long, include/bmv.h): reads of more than 65 536 bases, as the
reference aligns any query.size() against a window of any width (bucket_map/locator/bucket_locator.h:549-589).

The long path's kernels (csrc/bmv_long.hip.h) are held to the existing ones inside the old limits (BMV_LONG_FROM sends
every query through them; the existing kernels are oracle-identical, so this pins the tie rules), to the two-row
checker and an independent big-int Myers bottom row beyond them, to a planted 1-Mbp optimum, and end to end through
`bucketmap_align`."""
import multiprocessing
import os
import re
import subprocess
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from oracle import oracle_c as oc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(a):
    return np.frombuffer(bytes(a).translate(COMP)[::-1], np.uint8)


def _mutate(rng, seq, sub, ins, dele):
    """ONT-like noise, vectorised: per base a deletion, else an optional inserted base before it and a substitution."""
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


def _assert_same(got, want, what):
    s, b, o, c = got
    s2, b2, o2, c2 = want
    bad = np.nonzero(s != s2)[0]
    assert bad.size == 0, f"{what}: scores differ at {bad[:10]}: {s[bad[:5]]} vs {s2[bad[:5]]}"
    bad = np.nonzero(b != b2)[0]
    assert bad.size == 0, f"{what}: begin positions differ at {bad[:10]}"
    assert np.array_equal(o, o2), f"{what}: CIGAR lengths differ"
    assert np.array_equal(c, c2), f"{what}: CIGARs differ"


def _assert_optimal(genome, batch, res, what):
    bad = oc.check_alignments(genome, *batch, *res)
    assert not bad.any(), f"{what}: check_alignments reports {bad[bad != 0][:5]} at {np.flatnonzero(bad)[:5]}"


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


def _limits_batch(rng, genome):
    """Query lengths around every word, strip and limit boundary, both strands, N bases, short / empty texts, a text at the genome's end."""
    b = _Batch()
    g = len(genome)
    for m in (1, 63, 64, 65, 500, 5000, 20000, 32768, 32769, 49200, 65536):
        for rc in (0, 1):
            width = m + 1 + m // 10
            start = int(rng.integers(0, g - width))
            src = genome[start + 1: start + 1 + m]
            q = _mutate(rng, _revcomp(src) if rc else src, 0.03, 0.025, 0.025)[:m]
            if len(q) < m:
                q = np.concatenate([q, rng.choice(list(b"ACGT"), m - len(q)).astype(np.uint8)])
            b.add(q, start, min(width, 81920), rc)
    q = rng.choice(list(b"ACGTN"), 3000).astype(np.uint8)                          # N bases, unrelated
    b.add(q, 1000, 3301, 0)
    q = genome[5001:7001].copy()
    q[::97] = ord("N")
    b.add(q, 5000, 2201, 1)
    b.add(genome[9000:9800], 9000, 300, 0)                                         # text shorter than the query
    b.add(genome[9000:9800], 9100, 3, 1)
    b.add(genome[12000:12500], 12000, 0, 0)                                        # empty text
    b.add(genome[12000:40000], 12000, 0, 1)
    b.add(genome[g - 20000:], g - 22000, 22000, 0)                                 # a text that ends at the genome's last base
    b.add(_revcomp(genome[g - 60000:]), g - 72000, 72000, 1)
    return b.args()


@pytest.fixture(scope="module")
def genome():
    return np.random.default_rng(20241001).choice(list(b"ACGT"), 1_600_000).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("scratch_mb", [None, 160])
def test_long_path_equals_existing_kernels_within_the_limits(genome, monkeypatch, scratch_mb):
    """BMV_LONG_FROM=1: every query takes the new tiles; score, begin and every CIGAR entry equal bmv_align's."""
    rng = np.random.default_rng(11)
    batch = _limits_batch(rng, genome)
    v = _verifier(scratch_mb)
    v.load_genome(genome)
    want = v.align(*batch)
    monkeypatch.setenv("BMV_LONG_FROM", "1")
    got = v.align_long(*batch)
    _assert_same(got, want, "long path against bmv_align")
    if scratch_mb is None:                                   # a few short tiles per alignment: many launches, one piece
        monkeypatch.setenv("BMV_LONG_CHUNK", "1024")
        _assert_same(v.align_long(*batch), want, "1024-step tiles")
    v.close()


def _last_min_column(text: bytes, query: bytes):
    """Myers' bottom row with Python ints (the whole query one integer): the minimum and its LAST column (rule 1)."""
    m = len(query)
    full, top = (1 << m) - 1, 1 << (m - 1)
    qa = np.frombuffer(query, np.uint8)
    peq = {c: int.from_bytes(np.packbits(qa[::-1] == c).tobytes(), "big") >> ((-m) % 8) for c in b"ACGT"}
    pv, mv, score, best, best_j = full, 0, m, m, 0
    for j, c in enumerate(text, 1):
        eq = peq[c]
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | (~(xh | pv) & full)
        mh = pv & xh
        if ph & top:
            score += 1
        elif mh & top:
            score -= 1
        ph = (ph << 1) & full
        mh = (mh << 1) & full
        pv = mh | (~(xv | ph) & full)
        mv = ph & xv
        if score <= best:
            best, best_j = score, j
    return best, best_j


def test_big_int_bottom_row_agrees_with_the_oracle():
    """The independent rule-1 check itself, on small cases against the C oracle (CPU)."""
    rng = np.random.default_rng(5)
    for _ in range(100):
        t = bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 90))).astype(np.uint8))
        q = bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 80))).astype(np.uint8))
        s, b, cg = oc.align(t, q, False)
        used = sum(int(n) for n, o in re.findall(r"(\d+)([MID])", cg) if o in "MD")
        assert _last_min_column(t, q) == (-s, b + used)


def _window(genome, start, width, rc):
    t = genome[start: start + width]
    return bytes(_revcomp(t) if rc else t)


@pytest.mark.gpu
def test_long_alignments_are_optimal(genome):
    """65 537, 100 000 and 250 000 bases at ONT-like error rates, both strands, text = m + 1 + 10 %: the two-row checker
    reports nothing, and the big-int bottom row's last minimal column is begin + the text the CIGAR consumes."""
    rng = np.random.default_rng(12)
    b = _Batch()
    for m in (65537, 100_000, 250_000):
        for rc in (0, 1):
            width = m + 1 + m // 10
            start = int(rng.integers(0, len(genome) - width))
            src = genome[start + 1: start + 1 + m]
            b.add(_mutate(rng, _revcomp(src) if rc else src, 0.03, 0.025, 0.025), start, width, rc)
    batch = b.args()
    reads, ts, tl, trc, qs, ql = batch
    v = _verifier()
    v.load_genome(genome)
    res = v.align_long(*batch)
    v.close()
    score, begin, off, cg = res
    texts = [_window(genome, int(ts[a]), int(tl[a]), int(trc[a])) for a in range(len(ts))]
    queries = [bytes(reads[int(qs[a]): int(qs[a]) + int(ql[a])]) for a in range(len(ts))]
    # (fresh interpreters, not forks of this one: they never touch the GPU)
    with ProcessPoolExecutor(min(len(ts), max(1, len(os.sched_getaffinity(0)) // 2)),
                             mp_context=multiprocessing.get_context("spawn")) as pool:
        rows = [pool.submit(_last_min_column, t, q) for t, q in zip(texts, queries)]
        _assert_optimal(genome, batch, res, "long alignments")
        for a, f in enumerate(rows):
            best, best_j = f.result()
            used = sum(int(e) >> 4 for e in cg[off[a]: off[a + 1]] if int(e) & 15 != 1)
            assert -best == score[a] and best_j == begin[a] + used, (a, best, best_j, score[a], begin[a], used)
    assert (score < -0.04 * ql).all() and (score > -0.12 * ql).all()


@pytest.mark.gpu
@pytest.mark.parametrize("rc", [0, 1])
def test_one_megabase_query_planted_substitutions(rc):
    """A 1 048 576-base query with only substitutions at least 1 kbp apart: the optimum is unique -- score = -subs,
    the planted begin, 1048576M."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(13 + rc)
    m, width = 1 << 20, 1_150_000
    genome = rng.choice(list(b"ACGT"), width + 50_000).astype(np.uint8)
    start, p = 20_000, 40_000                                # text genome[start, +width); the query at p in it
    q = genome[start + p: start + p + m].copy()
    at = np.cumsum(rng.integers(1000, 3000, m // 1000))
    at = at[at < m - 10]
    q[at] = np.frombuffer(bytes(q[at]).translate(bytes.maketrans(b"ACGT", b"CGTA")), np.uint8)
    if rc:
        q = _revcomp(q)
    v = verify.Verifier()
    v.load_genome(genome)
    score, begin, off, cg = v.align_long(q, [start], [width], [rc], [0], [m])
    stats = v.stats()
    v.close()
    assert score[0] == -len(at)
    assert begin[0] == (width - p - m if rc else p)
    assert verify.cigar_string(cg[off[0]: off[1]]) == f"{m}M"
    assert stats["cells"] == m * width


@pytest.mark.gpu
def test_mixed_batch(genome, monkeypatch):
    """300 bp, 10 kbp and 80 kbp in one align_long call: the short ones exactly as align alone gives them, the long ones
    optimal."""
    monkeypatch.delenv("BMV_LONG_FROM", raising=False)
    rng = np.random.default_rng(14)
    b, short = _Batch(), []
    for a in range(60):
        m = (300, 10_000, 80_000)[a % 3] if a < 57 else 80_000 + 17 * a
        rc = int(rng.integers(0, 2))
        width = m + 1 + m // 10
        start = int(rng.integers(0, len(genome) - width))
        src = genome[start + 1: start + 1 + m]
        b.add(_mutate(rng, _revcomp(src) if rc else src, 0.03, 0.025, 0.025), start, width, rc)
        if m < 65536:
            short.append(a)
    batch = b.args()
    v = _verifier()
    v.load_genome(genome)
    res = v.align_long(*batch)
    sub = _Batch()
    for a in short:
        sub.add(b.reads[a], b.ts[a], b.tl[a], b.trc[a])
    want = v.align(*sub.args())
    v.close()
    score, begin, off, cg = res
    s_sub = score[short], begin[short]
    got_off = np.concatenate([[0], np.cumsum([off[a + 1] - off[a] for a in short])]).astype(np.uint64)
    got_cg = np.concatenate([cg[off[a]: off[a + 1]] for a in short]).astype(np.uint32)
    _assert_same((s_sub[0], s_sub[1], got_off, got_cg), want, "short ones of a mixed batch")
    _assert_optimal(genome, batch, res, "mixed batch")


@pytest.mark.gpu
def test_trace_beyond_the_scratch_is_refused_cleanly(genome):
    """A 200-kbp alignment whose trace does not fit a tiny scratch: BMV_ERR_UNSUPPORTED, naming it; the same Verifier
    then aligns a normal batch correctly."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(15)
    v = _verifier(64)
    v.load_genome(genome)
    m = 200_000
    src = genome[1001: 1001 + m]
    q = _mutate(rng, src, 0.03, 0.025, 0.025)
    with pytest.raises(verify.BmvError) as e:
        v.align_long(q, [1000], [m + 1 + m // 10], [0], [0], [len(q)])
    assert e.value.code == 5 and "alignment 0" in str(e.value) and "bytes" in str(e.value)
    b = _Batch()
    for a in range(40):
        mm = int(rng.integers(100, 3000))
        start = int(rng.integers(0, len(genome) - 2 * mm))
        b.add(_mutate(rng, genome[start + 1: start + 1 + mm], 0.02, 0.01, 0.01), start, mm + 1 + mm // 10, a % 2)
    batch = b.args()
    _assert_same(v.align_long(*batch), oc.align_batch(genome, *batch), "after a refusal")
    v.close()


# ------------------------------------------------------------------------------------------------ the tool

def _fastq_records(path, prefix):
    lines = open(path, "rb").read().split(b"\n")
    out = []
    for x in range(0, len(lines) - 3, 4):
        if lines[x].startswith(b"@"):
            out.append(b"@" + prefix + lines[x][1:] + b"\n" + lines[x + 1] + b"\n+\n" + lines[x + 3] + b"\n")
    return out


def _run(exe, args, cwd, env=None):
    r = subprocess.run([exe, *args], cwd=str(cwd), capture_output=True, text=True,
                       env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _records(path):
    return [l for l in open(path, "rb").read().split(b"\n") if l and not l.startswith(b"@")]


@pytest.mark.gpu
def test_bucketmap_align_with_ultralong_reads(tmp_path):
    """`bucketmap_align` with the ultralong profile's flags on a FASTQ that holds four reads of 70-120 kbp among
    4-18 kbp ones: exits 0, the long reads' CIGARs consume them and are optimal, every other read's SAM lines are those
    of a run without the long reads, and two contexts write the same file."""
    from bucket_map_amd import host
    exe = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    g = host.Genome.synth(32, [1_500_000])
    g.write_fasta(str(tmp_path / "g.fa"))
    short, long_ = [], []
    for k, (length, count) in enumerate([(4000, 6), (10_000, 4), (18_000, 3)]):
        rd = host.Reads(g, 262144, 300, length, count, sub=0.03, ins=0.025, dele=0.025, seed=40 + k)
        rd.write_fastq(str(tmp_path / f"s{k}"))
        short += _fastq_records(tmp_path / f"s{k}.fastq", b"s%d_" % k)
    for k, length in enumerate([70_000, 120_000]):
        rd = host.Reads(g, 262144, 300, length, 2, sub=0.03, ins=0.025, dele=0.025, seed=50 + k)
        rd.write_fastq(str(tmp_path / f"l{k}"))
        long_ += _fastq_records(tmp_path / f"l{k}.fastq", b"l%d_" % k)
    mixed = short[:4] + long_[:2] + short[4:9] + long_[2:] + short[9:]
    (tmp_path / "mixed.fastq").write_bytes(b"".join(mixed))
    (tmp_path / "short.fastq").write_bytes(b"".join(short))
    names = [r.split(b"\n")[0][1:] for r in mixed]
    assert len(set(names)) == len(names)
    long_names = {r.split(b"\n")[0][1:] for r in long_}
    flags = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "262144", "-f", "1", "-s", "30", "-e", "0.9", "-n", "0.1",
             "-l", "12", "-p", "20", "-u", "5"]
    err = _run(exe, [*flags, "-q", "mixed.fastq", "-o", "mixed.sam"], tmp_path, env={"BM_DUMP_ALIGNMENTS": str(tmp_path / "dump.txt")})
    assert "GPU alignment verification" in err
    _run(exe, [*flags, "-q", "short.fastq", "-o", "short.sam"], tmp_path)
    _run(exe, [*flags, "-q", "mixed.fastq", "-o", "two.sam", "--gpus", "0,0"], tmp_path)
    mixed_recs = _records(tmp_path / "mixed.sam")
    assert (tmp_path / "two.sam").read_bytes() == (tmp_path / "mixed.sam").read_bytes()
    # every other read: byte-identical lines
    assert [r for r in mixed_recs if r.split(b"\t")[0] not in long_names] == _records(tmp_path / "short.sam")
    # the long reads: records whose CIGARs consume them
    seen = set()
    for r in mixed_recs:
        f = r.split(b"\t")
        if f[0] in long_names:
            seen.add(f[0])
            used = sum(int(n) for n, o in re.findall(rb"(\d+)([MID])", f[5]) if o in b"MI")
            assert used == len(f[9]) > 65536
    assert seen == long_names
    # their alignments, as the verifier returned them: optimal
    flat, _ = g.flat()
    seqs = [np.frombuffer(r.split(b"\n")[1], np.uint8) for r in mixed]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    reads = np.concatenate(seqs)
    rows = [l.split() for l in open(tmp_path / "dump.txt")]
    rows = [r for r in rows if int(r[4]) > 65536]
    assert len({int(r[0]) for r in rows}) == len(long_names)
    rd = np.array([int(r[0]) for r in rows])
    ql = np.array([int(r[4]) for r in rows], np.uint32)
    assert np.array_equal(ql, np.diff(offsets)[rd].astype(np.uint32))
    cig, off = [], [0]
    for r in rows:
        if r[7] != "*":
            cig += [(int(n) << 4) | "MID".index(op) for n, op in re.findall(r"(\d+)([MID])", r[7])]
        off.append(len(cig))
    bad = oc.check_alignments(flat, reads, np.array([int(r[1]) for r in rows], np.uint64),
                              np.array([int(r[2]) for r in rows], np.uint32), np.array([int(r[3]) for r in rows], np.uint8),
                              offsets[rd], ql, np.array([int(r[5]) for r in rows], np.int32),
                              np.array([int(r[6]) for r in rows], np.uint32), np.array(off, np.uint64), np.array(cig, np.uint32))
    assert not bad.any(), (np.flatnonzero(bad)[:5], bad[bad != 0][:5])
