"""The annotation pass on the GPU (bmv_annotate, include/bmv.h): forward-strand pos, =/X/I/D entries, NM and the reference
bases under X and D columns, for hand-planted CIGARs and for what align / align_long / align_bounded return; the refusals;
and `bucketmap_align --annotate`, whose records are walked over the FASTA in Python.

Expected values come from test_annotate.restate, the plain-Python restatement pinned on hand-worked cases there."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from test_annotate import D, EQ, I, M, X, pack, rank, restate

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COMP = bytes.maketrans(b"ACGT", b"TGCA")
LETTERS = [b"AaNnRrWwMm", b"CcYySsBb", b"GgKk", b"TtUu"]        # by dna4 rank


def _revcomp(a):
    return np.frombuffer(bytes(a).translate(COMP)[::-1], np.uint8)


def _mutate(rng, seq, sub, ins, dele):
    seq = np.asarray(seq, np.uint8)
    r = rng.random(len(seq))
    keep = r >= dele
    insert = keep & (r < dele + ins)
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


def _unpack(c):
    return [(int(e) & 15, int(e) >> 4) for e in c]


def _expected(genome, batch, begin, off, cg):
    reads, ts, tl, trc, qs, ql = batch
    return [restate(bytes(genome[int(ts[a]): int(ts[a]) + int(tl[a])]), int(trc[a]), bytes(reads[int(qs[a]): int(qs[a]) + int(ql[a])]),
                    int(begin[a]), _unpack(cg[int(off[a]): int(off[a + 1])])) for a in range(len(ts))]


def _assert_annotations(got, want, what):
    """got: Verifier.annotate's seven arrays; want: restate's tuple per alignment.  Every array, every element."""
    from bucket_map_amd import verify
    nm, pos, ref_len, xo, xc, ro, rb = got
    n = len(want)
    assert len(nm) == len(pos) == len(ref_len) == n and len(xo) == len(ro) == n + 1
    assert xo[0] == 0 and ro[0] == 0 and xo[n] == len(xc) and ro[n] == len(rb), f"{what}: the totals are not the offsets' ends"
    for a, (w_pos, w_ref_len, w_xc, w_nm, w_ref, w_md) in enumerate(want):
        g_xc = _unpack(xc[int(xo[a]): int(xo[a + 1])])
        g_ref = bytes(rb[int(ro[a]): int(ro[a + 1])])
        assert (int(pos[a]), int(ref_len[a]), g_xc, int(nm[a]), g_ref) == (w_pos, w_ref_len, w_xc, w_nm, w_ref), \
            f"{what}: alignment {a} differs from the restatement"
        assert all(p[0] != q[0] for p, q in zip(g_xc, g_xc[1:])), f"{what}: alignment {a} has adjacent entries of one op"
        assert verify.md_string(xc[int(xo[a]): int(xo[a + 1])], g_ref) == w_md, f"{what}: MD of alignment {a}"


def _verifier():
    from bucket_map_amd import verify
    return verify.Verifier()


@pytest.fixture(scope="module")
def genome():
    """200 000 random bases with stretches of N, lower case and IUPAC letters."""
    rng = np.random.default_rng(20250701)
    g = rng.choice(list(b"ACGT"), 200_000).astype(np.uint8)
    odd = np.frombuffer(b"NnacgtRYKMSWBDHVu", np.uint8)
    at = rng.integers(0, len(g), 6000)
    g[at] = odd[rng.integers(0, len(odd), len(at))]
    g[50_000:50_040] = ord("N")
    return g


# ------------------------------------------------------------------------------------------------ 1. planted CIGARs

def _plant(rng, genome, b, spec, rc, begin=None, end_slack=None, start=None, exact=False):
    """One hand-built alignment.  spec: (op, length) runs with op in = X I D, 5' to 3' of the query, in the aligner's frame.
    The query is written so that exactly these columns come out: a letter of the text's rank under =, of another rank under
    X (any spelling: case, N, IUPAC -- or the plain letter when `exact`).  Returns (begin, M/I/D CIGAR)."""
    R = sum(n for op, n in spec if op != I)
    begin = int(rng.integers(0, 9)) if begin is None else begin
    width = begin + R + (int(rng.integers(0, 9)) if end_slack is None else end_slack)
    start = int(rng.integers(0, len(genome) - width + 1)) if start is None else start
    assert start + width <= len(genome)
    window = genome[start: start + width]
    t = [rank(c) for c in window]
    if rc:
        t = [3 - r for r in reversed(t)]
    q, ti = [], begin
    pick = (lambda r: b"ACGT"[r]) if exact else (lambda r: LETTERS[r][int(rng.integers(0, len(LETTERS[r])))])
    for op, n in spec:
        for _ in range(n):
            if op == I:
                q.append(pick(int(rng.integers(0, 4))))
            elif op == D:
                ti += 1
            else:
                q.append(pick(t[ti] if op == EQ else (t[ti] + int(rng.integers(1, 4))) % 4))
                ti += 1
    cigar = []
    for op, n in spec:
        op = M if op in (EQ, X) else op
        if cigar and cigar[-1][0] == op:
            cigar[-1][1] += n
        else:
            cigar.append([op, n])
    b.add(np.array(q, np.uint8), start, width, rc)
    return begin, [tuple(e) for e in cigar]


def _planted_specs(rng):
    specs = []
    for n in (1, 63, 64, 65, 127, 128, 129):                  # M runs of these lengths: all =, all X, mixed
        specs += [[(EQ, n)], [(X, n)]]
        runs, left = [], n
        while left:
            k = min(left, int(rng.integers(1, 40)))
            runs.append((X if (len(runs) & 1) else EQ, k))
            left -= k
        specs.append(runs)
    specs += [
        [(EQ, 50), (X, 30), (EQ, 20)],                        # an X run from one 64-column step into the next
        [(X, 40), (EQ, 40), (X, 20)],                         # an = run likewise
        [(EQ, 60), (X, 10), (EQ, 120), (X, 70), (EQ, 3)],     # runs over two boundaries
        [(EQ, 70), (I, 3), (EQ, 70)],                         # an = run on both sides of an I entry
        [(X, 70), (I, 1), (X, 70)],
        [(EQ, 64), (I, 2), (EQ, 64)],
        [(EQ, 200)], [(X, 200)],
        [(I, 3), (EQ, 20)], [(EQ, 20), (I, 3)], [(I, 2), (EQ, 70), (X, 1), (I, 4)],
        [(D, 3), (EQ, 20)], [(EQ, 20), (D, 3)], [(D, 2), (EQ, 70), (X, 1), (D, 4)],
        [(EQ, 10), (D, 2), (X, 1), (D, 3), (EQ, 10)],         # D directly before and directly after an X column
        [(EQ, 5), (X, 1), (D, 70), (X, 1), (EQ, 5)],
        [(EQ, 8), (I, 2), (D, 3), (EQ, 8)],                   # I directly followed by D
        [(EQ, 8), (D, 3), (I, 2), (X, 8)],
        [(EQ, 1)], [(X, 1)], [(I, 1)],                        # query length 1
        [(D, 5), (I, 1)],
        [(D, 130)], [(I, 130)],
    ]
    return specs


@pytest.mark.gpu
def test_planted_cigars(genome):
    """A few hundred valid, deliberately non-optimal alignments on both strands: every output array is the restatement's."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(31)
    b, begins, cigars = _Batch(), [], []

    def plant(spec, rc, **kw):
        bg, cg = _plant(rng, genome, b, spec, rc, **kw)
        begins.append(bg)
        cigars.append(cg)

    def empty(qlen):
        b.add(rng.choice(list(b"ACGT"), qlen).astype(np.uint8), int(rng.integers(0, 100_000)), 40, int(rng.integers(0, 2)))
        begins.append(0)
        cigars.append([])

    for spec in _planted_specs(rng):
        for rc in (0, 1):
            plant(spec, rc)
    empty(30)                                                  # an empty CIGAR between two non-empty ones (a rejected alignment)
    for rc in (0, 1):
        plant([(EQ, 30), (X, 2), (EQ, 30)], rc, begin=0)
        plant([(EQ, 30), (X, 2), (EQ, 30)], rc, end_slack=0)   # begin + R = text_len exactly
        plant([(X, 1), (EQ, 70), (D, 1)], rc, begin=0, end_slack=0)
        plant([(EQ, 100), (X, 1)], rc, start=len(genome) - 120, begin=19, end_slack=0)       # the genome's last base
        plant([(D, 2), (X, 3), (EQ, 90)], rc, start=len(genome) - 100, begin=5, end_slack=0)
        empty(0)                                               # a zero-length query
        # genome N against read A is a match; an N under X or D is written A
        plant([(EQ, 40)], rc, start=50_000, begin=0, end_slack=0, exact=True)
        plant([(EQ, 5), (X, 10), (D, 10), (EQ, 5)], rc, start=49_990, begin=5, end_slack=5, exact=True)
    while len(begins) < 300:                                   # random ones on top
        spec, last = [], None
        for _ in range(int(rng.integers(1, 9))):
            op = int(rng.choice([o for o in (EQ, X, I, D) if o != last]))
            spec.append((op, int(rng.integers(1, 150 if op in (EQ, X) else 6))))
            last = op
        if not any(op != D for op, _ in spec):
            continue
        plant(spec, int(rng.integers(0, 2)))
    batch = b.args()
    off = np.concatenate([[0], np.cumsum([len(c) for c in cigars])]).astype(np.uint64)
    cg = np.concatenate([pack(c) for c in cigars]).astype(np.uint32)
    want = _expected(genome, batch, begins, off, cg)
    # the planted properties are really there
    n_at = next(a for a in range(len(begins)) if batch[1][a] == 50_000 and not batch[3][a])
    assert bytes(batch[0][int(batch[4][n_at]):][:40]) == b"A" * 40 and want[n_at][2] == [(EQ, 40)]
    assert want[n_at + 1][4] == b"A" * 20 and want[n_at + 1][5] == "5" + "A0" * 9 + "A0^AAAAAAAAAA5"
    assert any(not w[2] for w in want) and any(b.tl[a] == begins[a] + want[a][1] for a in range(len(want)))
    assert any(b.ts[a] + b.tl[a] == len(genome) for a in range(len(want)))
    v = _verifier()
    v.load_genome(genome)
    got = v.annotate(*batch, begins, off, cg)
    st = v.annotate_stats()
    assert st["columns"] == sum(n for c in cigars for _, n in c) and st["ms_kernels"] > 0
    _assert_annotations(got, want, "planted")
    # the call takes offsets that do not start at 0, as a share of a larger batch has them
    part = slice(100, 200)
    got = v.annotate(batch[0], *(x[part] for x in batch[1:]), begins[part], off[100:201], cg)
    v.close()
    _assert_annotations(got, want[part], "a share of the batch")
    assert verify.xcigar_string(got[4][: int(got[3][1])]) == "".join(f"{n}{'MIDNSHP=X'[op]}" for op, n in want[100][2])


# ------------------------------------------------------------------------------------------------ 2., 3. after the aligner

def _simulated(rng, genome, b, count, m, width, err):
    for _ in range(count):
        rc = int(rng.integers(0, 2))
        start = int(rng.integers(0, len(genome) - width))
        src = genome[start + 1: start + 1 + m]
        q = _mutate(rng, _revcomp(src) if rc else src, *err)[:m]
        if len(q) < m:
            q = np.concatenate([q, rng.choice(list(b"ACGT"), m - len(q)).astype(np.uint8)])
        b.add(q, start, width, rc)


@pytest.fixture(scope="module")
def plain_genome():
    return np.random.default_rng(20250702).choice(list(b"ACGT"), 400_000).astype(np.uint8)


@pytest.mark.gpu
def test_after_the_aligner(plain_genome):
    """2 000 x (300 x 307) and 40 x (10 000 x 11 001) simulated reads on both strands through align, one 70 000-base read
    with substitutions only (one M entry beyond 65 536 columns) through align_long: the restatement's arrays, nm = -score."""
    rng = np.random.default_rng(32)
    b = _Batch()
    _simulated(rng, plain_genome, b, 2000, 300, 307, (0.02, 0.01, 0.01))
    _simulated(rng, plain_genome, b, 40, 10_000, 11_001, (0.03, 0.025, 0.025))
    batch = b.args()
    v = _verifier()
    v.load_genome(plain_genome)
    score, begin, off, cg = v.align(*batch)
    got = v.annotate(*batch, begin, off, cg)
    assert (score < 0).any() and {0, 1, 2} <= set((cg & 15).tolist())
    _assert_annotations(got, _expected(plain_genome, batch, begin, off, cg), "after align")
    assert np.array_equal(got[0].astype(np.int64), -score.astype(np.int64)), "nm is not -score"
    for rc in (0, 1):
        b = _Batch()
        start = 1000 + rc
        src = plain_genome[start + 5: start + 5 + 70_000]
        q = _mutate(rng, _revcomp(src) if rc else src, 0.02, 0, 0)
        b.add(q, start, 70_020, rc)
        batch = b.args()
        score, begin, off, cg = v.align_long(*batch)
        assert len(cg) == 1 and int(cg[0]) == (70_000 << 4 | M)
        got = v.annotate(*batch, begin, off, cg)
        _assert_annotations(got, _expected(plain_genome, batch, begin, off, cg), "after align_long")
        # the read's source lies 5 bases into the window on the forward strand, whichever strand was read: the aligner's
        # begin counts from the other end for rc (70 020 - 5 - 70 000 = 15), the annotated pos does not
        assert int(got[0][0]) == -int(score[0]) > 500
        assert int(begin[0]) == (15 if rc else 5) and int(got[1][0]) == 5 and int(got[2][0]) == 70_000
    v.close()


@pytest.mark.gpu
def test_after_align_bounded(plain_genome):
    """Half the alignments at unrelated places under a bound of 10 %: the rejected come back with zeros and no entries,
    the others as after align."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(33)
    b = _Batch()
    _simulated(rng, plain_genome, b, 600, 300, 307, (0.02, 0.01, 0.01))
    batch = list(b.args())
    batch[1] = np.where(np.arange(600) % 2 == 1, (batch[1] + 150_000) % 390_000, batch[1]).astype(np.uint64)
    v = _verifier()
    v.load_genome(plain_genome)
    score, begin, off, cg = v.align_bounded(*batch, np.full(600, 30, np.uint32))
    rejected = score == verify.REJECTED
    assert 250 < rejected.sum() < 350
    got = v.annotate(*batch, begin, off, cg)
    v.close()
    _assert_annotations(got, _expected(plain_genome, batch, begin, off, cg), "after align_bounded")
    nm, pos, ref_len, xo = got[:4]
    assert not nm[rejected].any() and not pos[rejected].any() and not ref_len[rejected].any()
    assert (np.diff(xo.astype(np.int64))[rejected] == 0).all() and (np.diff(got[5].astype(np.int64))[rejected] == 0).all()
    assert np.array_equal(nm[~rejected].astype(np.int64), -score[~rejected].astype(np.int64))


# ------------------------------------------------------------------------------------------------ 4. refusals

@pytest.mark.gpu
def test_refusals_leave_the_context_usable(plain_genome):
    from bucket_map_amd import verify
    rng = np.random.default_rng(34)
    b = _Batch()
    _simulated(rng, plain_genome, b, 50, 300, 307, (0.02, 0.01, 0.01))
    batch = b.args()
    with pytest.raises(verify.BmvError) as e:
        verify.Verifier().annotate(*batch, np.zeros(50, np.uint32), np.zeros(51, np.uint64), np.zeros(0, np.uint32))
    assert e.value.code == 3                                     # BMV_ERR_STATE: no genome yet
    v = _verifier()
    v.load_genome(plain_genome)
    results = v.align(*batch)
    score, begin, off, cg = results
    good = v.annotate(*batch, begin, off, cg)
    want = _expected(plain_genome, batch, begin, off, cg)
    _assert_annotations(good, want, "before the refusals")
    one = tuple(x[7:8] for x in batch[1:])                       # alignment 7 alone, as alignment 2 of three
    three = (batch[0], *(np.concatenate([x[:2], y]) for x, y in zip(batch[1:], one)))
    head = [_unpack(cg[int(off[a]): int(off[a + 1])]) for a in (0, 1)]
    bad_cigars = {
        "consumes query_len - 1": [(M, 299)],
        "runs past the window": [(M, 300), (D, 8)],
        "a zero-length entry": [(M, 150), (I, 0), (M, 150)],
        "adjacent equal ops": [(M, 150), (M, 150)],
        "an op code of 3": [(M, 150), (3, 2), (M, 150)],
    }
    for what, bad in bad_cigars.items():
        cigs = head + [bad]
        o = np.concatenate([[0], np.cumsum([len(c) for c in cigs])]).astype(np.uint64)
        with pytest.raises(verify.BmvError) as e:
            v.annotate(*three, np.array([begin[0], begin[1], 0], np.uint32), o, np.concatenate([pack(c) for c in cigs]))
        assert e.value.code == 1 and "alignment 2" in str(e.value), (what, str(e.value))
    again = v.annotate(*batch, begin, off, cg)
    _assert_annotations(again, want, "after the refusals")
    import ctypes as C
    s2, b2, o2 = np.zeros(50, np.int32), np.zeros(50, np.uint32), np.zeros(51, np.uint64)
    c2 = np.zeros(len(cg), np.uint32)
    L = verify.lib()
    assert L.bmv_results(v._h, s2.ctypes.data_as(C.POINTER(C.c_int32)), b2.ctypes.data_as(C.POINTER(C.c_uint32)),
                         o2.ctypes.data_as(C.POINTER(C.c_uint64)), c2.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert all(np.array_equal(x, y) for x, y in zip((s2, b2, o2, c2), results)), "annotate changed bmv_results"
    assert v.stats()["cells"] == 50 * 300 * 307
    assert v.annotate(np.zeros(0, np.uint8), [], [], [], [], [], [], [0], [])[3].tolist() == [0]         # n == 0 is fine
    v.close()


# ------------------------------------------------------------------------------------------------ 5. the tool

def _tool(args, cwd):
    exe = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
    r = subprocess.run([exe, *args], cwd=str(cwd), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _records(path):
    return [l.split("\t") for l in open(path).read().split("\n") if l and not l.startswith("@")]


def _fasta(path):
    out, name = {}, None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split(" ")[0]
            out[name] = []
        elif line:
            out[name].append(line)
    return {k: "".join(v) for k, v in out.items()}


def _fastq(path):
    lines = open(path).read().split("\n")
    return {lines[i][1:].split(" ")[0]: (lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 3, 4)}


def _check_annotated(recs, ref, reads):
    """Every annotated record walked from POS over the forward FASTA with SEQ, on folded letters."""
    import re
    fold = lambda s: "".join("ACGT"[rank(ord(c))] for c in s)
    n16 = 0
    for f in recs:
        qname, flag, rname, pos, mapq, cigar, seq, qual = f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[9], f[10]
        tags = dict(t.split(":", 2)[::2] for t in f[11:])
        assert set(tags) == {"NM", "MD"}, f
        chrom, ti, qi = ref[rname], pos - 1, 0
        ops = [(int(n), op) for n, op in re.findall(r"(\d+)([=XID])", cigar)]
        assert "".join(f"{n}{op}" for n, op in ops) == cigar and ops, f"{qname}: CIGAR {cigar}"
        assert all(a[1] != b[1] for a, b in zip(ops, ops[1:])), f"{qname}: adjacent entries of one op in {cigar}"
        nm, md, run = 0, "", 0
        for n, op in ops:
            if op == "I":
                qi += n
                nm += n
                continue
            assert ti + n <= len(chrom), f"{qname}: the CIGAR leaves {rname}"
            t = fold(chrom[ti: ti + n])
            if op == "D":
                md += f"{run}^{t}"
                run = 0
                nm += n
            else:
                q = seq[qi: qi + n]
                assert len(q) == n, f"{qname}: the CIGAR consumes more than SEQ"
                same = [a == b for a, b in zip(t, q)]
                assert all(same) if op == "=" else not any(same), f"{qname}: {n}{op} at {ti} does not hold"
                if op == "=":
                    run += n
                else:
                    for c in t:
                        md += f"{run}{c}"
                        run = 0
                    nm += n
                qi += n
            ti += n
        md += str(run)
        assert qi == len(seq), f"{qname}: the CIGAR consumes {qi} of {len(seq)} bases"
        assert int(tags["NM"]) == nm and tags["MD"] == md, (qname, tags, nm, md)
        assert (60 - nm) % 256 == mapq, (qname, nm, mapq)
        r_seq, r_qual = reads[qname]
        if flag == 16:
            n16 += 1
            assert seq == fold(r_seq).translate(str.maketrans("ACGT", "TGCA"))[::-1] and qual == r_qual[::-1], qname
        else:
            assert flag == 0 and seq == fold(r_seq) and qual == r_qual, qname
    return n16


@pytest.mark.gpu
def test_bucketmap_align_with_annotate(tmp_path):
    """3 000 reads of 150 bases on a synthetic genome, plain and with --annotate: the same records, forward ones at the same
    POS, every annotated record true against the FASTA; two contexts write the same bytes; with --max-edit-rate the bounded
    run's records, annotated."""
    from bucket_map_amd import host
    g = host.Genome.synth(41, [700_000, 250_000])
    g.write_fasta(str(tmp_path / "g.fa"))
    rd = host.Reads(g, 8192, 150, 150, 3000, sub=0.03, ins=0.004, dele=0.004, seed=9)
    rd.write_fastq(str(tmp_path / "r"))
    common = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "8192", "-r", "150", "-f", "1", "-u", "0", "-q", "r.fastq"]
    err_plain = _tool([*common, "-o", "plain.sam"], tmp_path)
    err = _tool([*common, "-o", "ann.sam", "--annotate"], tmp_path)
    assert "GPU alignment annotation" in err and "GPU alignment annotation" not in err_plain
    _tool([*common, "-o", "ann2.sam", "--annotate", "--gpus", "0,0"], tmp_path)
    ref, reads = _fasta(tmp_path / "g.fa"), _fastq(tmp_path / "r.fastq")
    plain, ann = _records(tmp_path / "plain.sam"), _records(tmp_path / "ann.sam")
    head = lambda p: [l for l in open(tmp_path / p).read().split("\n") if l.startswith("@")]
    assert head("plain.sam") == head("ann.sam") and len(plain) == len(ann) > 1000
    assert all(len(f) == 11 for f in plain) and all(len(f) == 13 for f in ann)
    key = lambda f: (f[0], f[1], f[2], f[4])
    assert [key(f) for f in plain] == [key(f) for f in ann]      # the same records in the same order ...
    assert Counter(key(f) for f in plain) == Counter(key(f) for f in ann)
    assert all(p[3] == a[3] for p, a in zip(plain, ann) if p[1] == "0")
    n16 = _check_annotated(ann, ref, reads)
    assert n16 > 300 and any("I" in f[5] for f in ann) and any("D" in f[5] for f in ann) and any("X" in f[5] for f in ann)
    assert (tmp_path / "ann2.sam").read_bytes() == (tmp_path / "ann.sam").read_bytes()
    # a reduced job under an edit bound: the bounded run's records, annotated
    with open(tmp_path / "few.fastq", "w") as f:
        f.write("\n".join(open(tmp_path / "r.fastq").read().split("\n")[: 4 * 600]) + "\n")
    few = [*common[:-1], "few.fastq", "--max-edit-rate", "0.03125"]
    _tool([*few, "-o", "b.sam"], tmp_path)
    _tool([*few, "-o", "b_ann.sam", "--annotate"], tmp_path)
    b_plain, b_ann = _records(tmp_path / "b.sam"), _records(tmp_path / "b_ann.sam")
    assert [key(f) for f in b_plain] == [key(f) for f in b_ann] and 0 < len(b_ann)
    few_names = set(_fastq(tmp_path / "few.fastq"))
    assert len(b_ann) < sum(1 for f in plain if f[0] in few_names), "the bound rejected nothing: the run shows nothing"
    assert all(int(f[11].split(":")[2]) <= int(0.03125 * 150) for f in b_ann)
    _check_annotated(b_ann, ref, reads)
