"""Best alignment per read without a GPU: the contract of bmv_align_best restated in numpy (verify.select_best) against an
independent brute force over the C oracle's alignments, the MAPQ helper (verify.best_mapq, host/best_mapq.h), and the
tools' --best through the oracle-backed tool, whose verifier takes alignment_verifier::best's default (align everything,
select on the host)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle_c as oc

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")
BASES = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _d_end(res):
    """Distances and end columns (begin + M and D lengths) of oracle alignments, one Python loop per alignment."""
    s, b, o, c = res
    d, end = [], []
    for a in range(len(s)):
        r = sum(int(e) >> 4 for e in c[int(o[a]): int(o[a + 1])] if int(e) & 15 != 1)
        d.append(-int(s[a]))
        end.append(int(b[a]) + r)
    return d, end


def _brute(d, end, off, margin):
    """The contract, by the book: per group a sort over (d, index), then the margin."""
    from bucket_map_amd import verify
    winner, edits, out_end = [], [verify.BEYOND] * len(d), [0] * len(d)
    for g in range(len(off) - 1):
        members = list(range(int(off[g]), int(off[g + 1])))
        if not members:
            winner.append(verify.BEYOND)
            continue
        best, w = sorted((d[a], a) for a in members)[0]
        winner.append(w)
        for a in members:
            if d[a] <= best + int(margin[g]):
                edits[a], out_end[a] = d[a], end[a]
    return winner, edits, out_end


def _substituted(seq, n, rng):
    """seq with exactly n substitutions, each to a different base."""
    s = np.array(seq, np.uint8)
    for at in rng.choice(len(s), n, replace=False):
        s[at] = BASES[(int(np.flatnonzero(BASES == s[at])[0]) + 1 + int(rng.integers(0, 3))) % 4]
    return s


def test_header_binding_and_python_surface():
    from bucket_map_amd import verify
    text = open(os.path.join(ROOT, "include", "bmv.h")).read()
    assert re.search(r"#define\s+BMV_BEYOND\s+UINT32_MAX", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = verify.lib()
    for name in ("bmv_align_best", "bmv_best", "bmv_last_best_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
    decl = re.search(r"bmv_align_best\s*\((.*?)\)", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")][-6:] == ["n", "group_offset", "n_groups", "margin", "hint", "total_cigar"]
    assert verify.BEYOND == 2 ** 32 - 1
    for fn in ("align_best", "best_stats"):
        assert callable(getattr(verify.Verifier, fn))
    assert callable(verify.select_best) and callable(verify.best_mapq)
    total = C.c_uint64()
    assert L.bmv_align_best(None, None, 0, None, None, None, None, None, 0, None, 0, None, None, C.byref(total)) == 1
    assert b"bmv_align_best" in L.bmv_last_error()
    assert L.bmv_best(None, None, None, None) == 1 and L.bmv_last_best_stats(None, *[None] * 8) == 1


def test_select_best_against_a_brute_force_over_the_oracle():
    from bucket_map_amd import verify
    rng = np.random.default_rng(20250902)
    genome = rng.choice(list(b"ACGT"), 30_000).astype(np.uint8)
    reads, at = [], 0
    ts, tl, trc, qs, ql, off = [], [], [], [], [], [0]
    for _ in range(300):
        m = int(rng.integers(0, 90)) if rng.random() < 0.9 else 0
        pos = int(rng.integers(100, len(genome) - 300))
        rc = int(rng.integers(0, 2))
        src = genome[pos: pos + m]
        q = _substituted(src, int(rng.integers(0, m // 8 + 1)), rng) if m else src
        if rc:
            q = np.frombuffer(bytes(bytearray(q)).translate(COMP)[::-1], np.uint8)
        reads.append(q)
        for k in range(int(rng.integers(0, 6))):
            kind = int(rng.integers(0, 3))
            start = pos - int(rng.integers(0, 12)) if kind < 2 else int(rng.integers(0, len(genome) - 200))
            ts.append(start); tl.append(m + 1 + int(rng.integers(0, 24))); trc.append(rc if kind else 1 - rc)
            qs.append(at); ql.append(m)
        at += m
        off.append(len(ts))
    res = oc.align_batch(genome, np.concatenate(reads), ts, tl, trc, qs, ql)
    d, end = _d_end(res)
    sizes = np.diff(off)
    assert (sizes == 0).any() and (sizes > 3).any() and (np.array(ql) == 0).any()
    for margin in (np.zeros(300, np.uint32), rng.integers(0, 12, 300).astype(np.uint32), np.full(300, 2 ** 32 - 1, np.uint32)):
        w, e, x = verify.select_best(d, end, off, margin)
        bw, be, bx = _brute(d, end, off, margin)
        assert w.tolist() == bw and e.tolist() == be and x.tolist() == bx
        assert w.dtype == e.dtype == x.dtype == np.uint32


def test_select_best_hand_worked():
    """One 60-base read against copies with exactly 0, 3, 4 and 0 substitutions: a tie (the lowest index wins), a runner-up
    exactly at best + margin and one at best + margin + 1; empty groups; a zero-length query."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(3)
    genome = rng.choice(list(b"ACGT"), 4000).astype(np.uint8)
    read = genome[100:160].copy()
    for k, (at, subs) in enumerate(((1000, 3), (2000, 4), (3000, 0))):
        genome[at: at + 60] = _substituted(read, subs, np.random.default_rng(10 + k))
    win = lambda at: (at - 5, 72)                        # noqa: E731
    ts, tl = zip(*(win(at) for at in (1000, 100, 2000, 3000)))           # group 1: d = 3, 0, 4, 0
    ts, tl = list(ts) + [100, 100], list(tl) + [72, 0]                   # group 3: a zero-length query, twice (one empty text)
    qs, ql = [0] * 4 + [60, 60], [60] * 4 + [0, 0]
    off = [0, 0, 4, 4, 6, 6]                                             # groups 0, 2 and 4 are empty
    res = oc.align_batch(genome, read, ts, tl, [0] * 6, qs, ql)
    d, end = _d_end(res)
    assert d == [3, 0, 4, 0, 0, 0], d
    assert end[:4] == [65, 65, 65, 65] and end[4:] == [72, 0], end       # (the empty query ends at the last column)
    B = verify.BEYOND
    w, e, x = verify.select_best(d, end, off, [9, 3, 9, 0, 9])
    assert w.tolist() == [B, 1, B, 4, B]                                 # index 1 beats its equal at index 3
    assert e.tolist() == [3, 0, B, 0, 0, 0] and x.tolist() == [65, 65, 0, 65, 72, 0]
    w, e, x = verify.select_best(d, end, off, [0, 4, 0, 0, 0])
    assert e.tolist() == [3, 0, 4, 0, 0, 0]
    w, e, x = verify.select_best(d, end, off, [0, 2, 0, 0, 0])
    assert w.tolist() == [B, 1, B, 4, B] and e.tolist() == [B, 0, B, 0, 0, 0] and x.tolist() == [0, 65, 0, 65, 72, 0]
    assert _brute(d, end, off, [0, 2, 0, 0, 0]) == (w.tolist(), e.tolist(), x.tolist())
    with pytest.raises(ValueError):
        verify.select_best(d, end, [0, 4, 3, 6], [0, 0, 0])


def test_best_mapq():
    from bucket_map_amd import verify
    B = verify.BEYOND
    # unique: nothing else within the margin
    assert verify.best_mapq(0, [2, B, B], [150, 0, 0], [1000, 5000, 9000], [160] * 3, [0, 0, 0], 7) == (60, 1)
    assert verify.best_mapq(0, [2], [150], [1000], [160], [1], 7) == (60, 1)
    # a second locus at e1
    assert verify.best_mapq(0, [2, 2], [150, 150], [1000, 5000], [160, 160], [0, 0], 7) == (0, 2)
    # the same locus through two overlapping windows does not count: forward 1000 + 150 = 990 + 160 ...
    assert verify.best_mapq(0, [2, 2], [150, 160], [1000, 990], [160, 170], [0, 0], 7) == (60, 1)
    # ... and reverse: 1000 + 160 - 150 = 1004 + 160 - 154; the other strand at the same number is another locus
    assert verify.best_mapq(1, [2, 2], [150, 154], [1000, 1004], [160, 160], [1, 1], 7) == (60, 1)
    assert verify.best_mapq(0, [2, 2], [150, 150], [1000, 1000], [160, 160], [0, 1], 7) == (0, 2)
    # the same second locus twice is one locus; a third one makes X0 3
    assert verify.best_mapq(0, [2, 2, 2, 2], [150, 150, 140, 150], [1000, 5000, 5010, 9000], [160] * 4, [0] * 4, 7) == (0, 3)
    # the integer formula at e2 - e1 = 1 and at e2 - e1 = M, M = 7: 60 / 8 and 7 * 60 / 8
    assert verify.best_mapq(0, [2, 3], [150, 150], [1000, 5000], [160, 160], [0, 0], 7) == (7, 1)
    assert verify.best_mapq(0, [2, 9, 5], [150, 150, 150], [1000, 5000, 9000], [160] * 3, [0] * 3, 7)[0] == 3 * 60 // 8
    assert verify.best_mapq(1, [9, 2], [150, 150], [1000, 5000], [160, 160], [0, 0], 7) == (52, 1)
    assert verify.best_mapq(0, [0, 1], [150, 150], [1000, 5000], [160, 160], [0, 0], 0) == (60, 1)     # M = 0: only ties count


@pytest.fixture(scope="module")
def duplicated(tmp_path_factory):
    """A 30-kbp record and a second one holding a copy of 12 kbp of it, half of it exact and half diverged by 1 %; 150 reads
    of 150 bases from the first record, every other one reverse-complemented."""
    d = tmp_path_factory.mktemp("best")
    rng = np.random.default_rng(5)

    def mutate(seq, rate):
        s = seq.copy()
        hit = rng.random(len(s)) < rate
        s[hit] = BASES[rng.integers(0, 4, int(hit.sum()))]
        return s
    a = BASES[rng.integers(0, 4, 30_000)]
    b = np.concatenate([BASES[rng.integers(0, 4, 3000)], a[5000:11000], mutate(a[11000:17000], 0.01), BASES[rng.integers(0, 4, 2000)]])
    with open(d / "g.fa", "w") as f:
        f.write(f">chrA\n{bytes(a).decode()}\n>chrB\n{bytes(b).decode()}\n")
    with open(d / "reads.fastq", "w") as f:
        for i in range(150):
            p = int(rng.integers(0, 30_000 - 160)) if i % 3 else int(rng.integers(5000, 16_800))
            s = bytes(mutate(a[p: p + 150], 0.02))
            if i % 2:
                s = s.translate(COMP)[::-1]
            f.write(f"@r{i}\n{s.decode()}\n+\n{'I' * 150}\n")
    return d


ARGS = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "4096", "-r", "150", "-f", "1", "-q", "reads.fastq"]


def _tool(d, out, *extra, dump=None, ok=True):
    env = dict(os.environ, BM_VERIFY_BLOCK_READS="37")
    if dump:
        env["BM_DUMP_ALIGNMENTS"] = str(d / dump)
    r = subprocess.run([TOOL, *ARGS, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def expected_best_records(plain_sam, plain_dump, rate, u=40, max_edit_rate=None):
    """What --best must write, from a run WITHOUT it: the dump lists every alignment in record order (read, text start,
    text length, strand, query length, score, begin, CIGAR), the SAM file a record for each that passes the MAPQ rule.  Returns
    (records, winners' dump lines): per read the winner's record with MAPQ and X0 from the helper."""
    from bucket_map_amd import verify
    rows = [l.split() for l in plain_dump.split("\n") if l]
    recs = [l for l in plain_sam.split("\n") if l and not l.startswith("@")]
    written = [not ((60 + int(r[5])) % 2 ** 32 < u) for r in rows]
    assert sum(written) == len(recs)
    rec_of, k = {}, 0
    for a, w in enumerate(written):
        if w:
            rec_of[a] = recs[k]
            k += 1
    reads = sorted({int(r[0]) for r in rows})
    d = [-int(r[5]) for r in rows]
    end = []
    for r in rows:
        ops = re.findall(r"(\d+)([MID])", r[7])
        end.append(int(r[6]) + sum(int(n) for n, op in ops if op != "I"))
    off = [0]
    for read in reads:
        off.append(off[-1] + sum(1 for r in rows if int(r[0]) == read))
    assert [int(r[0]) for r in rows] == sorted(int(r[0]) for r in rows)
    margin = [max(1, int(np.float32(rate) * np.float32(int(rows[off[g]][4])))) for g in range(len(reads))]
    winner, edits, out_end = verify.select_best(d, end, off, margin)
    out, dump = [], []
    for g, w in enumerate(winner):
        a0, a1 = off[g], off[g + 1]
        w = int(w)
        dump.append(" ".join(rows[w]))
        if not written[w]:
            continue
        if max_edit_rate is not None and d[w] > int(np.float32(max_edit_rate) * np.float32(int(rows[w][4]))):
            continue
        mapq, x0 = verify.best_mapq(w - a0, edits[a0:a1], out_end[a0:a1], [int(r[1]) for r in rows[a0:a1]],
                                    [int(r[2]) for r in rows[a0:a1]], [int(r[3]) for r in rows[a0:a1]], margin[g])
        f = rec_of[w].split("\t")
        f[4] = str(mapq)
        out.append("\t".join(f + [f"X0:i:{x0}"]))
    return out, dump, np.diff(off)


def test_tool_writes_the_winner_with_its_mapq(duplicated):
    d = duplicated
    _tool(d, "plain.sam", dump="plain.txt")
    plain = open(d / "plain.sam").read()
    for name, extra, rate, bound in (("best", ["--best"], 0.05, None), ("wide", ["--best-margin", "0.1"], 0.1, None),
                                     ("zero", ["--best-margin=0"], 0.0, None),
                                     ("bounded", ["--best", "--max-edit-rate", "0.02"], 0.05, 0.02)):
        _tool(d, f"{name}.sam", *extra, dump=f"{name}.txt")
        got = open(d / f"{name}.sam").read().split("\n")
        want, dump, sizes = expected_best_records(plain, open(d / "plain.txt").read(), rate, max_edit_rate=bound)
        assert (sizes > 1).sum() >= 10, "the fixture has too few reads with several candidates: the test shows nothing"
        assert [l for l in got if l.startswith("@")] == [l for l in plain.split("\n") if l.startswith("@")]
        recs = [l for l in got if l and not l.startswith("@")]
        names = [l.split("\t")[0] for l in recs]
        assert len(names) == len(set(names)), "more than one record for a read"
        assert recs == want
        if bound is None:
            assert open(d / f"{name}.txt").read().split("\n")[:-1] == dump
        mapqs = {l.split("\t")[4] for l in recs}
        if name == "best":
            assert "0" in mapqs and "60" in mapqs and any("X0:i:2" in l for l in recs)
        if name == "bounded":
            assert len(recs) < len([l for l in open(d / "best.sam").read().split("\n") if l and not l.startswith("@")])
    # without the option the file is what it was
    _tool(d, "again.sam")
    assert open(d / "again.sam").read() == plain


def test_negative_margin_is_refused(duplicated):
    for bad in (["--best-margin", "-0.1"], ["--best-margin=-1"], ["--best-margin", "nan"], ["--best-margin", "x"]):
        r = _tool(duplicated, "never.sam", *bad, ok=False)
        assert "Value parse failed for --best-margin" in r.stderr and not os.path.exists(duplicated / "never.sam")
    r = _tool(duplicated, "never.sam", "--best-margin", ok=False)
    assert "Missing value for option --best-margin" in r.stderr
