"""Paired-end reads on the GPU: the pair kernel (bmv_pair) against the plain-numpy contract verify.select_pairs on hand-built
numbers, bmv_align_paired against Verifier.align_long on the whole batch plus select_best and select_pairs -- exactly, whatever
the hint and whichever path the alignments take --, bmv_align_best on the same batch after the refactor, and the tool against
the oracle-backed tool."""
import os
import subprocess

import numpy as np
import pytest

from test_best_gpu import _assert_best, _mutate, _reference, _revcomp
from test_pair import ARGS, assert_pairs_equal, edge_cases, flatten, make_paired_fixture, random_pairs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GPU_TOOL = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
ORACLE_TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")
SIZES = (0, 1, 2, 63, 64, 65, 130)


def _arrays(ts, tl, trc, ql, ed, en, off):
    return (np.array(ts, np.uint64), np.array(tl, np.uint32), np.array(trc, np.uint8), np.array(ql, np.uint32),
            np.array(ed, np.uint32), np.array(en, np.uint32), np.array(off, np.uint32))


def _check(v, arrays, lo, hi, contig, what):
    from bucket_map_amd import verify
    ts, tl, trc, ql, ed, en, off = arrays
    got = v.pair(ts, tl, trc, ql, ed, en, off, lo, hi, contig)
    want = verify.select_pairs(ts, tl, trc, ql, ed, en, off, lo, hi, contig)
    assert_pairs_equal(got, want, what)
    sizes = np.diff(off.astype(np.int64))
    assert v.pair_stats()["combinations"] == int((sizes[0::2] * sizes[1::2]).sum())
    return got


def _sized_pairs():
    """Every ordered pair of group sizes out of SIZES, all combinations proper (mate 1 forward around 1 000, mate 2 reverse
    ending around 1 400 .. 1 530), edits 5 .. 20 but for ONE alignment per mate with 0: the unique minimum, at the first, the
    last, the 64th and the 65th index of its group wherever the group has them."""
    rng = np.random.default_rng(20251002)
    ts, tl, trc, ql, ed, en, off, where = [], [], [], [], [], [], [0], []
    spots = lambda size: sorted({x for x in (0, size - 1, 63, 64) if 0 <= x < size}) or [None]      # noqa: E731
    for sa in SIZES:
        for sb in SIZES:
            for pa in spots(sa):
                for pb in spots(sb):
                    for size, at, rc in ((sa, pa, 0), (sb, pb, 1)):
                        for k in range(size):
                            m = 100
                            left = 1000 + k if rc == 0 else 1300 + k
                            ts.append(left - (10 if rc else 5)); tl.append(m + 15); en.append(m + 5)       # L = left on either strand
                            trc.append(rc); ql.append(m)
                            ed.append(0 if k == at else int(rng.integers(5, 21)))
                        off.append(len(ts))
                    where.append((sa, sb, pa, pb))
    return _arrays(ts, tl, trc, ql, ed, en, off), where


@pytest.mark.gpu
def test_pair_kernel_over_group_sizes():
    """Groups of 0, 1, 2, 63, 64, 65 and 130 candidates in every order -- one lane chunk, exactly one, one and a lane, three --
    with the unique minimum at the chunk borders of either mate; 130 x 130 is more than 64 x 64 combinations in one pair."""
    from bucket_map_amd import verify
    arrays, where = _sized_pairs()
    v = verify.Verifier()
    got = _check(v, arrays, 200, 800, None, "sizes")
    off = arrays[6].astype(np.int64)
    for p, (sa, sb, pa, pb) in enumerate(where):
        if sa and sb:
            assert got["proper"][p] == 1 and got["s1"][p] == 0
            assert got["pick"][2 * p] == off[2 * p] + pa and got["pick"][2 * p + 1] == off[2 * p + 1] + pb, (sa, sb, pa, pb)
            assert (got["s2"][p] == verify.PAIR_NONE) == (sa == 1 and sb == 1)
        else:
            assert got["proper"][p] == 0 and got["s1"][p] == verify.PAIR_NONE
    # nothing but ties, behind a run of unknown candidates that is longer than a lane chunk: the first known (i, j) wins
    ts, tl, trc, ql, ed, en, off = (x.copy() for x in arrays)
    p = where.index((130, 130, 0, 0))
    a0, b0, b1 = int(off[2 * p]), int(off[2 * p + 1]), int(off[2 * p + 2])
    ed[a0:b1] = 3
    ed[a0: a0 + 70] = verify.BEYOND
    ed[b0: b0 + 66] = verify.BEYOND
    got = _check(v, (ts, tl, trc, ql, ed, en, off), 200, 800, None, "ties")
    assert got["pick"][2 * p] == a0 + 70 and got["pick"][2 * p + 1] == b0 + 66 and got["s1"][p] == got["s2"][p] == 6
    assert got["winner"][2 * p] == a0 + 70 and got["winner"][2 * p + 1] == b0 + 66
    # only the LAST combination is proper (every other candidate on another contig)
    ctg = np.zeros(len(ts), np.uint32)
    ctg[a0: b0 - 1] = 1
    ctg[b0: b1 - 1] = 2
    got = _check(v, (ts, tl, trc, ql, ed, en, off), 200, 800, ctg, "the last combination")
    assert got["pick"][2 * p] == b0 - 1 and got["pick"][2 * p + 1] == b1 - 1 and got["s2"][p] == verify.PAIR_NONE
    v.close()


@pytest.mark.gpu
def test_pair_kernel_edge_cases_and_random_pairs():
    from bucket_map_amd import verify
    v = verify.Verifier()
    cases = edge_cases()
    arrays = _arrays(*flatten(cases.values()))
    got = _check(v, arrays, 200, 500, None, "edge cases")
    assert dict(zip(cases, got["proper"].tolist()))["negative L"] == 1
    ctg = np.zeros(len(arrays[0]), np.uint32)
    ctg[arrays[6][1]] = 7
    assert _check(v, arrays, 200, 500, ctg, "edge cases, contigs")["proper"][0] == 0
    rng = np.random.default_rng(20251001)
    ts, tl, trc, ql, ed, en, ctg, off = random_pairs(rng, 400)                    # the CPU test's pairs
    for contig in (np.array(ctg, np.uint32), None):
        for lo, hi in ((1, 1000), (300, 600), (0, 2 ** 32 - 1)):
            _check(v, _arrays(ts, tl, trc, ql, ed, en, off), lo, hi, contig, f"the CPU test's pairs, {lo}..{hi}")
    ts, tl, trc, ql, ed, en, ctg, off = random_pairs(np.random.default_rng(20251003), 1000, sizes=(0, 1, 2, 3, 4, 7, 20, 70))
    got = _check(v, _arrays(ts, tl, trc, ql, ed, en, off), 1, 1000, np.array(ctg, np.uint32), "1 000 random pairs")
    assert got["proper"].sum() > 200 and (got["pick"] != got["winner"]).sum() > 50
    # refusals: nothing ran, the context stays usable
    arrays = _arrays(ts, tl, trc, ql, ed, en, off)
    odd = np.append(arrays[6], arrays[6][-1])                                     # one more, empty, group
    for bad, words in (((*arrays[:6], odd), "groups"), (arrays, "min_frag")):
        with pytest.raises(verify.BmvError) as e:
            v.pair(*bad, 900 if words == "min_frag" else 1, 800)
        assert e.value.code == 1 and words in str(e.value)
    assert_pairs_equal(v.pair(*arrays, 1, 1000, np.array(ctg, np.uint32)), got, "after the refusals")
    empty = v.pair(*(np.zeros(0, t) for t in (np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint32)), np.zeros(1, np.uint32), 1, 1000)
    assert all(len(x) == 0 for x in empty.values())
    v.close()


def build_pairs_batch():
    """About 300 pairs of 100 .. 300-base reads from fragments of 250 .. 750 bases of a 30-kbp genome with two planted repeats
    (2 kbp exact, 1.5 kbp diverged by 1 %); per mate the true window, the copy's where there is one, and decoys (the other
    strand, a shifted window, a random place); group sizes 0 .. 5.  Returns (genome, batch, group offsets, margins)."""
    rng = np.random.default_rng(20251004)
    genome = rng.choice(list(b"ACGT"), 30_000).astype(np.uint8)
    genome[20_000:22_000] = genome[5_000:7_000]
    genome[25_000:26_500] = _mutate(rng, genome[10_000:11_500], 0.01, 0, 0)
    copies = ((5_000, 20_000, 2_000), (10_000, 25_000, 1_500))
    reads, at = [], 0
    ts, tl, trc, qs, ql, off = [], [], [], [], [], [0]
    for p in range(300):
        frag = int(rng.integers(250, 751))
        s = int(rng.integers(200, len(genome) - frag - 400)) if p % 3 else int(rng.integers(4_800, 6_900))
        flip = int(rng.integers(0, 2))                         # which mate is the forward read
        for mate in range(2):
            m = min(int(rng.integers(100, 301)), frag)
            forward = (mate == 0) != bool(flip)
            pos = s if forward else s + frag - m
            src = genome[pos: pos + m + 8]
            q = _mutate(rng, src, 0.02, 0.004, 0.004)[:m]
            if len(q) < m:
                q = np.concatenate([q, rng.choice(list(b"ACGT"), m - len(q)).astype(np.uint8)])
            rc = 0 if forward else 1
            if rc:
                q = _revcomp(_mutate(rng, genome[pos: pos + m], 0.02, 0, 0))
            reads.append(q)
            slack = m // 20 + 6
            width = m + 1 + slack
            cands = [(pos - int(rng.integers(0, slack)), width, rc)]
            for a, b, n in copies:
                for here, there in ((a, b), (b, a)):
                    if here <= pos and pos + m <= here + n:
                        cands.append((there + (pos - here) - slack // 2, width, rc))
            cands += [(pos - slack // 2, width, 1 - rc), (pos - int(rng.integers(0, slack)), width, rc),
                      (int(rng.integers(0, len(genome) - width)), width, int(rng.integers(0, 2)))]
            size = int(rng.integers(0, 6))
            for k in rng.permutation(min(size, len(cands))):
                start, w, r = cands[k]
                ts.append(max(start, 0)); tl.append(w); trc.append(r); qs.append(at); ql.append(len(q))
            at += len(q)
            off.append(len(ts))
    batch = (np.concatenate(reads), np.array(ts, np.uint64), np.array(tl, np.uint32), np.array(trc, np.uint8),
             np.array(qs, np.uint64), np.array(ql, np.uint32))
    off = np.array(off, np.uint32)
    margin = np.array([max(1, int(ql[off[g]]) // 20) if off[g + 1] > off[g] else 1 for g in range(len(off) - 1)], np.uint32)
    return genome, batch, off, margin


@pytest.fixture(scope="module")
def pairs_batch():
    """build_pairs_batch() with a verifier that holds its genome; the reference (align_long on the whole batch) is computed once."""
    from bucket_map_amd import verify
    genome, batch, off, margin = build_pairs_batch()
    v = verify.Verifier()
    v.load_genome(genome)
    ref, d, end = _reference(v, batch)
    return {"v": v, "batch": batch, "off": off, "ref": ref, "d": d, "end": end, "margin": margin}


def _assert_paired(got, pb, lo, hi, contig, what):
    from bucket_map_amd import verify
    batch, off, margin = pb["batch"], pb["off"], pb["margin"]
    s2, b2, o2, c2 = pb["ref"]
    winner, edits, out_end = verify.select_best(pb["d"], pb["end"], off, margin)
    want = verify.select_pairs(batch[1], batch[2], batch[3], batch[5], edits, out_end, off, lo, hi, contig)
    assert_pairs_equal(got, want, what)
    assert np.array_equal(got["winner"], winner) and np.array_equal(got["edits"], edits) and np.array_equal(got["end"], out_end), what
    n = len(pb["d"])
    s, b, o, c = got["score"], got["begin"], got["cigar_offset"], got["cigar"]
    picked = np.zeros(n, bool)
    picked[want["pick"][want["pick"] != verify.BEYOND]] = True
    lens = np.diff(o.astype(np.int64))
    assert o[0] == 0 and o[n] == len(c), f"{what}: total_cigar is not the sum of the picks' CIGARs"
    assert (s[~picked] == verify.REJECTED).all() and (b[~picked] == 0).all() and (lens[~picked] == 0).all(), \
        f"{what}: an alignment that was not picked carries a result"
    assert np.array_equal(s[picked], s2[picked]) and np.array_equal(b[picked], b2[picked]), f"{what}: picks' scores or begins differ"
    assert np.array_equal(lens[picked], np.diff(o2.astype(np.int64))[picked]), f"{what}: picks' CIGAR lengths differ"
    for a in np.flatnonzero(picked):
        assert np.array_equal(c[o[a]: o[a + 1]], c2[o2[a]: o2[a + 1]]), f"{what}: CIGAR of pick {a} differs"
    return want


@pytest.mark.gpu
def test_align_paired_is_exact_whatever_the_hint(pairs_batch, monkeypatch):
    pb = pairs_batch
    v, batch, off, margin = pb["v"], pb["batch"], pb["off"], pb["margin"]
    sizes = np.diff(off.astype(np.int64))
    some = np.maximum(sizes, 1)
    rng = np.random.default_rng(6)
    hints = (("none", None), ("zero", np.zeros(len(sizes), np.uint32)), ("last", (some - 1).astype(np.uint32)),
             ("random", (rng.integers(0, 1 << 30, len(sizes)) % some).astype(np.uint32)))
    contig = (batch[1] >= 15_000).astype(np.uint32)
    for ctg_name, ctg in (("one contig", None), ("two contigs", contig)):
        first = None
        for name, hint in hints:
            got = v.align_paired(*batch, off, margin, 200, 800, hint, ctg)
            want = _assert_paired(got, pb, 200, 800, ctg, f"{ctg_name}, hint {name}")
            print(f"{ctg_name}, hint {name}: {v.best_stats()} {v.pair_stats()}")
            if first is None:
                first = got
                assert want["proper"].sum() > 100 and (want["pick"] != want["winner"]).sum() >= 5, \
                    "the fixture shows nothing: too few proper pairs, or the pick is always the own winner"
                assert (want["s2"] != 2 ** 64 - 1).sum() >= 5
            for key in first:
                assert np.array_equal(first[key], got[key]), f"{ctg_name}: {key} depends on the hint ({name})"
        # every query of 200 bases and more through the long path: the same results
        monkeypatch.setenv("BMV_LONG_FROM", "200")
        got = v.align_paired(*batch, off, margin, 200, 800, None, ctg)
        monkeypatch.delenv("BMV_LONG_FROM")
        for key in first:
            assert np.array_equal(first[key], got[key]), f"{ctg_name}: {key} differs with BMV_LONG_FROM=200"
    # refusals leave the context usable
    from bucket_map_amd import verify
    with pytest.raises(verify.BmvError) as e:
        v.align_paired(*batch, np.append(off, off[-1]), np.append(margin, 1).astype(np.uint32), 200, 800)      # an odd number of groups
    assert e.value.code == 1 and "groups" in str(e.value)
    with pytest.raises(verify.BmvError) as e:
        v.align_paired(*batch, off, margin, 801, 800)
    assert e.value.code == 1 and "min_frag" in str(e.value)
    again = v.align_paired(*batch, off, margin, 200, 800, None, contig)
    for key in first:
        assert np.array_equal(first[key], again[key]), f"{key} differs after the refusals"


@pytest.mark.gpu
def test_align_best_on_the_same_batch_is_what_it_was(pairs_batch):
    """bmv_align_best shares its first three rounds with bmv_align_paired since the refactor: the same batch through it, held
    against select_best as tests/test_best_gpu.py holds it, before and after a paired call on the same context."""
    pb = pairs_batch
    v, batch, off, margin = pb["v"], pb["batch"], pb["off"], pb["margin"]
    before = v.align_best(*batch, off, margin)
    _assert_best(before, pb["ref"], pb["d"], pb["end"], off, margin, "align_best")
    v.align_paired(*batch, off, margin, 200, 800)
    pairs = v._pairs(len(off) - 1)
    after = v.align_best(*batch, off, margin, (np.maximum(np.diff(off.astype(np.int64)), 1) - 1).astype(np.uint32))
    _assert_best(after, pb["ref"], pb["d"], pb["end"], off, margin, "align_best after align_paired")
    for key in before:
        assert np.array_equal(before[key], after[key])
    assert_pairs_equal(v._pairs(len(off) - 1), pairs, "bmv_pairs after an align_best")


@pytest.mark.gpu
def test_tool_equals_the_oracle_backed_tool(tmp_path):
    """bucketmap_align --paired writes, byte for byte, what the oracle-backed tool writes on the CPU test's files -- whose
    verifier aligns everything and picks on the host and whose records are annotated on the host --; --gpus 0,0 writes the
    same bytes."""
    d = tmp_path
    make_paired_fixture(d)

    def tool(exe, fastq, out, *extra):
        env = dict(os.environ, BM_VERIFY_BLOCK_READS="6")
        r = subprocess.run([exe, *ARGS, "-q", fastq, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        return (d / out).read_bytes(), r.stderr

    (d / "rest.fastq").write_text((d / "unique.fastq").read_text() + (d / "lonely.fastq").read_text())
    for fastq, name, extra, twice in (("pairs.fastq", "range", ["--frag-range", "300,800"], True),
                                      ("pairs.fastq", "bounded", ["--paired", "--max-edit-rate", "0.1"], False),
                                      ("rest.fastq", "rest", ["--paired"], False)):
        cpu, _ = tool(ORACLE_TOOL, fastq, f"cpu_{name}.sam", *extra)
        gpu, err = tool(GPU_TOOL, fastq, f"gpu_{name}.sam", *extra)
        assert "best per pair" in err
        assert gpu == cpu, f"{fastq} {extra}"
        if twice:
            two, _ = tool(GPU_TOOL, fastq, f"gpu2_{name}.sam", *extra, "--gpus", "0,0")
            assert two == gpu, f"{fastq} {extra}: --gpus 0,0 differs from --gpus 0"
    recs = [l.split("\t") for l in (d / "gpu_range.sam").read_text().split("\n") if l and not l.startswith("@")]
    assert len(recs) == 48 and all(int(r[1]) & 0x3 == 0x3 and r[4] == "60" for r in recs)
