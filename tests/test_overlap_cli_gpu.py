"""`bucketmap_align --clip-overlap` on the GPU: a small simulated genome with planted SNVs, a few thousand interleaved 2 x 100 bp
pairs on fragments of 120 to 180 bases, run with --paired once without and once with the option, plain (SAM) and with
--clip --affine --left-align --rescue --markdup -o x.bam --depth --pileup --vcf --vcf-indels.

1. The records of the run WITH the option are derived from the run WITHOUT it: the pairs written as 0x2 on one reference whose
   spans overlap without containment are counted from the parent's records alone, the Python rule (overlap_rule.cut) applied to
   them gives POS, CIGAR, NM, MD, AS, PNEXT and TLEN of the other run, everything else is equal, and stderr names that count.
2. With the option no reference position lies under both records of a pair, the depth file never exceeds the simulated
   fragments over a position, and --markdup marks the same records.
3. An error planted at one fragment position in both mates is a pileup site with alt count 2 without the option and no site
   with it.
4. Pairs on fragments of more than twice the read length: the two runs write identical files."""
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_rule
from overlap_rule import NO_MATE
from test_annotate import D, EQ, I, X
from test_bgzf import bam_to_sam

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EXE = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
COMP = bytes.maketrans(b"ACGT", b"TGCA")
READ = 100
N_PAIRS = 3000
ARGS = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "8192", "-r", "100", "-f", "1", "-u", "0"]
FULL = ["--clip", "--affine", "--left-align", "--rescue", "--markdup", "--depth", "{s}.bedgraph", "--pileup", "{s}.tsv", "--vcf", "{s}.vcf",
        "--vcf-indels", "--pileup-min-alt", "2", "--pileup-min-frac", "0.01"]
OPS = "MIDNSHP=X"


def _tool(args, cwd):
    r = subprocess.run([EXE, *args], cwd=str(cwd), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stderr


def _simulate(d, seed, n_pairs, frag_lo, frag_hi, fastq, planted=True):
    """Writes g.fa (once) and an interleaved FASTQ file of pairs drawn from a sample that differs from the reference at a few
    SNVs.  Returns the fragments as (contig index, start, length) and the planted errors as (contig index, position)."""
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", np.uint8)
    ref = [bases[np.random.default_rng(90 + c).integers(0, 4, n)] for c, n in enumerate((50_000, 30_000))]
    if not os.path.exists(d / "g.fa"):
        with open(d / "g.fa", "w") as f:
            for c, r in enumerate(ref):
                f.write(f">chr{c}\n{bytes(r).decode()}\n")
    sample = [r.copy() for r in ref]
    snv = [set(int(x) for x in np.random.default_rng(95 + c).choice(len(r), 12, replace=False)) for c, r in enumerate(ref)]
    for c, at in enumerate(snv):
        for p in at:
            sample[c][p] = bases[(int(np.searchsorted(bases, ref[c][p])) + 1) % 4]
    frags, errors, taken, planted_in = [], [], set(), set()
    for k in range(n_pairs):
        if k % 100 == 99:                                       # an exact copy of the fragment before: a duplicate for --markdup
            c, g0, L = frags[-1]
        else:
            c = int(rng.integers(0, 2))
            L = int(rng.integers(frag_lo, frag_hi + 1))
            g0 = int(rng.integers(0, len(ref[c]) - L))
        frags.append((c, g0, L))
        x = g0 + L // 2                                         # under both mates: L - READ <= L // 2 < READ
        if planted and k % 50 == 0 and L < 2 * READ and (c, x) not in taken and x not in snv[c]:
            errors.append((c, x))
            taken.add((c, x))
            planted_in.add(k)
    with open(d / fastq, "w") as f:
        for k, (c, g0, L) in enumerate(frags):
            frag = sample[c][g0: g0 + L].copy()
            m1, m2 = frag[:READ].copy(), frag[L - READ:].copy()
            if k % 4 == 1:                                       # sequencing errors, independent in the two mates, none at a planted place
                for m, lo in ((m1, g0), (m2, g0 + L - READ)):
                    for x in np.flatnonzero(rng.random(READ) < 0.01):
                        if (c, lo + int(x)) not in taken:
                            m[x] = bases[(int(np.searchsorted(bases, m[x])) + 1 + int(rng.integers(0, 3))) % 4]
            x = L // 2
            if k in planted_in:
                alt = bases[(int(np.searchsorted(bases, frag[x])) + 2) % 4]
                m1[x] = alt                                      # one error of the library preparation, seen by both mates
                m2[x - (L - READ)] = alt
            s1, s2 = bytes(m1), bytes(m2).translate(COMP)[::-1]
            if k % 2:
                s1, s2 = s2, s1
            f.write(f"@f{k}/1\n{s1.decode()}\n+\n{'I' * READ}\n@f{k}/2\n{s2.decode()}\n+\n{'I' * READ}\n")
    return frags, errors


def _records(sam_text):
    return [l.split("\t") for l in sam_text.split("\n") if l and not l.startswith("@")]


def _by_name(recs):
    """(QNAME, first or second mate) -> record; a record per mate at the most (--paired writes one)."""
    out = {}
    for f in recs:
        key = (f[0], bool(int(f[1]) & 0x80))
        assert key not in out, key
        out[key] = f
    return out


def _columns(f):
    """Of a record: (soft clip left, the kept columns' ops, soft clip right, the reference letters under X and D)."""
    parts = [(int(n), OPS.index(op)) for n, op in re.findall(r"(\d+)([=XIDSM])", f[5])]
    left = parts[0][0] if parts[0][1] == 4 else 0
    right = parts[-1][0] if len(parts) > 1 and parts[-1][1] == 4 else 0
    cols = [op for n, op in parts if op != 4 for _ in range(n)]
    md = next(t[5:] for t in f[11:] if t.startswith("MD:Z:"))
    return left, cols, right, re.sub(r"[\d^]", "", md)


def _derive(f, l, r, match, penalty, affine):
    """What the rule makes of record f when it keeps the columns [l, r) of its kept part: (POS, CIGAR, NM, MD, AS or None)."""
    left, cols, right, ref = _columns(f)
    before, kept, after = cols[:l], cols[l:r], cols[r:]
    left += sum(1 for op in before if op != D)
    right += sum(1 for op in after if op != D)
    runs = []
    for op in kept:
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    cigar = (f"{left}S" if left else "") + "".join(f"{n}{OPS[op]}" for op, n in runs) + (f"{right}S" if right else "")
    at = sum(1 for op in before if op in (X, D))
    md, run = "", 0
    for op, n in runs:
        if op == EQ:
            run += n
        elif op == X:
            for k in range(n):
                md += f"{run}{ref[at + k]}"
                run = 0
            at += n
        elif op == D:
            md += f"{run}^{ref[at: at + n]}"
            run = 0
            at += n
    n_eq = sum(1 for op in kept if op == EQ)
    score = None
    if match:
        score = match * n_eq - penalty * (len(kept) - n_eq)
    elif affine:                                                 # sam_tags::affine_score of the written entries, 1,4,6,1
        score = sum(n if op == EQ else -4 * n if op == X else -(6 + n) for op, n in runs)
    return int(f[3]) + sum(1 for op in before if op != I), cigar, len(kept) - n_eq, md + str(run), score


def _span(f):
    _, cols, _, _ = _columns(f)
    return int(f[3]), int(f[3]) + sum(1 for op in cols if op != I)


def _check_derivation(without, with_, err, n_pairs, scores, affine):
    """1. of the module's text.  Returns the records of the run with the option by (QNAME, mate)."""
    a, b = _by_name(without), _by_name(with_)
    assert a.keys() == b.keys(), "which records exist changed"
    keys = sorted(a, key=lambda k: (int(k[0][1:]), k[1]))
    index = {k: i for i, k in enumerate(keys)}
    # the batch order of the tool: the picks in read order, rescued alignments behind them
    order = sorted(keys, key=lambda k: (any(t == "XR:i:1" for t in a[k][11:]), index[k]))
    slot = {k: i for i, k in enumerate(order)}
    cols, g, rng, mate, contig = [], [], [], [NO_MATE] * len(order), []
    overlapping = 0
    for k in order:
        f = a[k]
        _, c, _, _ = _columns(f)
        cols.append(c)
        g.append(overlap_rule.positions(c, int(f[3])))
        rng.append((0, len(c)))
        contig.append(f[2])
        other = (k[0], not k[1])
        if int(f[1]) & 0x2 and other in a and int(a[other][1]) & 0x2:
            mate[slot[k]] = slot[other]
            if not k[1] and f[2] == a[other][2]:                # counted from the parent's records alone
                (p0, e0), (p1, e1) = sorted([_span(f), _span(a[other])])
                overlapping += p1 < e0 <= e1
    final, clipped, role, m, pairs_cut = overlap_rule.cut(cols, g, rng, mate, contig)
    assert overlapping * 2 >= n_pairs, f"{overlapping} of {n_pairs} simulated pairs overlap as records: the simulation shows little"
    assert pairs_cut == overlapping, "the rule cuts other pairs than those that overlap without containment"
    told = re.search(r"Overlap: (\d+) of (\d+) pairs cut, (\d+) bases clipped", err)
    assert told and int(told.group(1)) == overlapping and int(told.group(3)) == sum(clipped), err[-2000:]
    assert int(told.group(2)) == sum(x != NO_MATE for x in mate) // 2
    changed = 0
    for k in order:
        f, w = a[k], b[k]
        i = slot[k]
        pos, cigar, nm, md, score = _derive(f, *final[i], *scores, affine)
        tags_f = {t[:2]: t for t in f[11:]}
        want = dict(tags_f, NM=f"NM:i:{nm}", MD=f"MD:Z:{md}")
        if "AS" in tags_f and (scores[0] or clipped[i]):
            want["AS"] = f"AS:i:{score}"
        pnext = f[7]
        if mate[i] != NO_MATE:
            other = a[(k[0], not k[1])]
            pnext = str(_derive(other, *final[mate[i]], *scores, affine)[0])
        assert w[:3] == f[:3] and w[4] == f[4] and w[6] == f[6] and w[8:11] == f[8:11], (k, "flag, RNAME, MAPQ, RNEXT, TLEN, SEQ or QUAL changed")
        assert (int(w[3]), w[5], w[7]) == (pos, cigar, pnext), (k, f[3], f[5], role[i], m[i])
        assert {t[:2]: t for t in w[11:]} == want and [t[:2] for t in w[11:]] == [t[:2] for t in f[11:]], (k, w[11:], f[11:])
        changed += w != f
    assert overlapping <= changed <= 2 * overlapping
    # 2. no reference position under both records of a pair
    for k in order:
        if not k[1] and (k[0], True) in b and b[k][2] == b[(k[0], True)][2] and role[slot[k]]:
            (p0, e0), (p1, e1) = sorted([_span(b[k]), _span(b[(k[0], True)])])
            assert e0 <= p1, (k, "a reference position lies under both records")
    return b


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_cli")
    frags, errors = _simulate(d, 97, N_PAIRS, 120, 180, "r.fastq")
    out = {"d": d, "frags": frags, "errors": errors}
    out["plain"] = _tool([*ARGS, "-q", "r.fastq", "-o", "plain.sam", "--paired"], d)
    out["plain_o"] = _tool([*ARGS, "-q", "r.fastq", "-o", "plain_o.sam", "--paired", "--clip-overlap"], d)
    out["plain_o2"] = _tool([*ARGS, "-q", "r.fastq", "-o", "plain_o2.sam", "--paired", "--clip-overlap", "--gpus", "0,0"], d)
    out["full"] = _tool([*ARGS, "-q", "r.fastq", "-o", "full.bam", "--paired", *[x.format(s="full") for x in FULL]], d)
    out["full_o"] = _tool([*ARGS, "-q", "r.fastq", "-o", "full_o.bam", "--paired", "--clip-overlap", *[x.format(s="full_o") for x in FULL]], d)
    return out


@pytest.mark.gpu
def test_plain_records_follow_from_the_run_without_the_option(runs):
    d = runs["d"]
    assert "Overlap:" not in runs["plain"] and "GPU overlap clipping" in runs["plain_o"]
    _check_derivation(_records((d / "plain.sam").read_text()), _records((d / "plain_o.sam").read_text()), runs["plain_o"], N_PAIRS,
                      (0, 0), False)
    # two contexts, the pairs shared out between them: the same bytes; and the oracle-backed tool, which clips on the host
    assert (d / "plain_o2.sam").read_bytes() == (d / "plain_o.sam").read_bytes()
    oracle = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")
    r = subprocess.run([oracle, *ARGS, "-q", "r.fastq", "-o", "plain_oo.sam", "--paired", "--clip-overlap"], cwd=str(d), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (d / "plain_oo.sam").read_bytes() == (d / "plain_o.sam").read_bytes()


@pytest.mark.gpu
def test_full_chain_records_depth_and_duplicates(runs):
    d = runs["d"]
    assert "Overlap:" not in runs["full"]
    without, with_ = _records(bam_to_sam(d / "full.bam")[0]), _records(bam_to_sam(d / "full_o.bam")[0])
    strip = lambda recs: [[x if i != 1 else str(int(x) & ~0x400) for i, x in enumerate(f)] for f in recs]
    b = _check_derivation(strip(without), strip(with_), runs["full_o"], N_PAIRS, (1, 2), True)
    dups = lambda recs: {(f[0], bool(int(f[1]) & 0x80)) for f in recs if int(f[1]) & 0x400}
    assert dups(without) == dups(with_) and len(dups(with_)) >= 20, "--markdup marks other records with the option"
    # the depth of the records never exceeds the simulated fragments over a position
    lens = {"chr0": 50_000, "chr1": 30_000}
    over = {name: np.zeros(n + 1, np.int64) for name, n in lens.items()}
    for c, g0, L in runs["frags"]:
        over[f"chr{c}"][g0] += 1
        over[f"chr{c}"][g0 + L] -= 1
    over = {name: np.cumsum(x)[:-1] for name, x in over.items()}
    worse = 0
    for stem in ("full", "full_o"):
        depth = {name: np.zeros(n, np.int64) for name, n in lens.items()}
        for line in (d / f"{stem}.bedgraph").read_text().split("\n"):
            if line and not line.startswith("#"):
                name, lo, hi, v = line.split("\t")
                depth[name][int(lo): int(hi)] = int(v)
        above = sum(int((depth[name] > over[name]).sum()) for name in lens)
        if stem == "full":
            worse = above
        else:
            assert above == 0, f"{above} positions are deeper than the fragments over them"
    assert worse > 5000, "without the option the overlaps were not counted twice: the comparison shows little"
    assert len(b) > 5000


@pytest.mark.gpu
def test_a_double_counted_error_becomes_a_single_observation(runs):
    d, errors = runs["d"], runs["errors"]
    assert len(errors) >= 20
    sites = lambda stem: {(f[0], int(f[1])): f for f in (l.split("\t") for l in (d / f"{stem}.tsv").read_text().split("\n")
                                                         if l and not l.startswith("#"))}
    without, with_ = sites("full"), sites("full_o")
    for c, p in errors:
        key = (f"chr{c}", p + 1)
        assert key in without, (key, "the planted error is no site without the option")
        counts = [int(x) for x in without[key][3:7]]
        ref_at = "ACGT".index(without[key][2].upper())
        assert sorted(counts[:ref_at] + counts[ref_at + 1:]) == [0, 0, 2], (key, without[key])
        assert key not in with_, (key, with_.get(key))
    assert set(with_) <= set(without)


@pytest.mark.gpu
def test_no_change_where_nothing_overlaps(tmp_path):
    _simulate(tmp_path, 98, 400, 2 * READ + 1, 2 * READ + 200, "far.fastq", planted=False)
    _tool([*ARGS, "-q", "far.fastq", "-o", "far.sam", "--paired"], tmp_path)
    err = _tool([*ARGS, "-q", "far.fastq", "-o", "far_o.sam", "--paired", "--clip-overlap"], tmp_path)
    assert re.search(r"Overlap: 0 of \d+ pairs cut, 0 bases clipped", err)
    assert (tmp_path / "far.sam").read_bytes() == (tmp_path / "far_o.sam").read_bytes()
    full = lambda s: [x.format(s=s) for x in FULL]
    _tool([*ARGS, "-q", "far.fastq", "-o", "far.bam", "--paired", *full("far")], tmp_path)
    _tool([*ARGS, "-q", "far.fastq", "-o", "far_o.bam", "--paired", "--clip-overlap", *full("far_o")], tmp_path)
    for ext in ("bam", "bam.bai", "bedgraph", "tsv", "vcf"):
        assert (tmp_path / f"far.{ext}").read_bytes() == (tmp_path / f"far_o.{ext}").read_bytes(), ext
