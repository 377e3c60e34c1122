"""The bias rule of include/bmb.h in plain Python, big integers, no wrap; written from the header's text.  The counted records
and the walk are bmp.h's (tests/pileup_rule.py, tests/depth_rule.py), which bases count is bmg.h's.

cells(records, ref_len, skip=None, **params) -> (fwd, rev, n, S): per reference (ref_len, 4) int64 arrays fwd and rev, columns
A C G T, and (ref_len,) int64 arrays n and S.  packed_strand / packed_mapq -> the uint64 cells of bmb_cells_at.
annotate_one(call, fwd4, rev4, n, S, LF, E) -> the 16 words of one call; annotate(...) for a list of calls.
fs(a, b, c, d, LF, E) -> FS in centi-phred or None.  The two tables LF and E are INPUTS: the rule never computes them
(bmb_tables of the library makes them); make_tables() here is what the tests compare that function with, within +-1.
vcf_lines is the file of --vcf --vcf-bias below the header, summary_line the line on stderr."""
import math
from decimal import Decimal, getcontext

import numpy as np

from depth_rule import BLOCK, QUERY, REF, SKIP_FLAGS, fields, refused  # noqa: F401
from genotype_rule import LETTER_OF_CODE, VARIANT
from pileup_rule import sequence_of

DEFAULTS = dict(min_mapq=0, min_bq=13)
N_LF, N_E, FS_CAP, FS_MAX_N, MAX_BASES = 65536, 12001, 6000, 65535, 2 ** 24 - 1
OUT_WORDS = 16
ANNOTATED, NO_FS = 1, 2
W_FWD, W_REV, W_MQ, W_FS, W_FLAGS, W_N, W_TABLE = 0, 4, 8, 9, 10, 11, 12


def cells(records, ref_len, skip=None, **params):
    pr = {**DEFAULTS, **params}
    n_ref = len(ref_len)
    assert n_ref > 0 and all(l > 0 for l in ref_len) and refused(records, n_ref) is None
    fwd = [np.zeros((l, 4), np.int64) for l in ref_len]
    rev = [np.zeros((l, 4), np.int64) for l in ref_len]
    n = [np.zeros(l, np.int64) for l in ref_len]
    S = [np.zeros(l, np.int64) for l in ref_len]
    for i, rec in enumerate(records):
        ref, pos, mapq, flag, l_seq, cigar, qual = fields(rec)
        if flag & SKIP_FLAGS or (skip is not None and skip[i]):
            continue
        if not (0 <= ref < n_ref and 0 <= pos < ref_len[ref]) or not cigar:
            continue
        if l_seq == 0 or (len(cigar) == 2 and cigar[0] == (l_seq << 4 | 4) and cigar[1] & 15 == 3):
            continue
        if mapq < pr["min_mapq"]:
            continue
        packed_seq = np.frombuffer(sequence_of(rec), np.uint8)
        letter = LETTER_OF_CODE[np.stack([packed_seq >> 4, packed_seq & 15], axis=1).reshape(-1)[:l_seq]]
        q = np.frombuffer(qual, np.uint8).astype(np.int64)
        counts = ((q == 0xFF) | (q >= pr["min_bq"])) & (letter < 4)
        strand = rev if flag & 0x10 else fwd
        rc, qc = pos, 0
        for word in cigar:
            op, length = word & 15, word >> 4
            if op in BLOCK:
                m = max(0, min(rc + length, ref_len[ref]) - rc)     # what lies beyond the reference does not count
                if m:
                    keep = np.flatnonzero(counts[qc: qc + m])
                    strand[ref][rc + keep, letter[qc + keep]] += 1   # a block visits a position once: no repeated index
                    n[ref][rc + keep] += 1
                    S[ref][rc + keep] += mapq * mapq
            if op in REF:
                rc += length
            if op in QUERY:
                qc += length
    return fwd, rev, n, S


def packed_strand(fwd, rev):
    assert int(fwd.max(initial=0)) <= MAX_BASES and int(rev.max(initial=0)) <= MAX_BASES
    return (fwd.astype(np.uint64) << np.uint64(32)) | rev.astype(np.uint64)


def packed_mapq(n, S):
    assert int(n.max(initial=0)) <= MAX_BASES and int(S.max(initial=0)) < 2 ** 40
    return (n.astype(np.uint64) << np.uint64(40)) | S.astype(np.uint64)


def mq(n, S):
    """The floor of the root mean square of the MAPQs to two decimals, in centi-units."""
    return math.isqrt(10000 * S // n) if n else 0


def make_tables():
    """LF and E from exact arithmetic (decimal, 60 digits), as Python lists."""
    getcontext().prec = 60
    lf, acc = [0], Decimal(0)
    for k in range(1, N_LF):
        acc += Decimal(k).log10()
        lf.append(int((1000 * acc).to_integral_value(rounding="ROUND_HALF_EVEN")))
    e = [int((Decimal(2 ** 40) * Decimal(10) ** (Decimal(-d) / 1000)).to_integral_value(rounding="ROUND_HALF_EVEN")) for d in range(N_E)]
    return lf, e


def fs(a, b, c, d, LF, E):
    """FS of the table ((a, b), (c, d)) in centi-phred, or None where the rule gives none."""
    r1, r2, c1, c2 = a + b, c + d, a + c, b + d
    if r1 + r2 > FS_MAX_N or 0 in (r1, r2, c1, c2):
        return None
    xs = range(max(0, c1 - r2), min(r1, c1) + 1)
    w = {x: -(int(LF[x]) + int(LF[r1 - x]) + int(LF[c1 - x]) + int(LF[r2 - c1 + x])) for x in xs}
    m = max(w.values())
    e_of = lambda k: int(E[k]) if k < N_E else 0
    s_all = sum(e_of(m - w[x]) for x in xs)
    s_ext = sum(e_of(m - w[x]) for x in xs if w[x] <= w[a] + 4)
    for k in range(FS_CAP):
        if s_all * int(E[k]) <= s_ext << 40:
            return k
    return FS_CAP


def table_of(call, fwd4, rev4):
    R = call[2]
    others = sorted({call[4], call[5]} - {R})
    return fwd4[R], rev4[R], sum(fwd4[x] for x in others), sum(rev4[x] for x in others)


def annotate_one(call, fwd4, rev4, n, S, LF, E):
    """The 16 words of the annotation of one call (24 words as bmg_call returns them)."""
    if not call[3] & VARIANT:
        return (0,) * OUT_WORDS
    t = table_of(call, fwd4, rev4)
    f = fs(*t, LF, E)
    return (*fwd4, *rev4, mq(n, S), 0 if f is None else f, ANNOTATED | (NO_FS if f is None else 0), n, *t)


def annotate(called, fwd, rev, n, S, LF, E):
    out = []
    for c in called:
        r, p = c[0], c[1]
        out.append(annotate_one(c, [int(x) for x in fwd[r][p]], [int(x) for x in rev[r][p]], int(n[r][p]), int(S[r][p]), LF, E))
    return out


BIAS_HEAD = ("##INFO=<ID=FS,", "##INFO=<ID=MQ,", "##FILTER=<ID=StrandBias,", "##FILTER=<ID=LowMQ,", "##FORMAT=<ID=ADF,", "##FORMAT=<ID=ADR,")


def vcf_lines(called, notes, names, min_qual=20, max_fs=60, min_mq=0):
    """The lines of --vcf --vcf-bias below the header: one per VARIANT call, in order."""
    out = []
    for c, b in zip(called, notes):
        if not c[3] & VARIANT:
            continue
        assert b[W_FLAGS] & ANNOTATED
        R, g = c[2], (c[4], c[5])
        alleles = [R] + [x for x in sorted(set(g)) if x != R]
        gt = sorted(alleles.index(x) for x in g)
        pl = []
        for hi in range(len(alleles)):
            for lo in range(hi + 1):
                x, y = sorted((alleles[lo], alleles[hi]))
                pl.append(c[12 + y * (y + 1) // 2 + x] // 100)
        has_fs = not b[W_FLAGS] & NO_FS
        filters = (["LowQual"] if c[7] < 100 * min_qual else []) + (["StrandBias"] if has_fs and b[W_FS] >= 100 * max_fs else []) + \
                  (["LowMQ"] if b[W_MQ] < 100 * min_mq else [])
        info = f"DP={c[22]}" + (";FS=%d.%02d" % (b[W_FS] // 100, b[W_FS] % 100) if has_fs else "") + ";MQ=%d.%02d" % (b[W_MQ] // 100, b[W_MQ] % 100)
        sample = ":".join([f"{gt[0]}/{gt[1]}", str(c[22]), ",".join(str(c[8 + x]) for x in alleles), ",".join(str(b[W_FWD + x]) for x in alleles),
                           ",".join(str(b[W_REV + x]) for x in alleles), str(c[6]), ",".join(str(x) for x in pl)])
        out.append("\t".join([names[c[0]], str(c[1] + 1), ".", "ACGT"[R], ",".join("ACGT"[x] for x in alleles[1:]), "%d.%02d" % (c[7] // 100, c[7] % 100),
                              ";".join(filters) or "PASS", info, "GT:DP:AD:ADF:ADR:GQ:PL", sample]))
    return out


def summary_line(notes, max_fs=60, min_mq=0):
    done = [b for b in notes if b[W_FLAGS] & ANNOTATED]
    biased = sum(1 for b in done if not b[W_FLAGS] & NO_FS and b[W_FS] >= 100 * max_fs)
    low = sum(1 for b in done if b[W_MQ] < 100 * min_mq)
    none = sum(1 for b in done if b[W_FLAGS] & NO_FS)
    return f"Bias: {len(done)} variants annotated ({biased} StrandBias, {low} LowMQ, {none} without FS)"
