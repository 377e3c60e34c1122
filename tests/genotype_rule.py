"""The genotype rule of include/bmg.h in plain Python, big integers, no wrap; written from the header's text.  The counted
records and the walk are bmp.h's (tests/pileup_rule.py, tests/depth_rule.py).

cells(records, ref_len, skip=None, **params) -> (n, Q): per reference an (ref_len, 4) int64 array each, columns A C G T.
packed(n, Q) -> the (ref_len, 4) uint64 cells n << 32 | Q of bmg_cells_at.
calls(n, Q, sites, **params) -> one 24-tuple per site (twelve numbers as bmp_sites returns them).
genotype(records, ref_len, sites, skip=None, **params) is both in one.  vcf_text is the file of --vcf, summary_line the line
on stderr."""
import numpy as np

from depth_rule import BLOCK, QUERY, REF, SKIP_FLAGS, fields, refused  # noqa: F401
from pileup_rule import sequence_of

DEFAULTS = dict(min_mapq=0, min_bq=13, q_absent=30, q_cap=60, prior=3000)
GENOTYPED, VARIANT = 1, 2
U32 = 2 ** 32 - 1
LETTER_OF_CODE = np.full(16, 4)
LETTER_OF_CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]
GENOTYPES = [(a, b) for b in range(4) for a in range(b + 1)]      # k = b (b + 1) / 2 + a: AA AC CC AG CG GG AT CT GT TT


def cells(records, ref_len, skip=None, **params):
    pr = {**DEFAULTS, **params}
    n_ref = len(ref_len)
    assert n_ref > 0 and all(l > 0 for l in ref_len) and refused(records, n_ref) is None
    assert 1 <= pr["q_cap"] <= 93 and pr["q_absent"] <= pr["q_cap"]
    n = [np.zeros((l, 4), np.int64) for l in ref_len]
    Q = [np.zeros((l, 4), np.int64) for l in ref_len]
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
        q_eff = np.where(q == 0xFF, pr["q_absent"], np.minimum(q, pr["q_cap"]))
        rc, qc = pos, 0
        for word in cigar:
            op, length = word & 15, word >> 4
            if op in BLOCK:
                m = max(0, min(rc + length, ref_len[ref]) - rc)     # what lies beyond the reference does not count
                if m:
                    keep = np.flatnonzero(counts[qc: qc + m])
                    n[ref][rc + keep, letter[qc + keep]] += 1        # a block visits a position once: no repeated index
                    Q[ref][rc + keep, letter[qc + keep]] += q_eff[qc + keep]
            if op in REF:
                rc += length
            if op in QUERY:
                qc += length
    return n, Q


def packed(n, Q):
    assert int(Q.max(initial=0)) <= U32 and int(n.max(initial=0)) <= U32
    return (n.astype(np.uint64) << np.uint64(32)) | Q.astype(np.uint64)


def call_one(n4, Q4, site, prior):
    """The 24 words of the call of one site from its position's n[A..T] and Q[A..T] (Python ints)."""
    ref, pos, R, kind = site[0], site[1], site[2], site[11]
    out = [ref, pos, R] + [0] * 5 + [min(x, U32) for x in n4] + [0] * 12
    depth = sum(n4)
    if not kind & 1 or R > 3 or depth == 0:
        return tuple(out)
    M = [100 * Q4[a] + 477 * n4[a] for a in range(4)]
    T = [301 * n4[a] for a in range(4)]
    cost = []
    for a, b in GENOTYPES:
        like = sum(M[c] for c in range(4) if c != a) if a == b else T[a] + T[b] + sum(M[c] for c in range(4) if c not in (a, b))
        cost.append(like + prior * len({a, b} - {R}))
    least = min(cost)
    k_rr = GENOTYPES.index((R, R))
    best = k_rr if cost[k_rr] == least else cost.index(least)
    second = sorted(cost)[1]                              # as a multiset: the smallest again on a tie
    out[3] = GENOTYPED | (VARIANT if best != k_rr else 0)
    out[4], out[5] = GENOTYPES[best]
    out[6] = min(99, (second - least) // 100)
    out[7] = min(cost[k_rr] - least, U32)
    out[12:22] = [min(c - least, U32) for c in cost]
    out[22] = min(depth, U32)
    return tuple(out)


def calls(n, Q, sites, **params):
    prior = {**DEFAULTS, **params}["prior"]
    return [call_one([int(x) for x in n[s[0]][s[1]]], [int(x) for x in Q[s[0]][s[1]]], s, prior) for s in sites]


def genotype(records, ref_len, sites, skip=None, **params):
    n, Q = cells(records, ref_len, skip, **params)
    return n, Q, calls(n, Q, sites, **params)


VCF_HEAD = ("##fileformat=VCFv4.2", "##source=", "##contig=", "##INFO=<ID=DP,", "##FILTER=<ID=LowQual,", "##FORMAT=<ID=GT,", "##FORMAT=<ID=DP,",
            "##FORMAT=<ID=AD,", "##FORMAT=<ID=GQ,", "##FORMAT=<ID=PL,", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t")


def vcf_lines(called, names, min_qual=20):
    """The lines of --vcf below the header: one per VARIANT call, in order."""
    out = []
    for c in called:
        if not c[3] & VARIANT:
            continue
        R, g = c[2], (c[4], c[5])
        alleles = [R] + [x for x in sorted(set(g)) if x != R]
        gt = sorted(alleles.index(x) for x in g)
        pl = []
        for hi in range(len(alleles)):                   # VCF order: j <= k at k (k + 1) / 2 + j
            for lo in range(hi + 1):
                a, b = sorted((alleles[lo], alleles[hi]))
                pl.append(c[12 + b * (b + 1) // 2 + a] // 100)
        sample = ":".join([f"{gt[0]}/{gt[1]}", str(c[22]), ",".join(str(c[8 + x]) for x in alleles), str(c[6]), ",".join(str(x) for x in pl)])
        out.append("\t".join([names[c[0]], str(c[1] + 1), ".", "ACGT"[R], ",".join("ACGT"[x] for x in alleles[1:]), "%d.%02d" % (c[7] // 100, c[7] % 100),
                              "PASS" if c[7] >= 100 * min_qual else "LowQual", f"DP={c[22]}", "GT:DP:AD:GQ:PL", sample]))
    return out


def check_vcf_header(text, refs, sample="sample"):
    """The header of a --vcf file names what it must, in order, with one contig line per reference; returns the lines below it."""
    lines = text.split("\n")
    assert lines[-1] == ""
    head = [l for l in lines[:-1] if l.startswith("#")]
    assert lines[: len(head)] == head and head[0] == "##fileformat=VCFv4.2" and head[1].startswith("##source=")
    assert head[2: 2 + len(refs)] == [f"##contig=<ID={name},length={length}>" for name, length in refs]
    rest = head[2 + len(refs):]
    assert len(rest) == 8 and all(l.startswith(p) for l, p in zip(rest, VCF_HEAD[3:])), rest
    assert rest[-1] == VCF_HEAD[-1] + sample
    return lines[len(head): -1]


def summary_line(called, sites, min_qual=20):
    variants = [c for c in called if c[3] & VARIANT]
    het = sum(1 for c in variants if c[4] != c[5])
    low = sum(1 for c in variants if c[7] < 100 * min_qual)
    snv = sum(1 for s in sites if s[11] & 1)
    return f"Genotypes: {len(variants)} variants ({het} het, {len(variants) - het} hom, {low} below QUAL) at {snv} SNV sites"
