"""The indel rule of include/bmn.h in plain Python with big integers, over a list of BAM record bytes; written from the header's
text.

indels(records, ref_len, skip=None, **params) -> Result with .events (one tuple (slot, w1, seq_lo, seq_hi) per event, in the
order of the records and of the ops inside a record), .alleles ([(ref, anchor, w1, seq_lo, seq_hi, n, 0, 0)]), .calls (16-tuples),
.cover (one uint32 array per reference) and .stats ([[n_reads, n_low_mapq, n_left_out]] per reference).  vcf_fields gives REF
and ALT of a call, indel_line the line on stderr."""
import numpy as np

from depth_rule import BLOCK, QUERY, REF, SKIP_FLAGS, fields, refused  # noqa: F401  (the record layout and the walk are bmc.h's)
from pileup_rule import sequence_of

DEFAULTS = dict(min_mapq=0, min_alt=2, min_frac_ppm=200000, q_indel=30, prior=4000)
INS, OTHER, MAX_INS, PPM, U32 = 1 << 31, 1 << 30, 32, 1000000, 2 ** 32 - 1
GENOTYPED, VARIANT = 1, 2
TWO_BITS = {1: 0, 2: 1, 4: 2, 8: 3}


class Result:
    def __init__(self, events, alleles, calls, cover, stats):
        self.events, self.alleles, self.calls, self.cover, self.stats = events, alleles, calls, cover, stats


def events_of(rec, ref_len, first):
    """(pos, end', events) of a counted record on a reference of ref_len bases whose first slot is `first`."""
    ref, pos, mapq, flag, l_seq, cigar, qual = fields(rec)
    end = pos + sum(w >> 4 for w in cigar if w & 15 in REF)
    endc = min(end, ref_len)
    packed = sequence_of(rec)
    code = lambda j: (packed[j >> 1] >> (0 if j & 1 else 4)) & 15
    out, rc, qc, anchored = [], pos, 0, False
    for word in cigar:
        op, n = word & 15, word >> 4
        if op in (1, 2) and n > 0 and anchored and rc >= 1:
            if op == 2 and rc + n <= ref_len:
                out.append((first + rc - 1, n, 0, 0))
            if op == 1 and rc < endc:
                codes = [code(qc + j) for j in range(n)] if n <= MAX_INS else [0]
                if all(c in TWO_BITS for c in codes):
                    seq = sum(TWO_BITS[c] << (2 * j) for j, c in enumerate(codes))
                    out.append((first + rc - 1, n | INS, seq & U32, seq >> 32))
                else:
                    out.append((first + rc - 1, n | INS | OTHER, 0, 0))
        if (op in BLOCK or op == 2) and n > 0:
            anchored = True
        if op in REF:
            rc += n
        if op in QUERY:
            qc += n
    return pos, endc, out


def call_of(anchor_alleles, D, pr):
    """The 16 words of the call of an anchor from its alleles (in allele order) and cover, or None if it is no site."""
    E = sum(a[5] for a in anchor_alleles)
    alt = None
    for a in anchor_alleles:
        if not a[2] & OTHER and (alt is None or a[5] > alt[5]):
            alt = a
    if alt is None:
        return None
    n_alt = alt[5]
    if not (D > 0 and n_alt >= pr["min_alt"] and n_alt * PPM >= pr["min_frac_ppm"] * D):
        return None
    n_ref, n_oth = max(D - E, 0), E - n_alt
    L = [100 * pr["q_indel"] * n_alt, 301 * (n_ref + n_alt) + pr["prior"], 100 * pr["q_indel"] * n_ref + pr["prior"]]
    g = 0
    if L[1] < L[g]:
        g = 1
    if L[2] < L[g]:
        g = 2
    ordered = sorted(L)
    gq = min(99, (ordered[1] - ordered[0]) // 100)
    sat = lambda v: min(v, U32)
    return (alt[0], alt[1], alt[2], alt[3], alt[4], GENOTYPED | (VARIANT if g else 0), g, gq, sat(L[0] - L[g]), n_ref, n_alt, sat(n_oth), D,
            sat(L[0] - L[g]), sat(L[1] - L[g]), sat(L[2] - L[g]))


def indels(records, ref_len, skip=None, **params):
    pr = {**DEFAULTS, **params}
    n_ref = len(ref_len)
    assert n_ref > 0 and all(l > 0 for l in ref_len) and refused(records, n_ref) is None
    assert pr["min_alt"] >= 1 and 0 <= pr["min_frac_ppm"] <= PPM and 1 <= pr["q_indel"] <= 93
    base = [0]
    for l in ref_len:
        base.append(base[-1] + l)
    diff = [np.zeros(l + 1, np.int64) for l in ref_len]
    stats = [[0] * 3 for _ in range(n_ref)]
    events = []
    for i, rec in enumerate(records):
        ref, pos, mapq, flag, l_seq, cigar, qual = fields(rec)
        if flag & SKIP_FLAGS or (skip is not None and skip[i]):
            continue
        if not (0 <= ref < n_ref and 0 <= pos < ref_len[ref]) or not cigar:
            continue
        st = stats[ref]
        if l_seq == 0 or (len(cigar) == 2 and cigar[0] == (l_seq << 4 | 4) and cigar[1] & 15 == 3):
            st[2] += 1
            continue
        if mapq < pr["min_mapq"]:
            st[1] += 1
            continue
        st[0] += 1
        pos, endc, found = events_of(rec, ref_len[ref], base[ref])
        if endc - pos >= 2:                              # spans the steps pos .. end' - 2
            diff[ref][pos] += 1
            diff[ref][endc - 1] -= 1
        events += found
    cover = [np.cumsum(d[:-1]) for d in diff]
    assert all(c.min(initial=0) >= 0 and c.max(initial=0) <= U32 for c in cover)
    counts = {}
    for e in events:
        counts[e] = counts.get(e, 0) + 1
    ref_of = lambda slot: max(r for r in range(n_ref) if base[r] <= slot)
    alleles = []
    for slot, w1, lo, hi in sorted(counts, key=lambda e: (e[0], e[1], e[3] << 32 | e[2])):
        r = ref_of(slot)
        alleles.append((r, slot - base[r], w1, lo, hi, counts[(slot, w1, lo, hi)], 0, 0))
    calls, at = [], 0
    while at < len(alleles):
        to = at
        while to < len(alleles) and alleles[to][:2] == alleles[at][:2]:
            to += 1
        r, a = alleles[at][:2]
        c = call_of(alleles[at:to], int(cover[r][a]), pr)
        if c is not None:
            calls.append(c)
        at = to
    return Result(events, alleles, calls, [c.astype(np.uint32) for c in cover], stats)


# ---- the VCF ----
def letter_of(byte):
    """The tools' convention for a reference letter: upper case, and what is not A C G T reads as A."""
    ch = chr(byte).upper()
    return ch if ch in "ACGT" else "A"


def vcf_fields(call, ref_bases):
    """(POS, REF, ALT) of a call; ref_bases is the reference's bytes."""
    anchor, w1 = call[1], call[2]
    n = w1 & ((1 << 28) - 1)
    first = letter_of(ref_bases[anchor])
    if w1 & INS:
        seq = call[3] | call[4] << 32
        return anchor + 1, first, first + "".join("ACGT"[(seq >> (2 * j)) & 3] for j in range(n))
    return anchor + 1, first + "".join(letter_of(b) for b in ref_bases[anchor + 1: anchor + 1 + n]), first


def vcf_line(call, name, ref_bases, min_qual):
    """The line of a variant call, as host/indel.h writes it; None for a call that is not a variant."""
    if not call[5] & VARIANT:
        return None
    pos, ref, alt = vcf_fields(call, ref_bases)
    gt = "0/1" if call[6] == 1 else "1/1"
    return (f"{name}\t{pos}\t.\t{ref}\t{alt}\t{call[8] // 100}.{call[8] % 100:02d}\t{'PASS' if call[8] >= 100 * min_qual else 'LowQual'}"
            f"\tINDEL;DP={call[12]}\tGT:DP:AD:GQ:PL\t{gt}:{call[12]}:{call[9]},{call[10]}:{call[7]}:{','.join(str(x // 100) for x in call[13:16])}")


def indel_line(res, min_qual):
    v = [c for c in res.calls if c[5] & VARIANT]
    het, hom = sum(1 for c in v if c[6] == 1), sum(1 for c in v if c[6] == 2)
    low = sum(1 for c in v if c[8] < 100 * min_qual)
    other = sum(a[5] for a in res.alleles if a[2] & OTHER)
    return f"Indels: {len(v)} variants ({het} het, {hom} hom, {low} below QUAL) at {len(res.calls)} sites from {len(res.events)} events ({other} other)"
