"""The pileup rule of include/bmp.h in plain Python and numpy, over a list of BAM record bytes; written from the header's text.

pile(records, ref_len, ref_bases, skip=None, **thresholds) -> Result with .counts (one (ref_len, 8) uint32 array per reference,
columns A C G T N DEL INS LOWQ), .sites ([(r, p, allele, A, C, G, T, N, DEL, INS, LOWQ, kind)]) and .stats ([[n_reads, n_low_mapq,
n_left_out, n_bases, n_lowq, n_sites]] per reference).  refused is depth_rule's (bmp_add checks what bmc_add checks).
pileup_text is the file of --pileup, summary_line the line on stderr."""
import numpy as np

from depth_rule import BLOCK, QUERY, REF, SKIP_FLAGS, fields, refused  # noqa: F401  (the record layout and the walk are bmc.h's)

A, C, G, T, N, DEL, INS, LOWQ = range(8)
SNV_BIT, DEL_BIT, INS_BIT = 1, 2, 4
DEFAULTS = dict(min_mapq=0, min_bq=13, min_alt=2, min_frac_ppm=200000)
COUNTER_OF_CODE = np.full(16, N)
COUNTER_OF_CODE[[1, 2, 4, 8]] = [A, C, G, T]
PPM = 1000000


def sequence_of(rec):
    """The packed sequence bytes of a record."""
    l_name, n_cigar, l_seq = rec[12], int.from_bytes(rec[16:18], "little"), int.from_bytes(rec[20:24], "little")
    at = 36 + l_name + 4 * n_cigar
    return rec[at: at + (l_seq + 1) // 2]


ALLELE_OF_BYTE = np.full(256, 4, np.int64)            # A C G T in either case give the allele 0 .. 3, every other byte none (4)
for _k, _letter in enumerate("ACGT"):
    ALLELE_OF_BYTE[[ord(_letter), ord(_letter.lower())]] = _k


class Result:
    def __init__(self, counts, sites, stats):
        self.counts, self.sites, self.stats = counts, sites, stats


def pile(records, ref_len, ref_bases, skip=None, **thresholds):
    th = {**DEFAULTS, **thresholds}
    n_ref = len(ref_len)
    assert n_ref > 0 and all(l > 0 for l in ref_len) and refused(records, n_ref) is None
    assert th["min_alt"] >= 1 and 0 <= th["min_frac_ppm"] <= PPM and [len(b) for b in ref_bases] == list(ref_len)
    counts = [np.zeros((l, 8), np.int64) for l in ref_len]
    stats = [[0] * 6 for _ in range(n_ref)]
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
        if mapq < th["min_mapq"]:
            st[1] += 1
            continue
        st[0] += 1
        # per query base the counter it selects: LOWQ by its quality, else the one of its 4-bit code (high nibble for even j)
        packed = np.frombuffer(sequence_of(rec), np.uint8)
        code = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq]
        q = np.frombuffer(qual, np.uint8)
        which = np.where((q != 0xFF) & (q < th["min_bq"]), LOWQ, COUNTER_OF_CODE[code])
        c = counts[ref]
        rc, qc, anchored = pos, 0, False
        for word in cigar:
            op, n = word & 15, word >> 4
            if op in BLOCK:
                m = max(0, min(rc + n, ref_len[ref]) - rc)      # what lies beyond the reference does not count
                if m:
                    c[np.arange(rc, rc + m), which[qc: qc + m]] += 1
            elif op == 2:
                c[min(rc, ref_len[ref]): min(rc + n, ref_len[ref]), DEL] += 1
            elif op == 1 and n > 0 and anchored and rc - 1 < ref_len[ref]:
                c[rc - 1, INS] += 1
            if (op in BLOCK or op == 2) and n > 0:
                anchored = True
            if op in REF:
                rc += n
            if op in QUERY:
                qc += n
    sites = []
    for r in range(n_ref):
        c = counts[r]
        span = c[:, [A, C, G, T, N, DEL]].sum(axis=1)
        allele = ALLELE_OF_BYTE[np.frombuffer(bytes(ref_bases[r]), np.uint8)]
        letters = c[:, :4].copy()
        has = allele < 4
        letters[np.flatnonzero(has), allele[has]] = -1      # the reference allele itself is no alternative
        alt = letters.max(axis=1)
        passes = lambda x: (x >= th["min_alt"]) & (x * PPM >= th["min_frac_ppm"] * span)
        kind = (has & passes(alt)) * SNV_BIT + passes(c[:, DEL]) * DEL_BIT + passes(c[:, INS]) * INS_BIT
        for p in np.flatnonzero(kind).tolist():
            sites.append((r, p, int(allele[p]), *[int(x) for x in c[p]], int(kind[p])))
        stats[r][3] = int(c[:, :5].sum())
        stats[r][4] = int(c[:, LOWQ].sum())
        stats[r][5] = int(np.count_nonzero(kind))
        assert c.max(initial=0) < 2 ** 32
    return Result([c.astype(np.uint32) for c in counts], sites, stats)


def pileup_text(res, names):
    out = "#rname\tpos\tref\tA\tC\tG\tT\tN\tdel\tins\tlowq\tkind\n"
    for s in res.sites:
        kind = "".join(ch for bit, ch in ((SNV_BIT, "S"), (DEL_BIT, "D"), (INS_BIT, "I")) if s[11] & bit)
        out += "\t".join([names[s[0]], str(s[1] + 1), "ACGT."[s[2]], *[str(x) for x in s[3:11]], kind]) + "\n"
    return out


def summary_line(res):
    total = [sum(s[j] for s in res.stats) for j in range(6)]
    return f"Pileup: {total[5]} sites on {total[3]} bases from {total[0]} records ({total[2]} left out, {total[1]} below MAPQ)"
