"""The reference-block rule of include/bmr.h in plain Python, written from the header's text: the costs of one position in big
integers (gq_one), the same over whole references in int64 with its bounds asserted (no wrap), the blocks, the gVCF text and
the line on stderr.  The cells are those of tests/genotype_rule.py.

positions(n, Q, bases, bands, exclude) -> (word0, dp): per reference two uint32 arrays, the per-position view of bmr_conf_at.
blocks(word0, dp) -> the list of 8-tuples of bmr_blocks.  run(...) is both in one."""
import numpy as np

from genotype_rule import GENOTYPES

DEFAULT_BANDS = (1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99)
IN, EXCLUDED, NO_ALLELE = 1 << 16, 1 << 17, 1 << 18
U32 = 2 ** 32 - 1
LETTER = np.full(256, 4)
for _k, _c in enumerate("ACGT"):
    LETTER[ord(_c)] = LETTER[ord(_c.lower())] = _k


def check_bands(bands):
    assert len(bands) <= 16 and all(1 <= b <= 99 for b in bands) and all(a < b for a, b in zip(bands, bands[1:])), bands


def costs(n4, Q4):
    """L(g) of the ten genotypes, without a prior (Python ints)."""
    M = [100 * Q4[a] + 477 * n4[a] for a in range(4)]
    T = [301 * n4[a] for a in range(4)]
    return [sum(M[c] for c in range(4) if c != a) if a == b else T[a] + T[b] + sum(M[c] for c in range(4) if c not in (a, b)) for a, b in GENOTYPES]


def gq_one(n4, Q4, R):
    """gq of one position with the reference allele R <= 3."""
    L = costs([int(x) for x in n4], [int(x) for x in Q4])
    k_rr = GENOTYPES.index((R, R))
    h = min(l for k, l in enumerate(L) if k != k_rr)
    return min(99, (h - L[k_rr]) // 100) if L[k_rr] <= h else 0


def gq_all(n, Q, R):
    """gq at every position of one reference (zero where R is 4), in int64: every cost stays below 2^45."""
    assert int(n.max(initial=0)) <= U32 and int(Q.max(initial=0)) <= U32
    M, T = 100 * Q + 477 * n, 301 * n
    total = M.sum(axis=1)
    L = np.stack([total - M[:, a] if a == b else T[:, a] + T[:, b] + total - M[:, a] - M[:, b] for a, b in GENOTYPES], axis=1)
    gq = np.zeros(len(n), np.int64)
    for r in range(4):
        k_rr = GENOTYPES.index((r, r))
        h = np.delete(L, k_rr, axis=1).min(axis=1)
        g = np.where(L[:, k_rr] <= h, np.minimum(99, (h - L[:, k_rr]) // 100), 0)
        gq = np.where(R == r, g, gq)
    return gq


def positions(n, Q, bases, bands=DEFAULT_BANDS, exclude=()):
    check_bands(bands)
    word0, dp = [], []
    for r, b in enumerate(bases):
        R = LETTER[np.frombuffer(bytes(b), np.uint8)]
        assert len(R) == len(n[r])
        gq = gq_all(n[r], Q[r], R)
        band = np.zeros(len(R), np.int64)
        for bound in bands:
            band += gq >= bound
        state = np.where(R <= 3, IN, NO_ALLELE)
        for ref, start, end in exclude:
            assert 0 <= ref < len(bases) and 0 <= start < end <= len(bases[ref])
            if ref == r:
                state[start:end] = EXCLUDED
        word0.append(np.where(state == IN, gq | band << 8 | IN, state).astype(np.uint32))
        dp.append(np.minimum(n[r].sum(axis=1), U32).astype(np.uint32))
    return word0, dp


def blocks(word0, dp):
    out = []
    for r, (w, d) in enumerate(zip(word0, dp)):
        w = w.astype(np.int64)
        key = np.where(w & IN, w >> 8, -1)                   # the band with the IN bit, -1 outside
        cut = np.flatnonzero(np.diff(key)) + 1
        for start, end in zip(np.concatenate([[0], cut]), np.concatenate([cut, [len(w)]])):
            if key[start] < 0:
                continue
            out.append((r, int(start), int(end), int(key[start]) & 0xFF, int((w[start:end] & 0xFF).min()), int(d[start:end].min()),
                        sum(int(x) for x in d[start:end].astype(np.uint64)) & U32, sum(int(x) for x in d[start:end].astype(np.uint64)) >> 32))
    return out


def run(n, Q, bases, bands=DEFAULT_BANDS, exclude=()):
    word0, dp = positions(n, Q, bases, bands, exclude)
    return word0, dp, blocks(word0, dp)


def conf_words(word0, dp):
    """One reference's view as bmr_conf_at returns it: (length, 2) uint32."""
    return np.stack([word0, dp], axis=1).astype(np.uint32)


def check_tiling(blks, word0):
    """Per reference the blocks, the excluded and the R = 4 positions partition [0, length): no overlap, no gap."""
    for r, w in enumerate(word0):
        covered = np.zeros(len(w), np.int64)
        for b in blks:
            if b[0] == r:
                assert 0 <= b[1] < b[2] <= len(w)
                covered[b[1]: b[2]] += 1
        covered += ((w & (EXCLUDED | NO_ALLELE)) != 0)
        assert (covered == 1).all(), (r, np.flatnonzero(covered != 1)[:10])
    assert blks == sorted(blks, key=lambda b: (b[0], b[1]))


# ---- the file of --gvcf ----
def ref_letter(byte):
    c = chr(byte & 0xDF)
    return c if c in "ACGT" else "A"


def block_lines(blks, names, bases):
    """(reference, POS, line) of every block."""
    out = []
    for b in blks:
        total, length = b[6] | b[7] << 32, b[2] - b[1]
        out.append((b[0], b[1] + 1, "\t".join([names[b[0]], str(b[1] + 1), ".", ref_letter(bases[b[0]][b[1]]), "<NON_REF>", ".", ".", f"END={b[2]}",
                                               "GT:DP:GQ:MIN_DP", f"0/0:{total // length}:{b[4]}:{b[5]}"])))
    return out


def excluded_by(variant_lines, names, ref_len):
    """The intervals the tools exclude, from the variant lines of the file: POS of every line, and the deleted bases of a
    deletion clipped to the reference."""
    out = []
    for line in variant_lines:
        f = line.split("\t")
        ref, pos0 = names.index(f[0]), int(f[1]) - 1
        out.append((ref, pos0, pos0 + 1))
        if len(f[3]) > 1 and pos0 + 1 < ref_len[ref]:
            out.append((ref, pos0 + 1, min(pos0 + len(f[3]), ref_len[ref])))
    return out


def merged(variant_lines, blks, names, bases):
    """The body of the --gvcf file: the variant lines in their order with the block lines between them by (reference, POS)."""
    keyed = [(names.index(l.split("\t")[0]), int(l.split("\t")[1]), 0, k, l) for k, l in enumerate(variant_lines)]
    keyed += [(r, pos, 1, k, l) for k, (r, pos, l) in enumerate(block_lines(blks, names, bases))]
    return [x[4] for x in sorted(keyed, key=lambda x: x[:4])]


GVCF_HEAD = ("##ALT=<ID=NON_REF,", "##INFO=<ID=END,", "##FORMAT=<ID=MIN_DP,")


def split_gvcf(text, refs, sample="sample"):
    """Checks the header of a --gvcf file; returns (the variant lines, the block lines) below it, each in file order."""
    lines = text.split("\n")
    assert lines[-1] == ""
    head = [l for l in lines[:-1] if l.startswith("#")]
    assert lines[: len(head)] == head and head[0] == "##fileformat=VCFv4.2" and head[1] == "##source=bucketmap --gvcf"
    assert head[2: 2 + len(refs)] == [f"##contig=<ID={name},length={length}>" for name, length in refs]
    for prefix in GVCF_HEAD:
        assert sum(l.startswith(prefix) for l in head) == 1, prefix
    assert head[-1] == "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + sample
    body = lines[len(head): -1]
    is_block = [l.split("\t")[4] == "<NON_REF>" for l in body]
    return [l for l, b in zip(body, is_block) if not b], [l for l, b in zip(body, is_block) if b], body


def vcf_header_of(gvcf_text):
    """The header a --vcf file of the same run has: the gVCF's without its three lines and with --vcf's source."""
    head = [l for l in gvcf_text.split("\n") if l.startswith("#")]
    return ["##source=bucketmap --vcf" if l.startswith("##source=") else l for l in head if not l.startswith(GVCF_HEAD)]


def summary_line(blks, word0):
    length = sum(len(w) for w in word0)
    on = sum(b[2] - b[1] for b in blks)
    band0 = sum(b[2] - b[1] for b in blks if b[3] == 0)  # bases, like the other figures
    under = sum(int(((w & EXCLUDED) != 0).sum()) for w in word0)
    none = sum(int(((w & NO_ALLELE) != 0).sum()) for w in word0)
    return f"Blocks: {len(blks)} blocks on {on} of {length} bases ({band0} in band 0, {under} under variant lines, {none} without a reference allele)"
