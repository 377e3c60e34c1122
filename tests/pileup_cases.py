"""Records and references for the pileup tests (tests/test_pileup.py without a GPU, tests/test_pileup_gpu.py with one): reads
cut from a sample of a random reference -- the reference with planted substitutions, insertions and deletions, so that reads
agree on them -- with a few random errors each, spread over depth_cases.REF_LENS so that reference borders fall everywhere
against the site passes' tiles of 2 048; and the edge list.  Every record carries a real 4-bit sequence and satisfies what
bmp_add checks."""
import struct

import numpy as np

import depth_cases
from depth_cases import EDGE_REFS, REF_LENS, SIZES, op, query_len, with_mapq  # noqa: F401
from test_markdup_gpu import OPS

QUALS = np.array([0, 1, 12, 13, 14, 30, 40, 93, 254, 255], np.uint8)
CODE_OF = {"=": 0, "A": 1, "C": 2, "M": 3, "G": 4, "R": 5, "T": 8, "N": 15}
LETTER_CODES = np.array([1, 2, 4, 8], np.uint8)      # A C G T
ACGT = np.frombuffer(b"ACGT", np.uint8)
ERROR_CODES = np.array([1, 2, 4, 8, 15, 0, 3], np.uint8)   # what a random error puts in a base's place
FLAGS = [0, 0, 0, 0, 0, 0, 0x800, 1 | 0x40, 1 | 0x80, 4, 0x100, 0x200, 0x400]


def rec_seq(ref, pos, flag, ops, codes, qual, name=b"r", tags=b"", mapq=30):
    """A BAM record with the 4-bit codes as its sequence (the high nibble first)."""
    l_seq = len(qual)
    codes = np.asarray(codes, np.uint8)
    assert codes.size == l_seq
    padded = np.concatenate([codes, np.zeros(l_seq & 1, np.uint8)])
    packed = (padded[0::2] << 4 | padded[1::2]).astype(np.uint8).tobytes()
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, mapq, 4680, len(ops), flag, l_seq, -1, -1, 0) + name + b"\0"
    body += struct.pack(f"<{len(ops)}I", *ops) + packed + bytes(qual) + tags
    return struct.pack("<I", len(body)) + body


def cigar_ops(cigar):
    out, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append(int(num) << 4 | OPS.index(ch))
            num = ""
    return out


def rec_letters(ref, pos, cigar, letters, qual=None, name=b"r", flag=0, mapq=30):
    """A record from a CIGAR string and sequence letters (A C G T N, and = M R for other codes); quality 40 unless given."""
    qual = bytes([40] * len(letters)) if qual is None else bytes(qual)
    return rec_seq(ref, pos, flag, cigar_ops(cigar), [CODE_OF[ch] for ch in letters], qual, name, mapq=mapq)


def with_sequence(record, seed):
    """The record with random 4-bit codes (mostly A C G T) in place of its sequence bytes."""
    rng = np.random.default_rng(seed)
    b = bytearray(record)
    l_name, n_cigar, l_seq = b[12], struct.unpack_from("<H", b, 16)[0], struct.unpack_from("<I", b, 20)[0]
    at = 36 + l_name + 4 * n_cigar
    codes = rng.choice(np.array([1, 2, 4, 8, 15, 0, 3], np.uint8), l_seq + (l_seq & 1), p=[0.23, 0.23, 0.23, 0.23, 0.04, 0.02, 0.02])
    b[at: at + (l_seq + 1) // 2] = (codes[0::2] << 4 | codes[1::2]).astype(np.uint8).tobytes()
    return bytes(b)


# ---- references and their samples ----
def references(ref_len=REF_LENS, seed=1):
    """One bytes object per reference: random A C G T, here and there lower case, N, n or another letter."""
    rng = np.random.default_rng(seed)
    out = []
    for n in ref_len:
        a = ACGT[rng.integers(0, 4, n)].copy()
        lower = rng.random(n) < 0.05
        a[lower] |= 0x20
        odd = rng.random(n) < 0.01
        a[odd] = np.frombuffer(b"NnRy-", np.uint8)[rng.integers(0, 5, int(odd.sum()))]
        out.append(a.tobytes())
    return out


class Sample:
    """The reference with planted variants: sub[p] (a code, 0 where none), and sorted indel positions with a length each
    (> 0: that many bases inserted behind p, < 0: that many positions deleted from p on)."""

    def __init__(self, bases, seed):
        rng = np.random.default_rng(seed)
        n = len(bases)
        ref = np.frombuffer(bases, np.uint8)
        upper = ref & 0xDF
        self.codes = np.full(n, 15, np.uint8)
        for letter, code in zip(b"ACGT", LETTER_CODES):
            self.codes[upper == letter] = code
        planted = rng.random(n) < 0.02
        self.codes[planted] = LETTER_CODES[rng.integers(0, 4, int(planted.sum()))]
        at = np.flatnonzero(rng.random(n) < 0.012)
        self.indel_at = at
        self.indel_len = np.where(rng.random(at.size) < 0.5, 1, -1) * rng.integers(1, 4, at.size)


class Pool:
    """Uniform numbers drawn from rng a hundred thousand at a time: a numpy call per number costs more than the records."""

    def __init__(self, rng):
        self.rng, self.u, self.at = rng, [], 0

    def random(self):
        if self.at == len(self.u):
            self.u, self.at = self.rng.random(100000).tolist(), 0
        self.at += 1
        return self.u[self.at - 1]

    def below(self, n):
        return int(self.random() * n)

    def between(self, lo, hi):
        return lo + int(self.random() * (hi - lo))

    def letters(self, n):
        return LETTER_CODES[self.rng.integers(0, 4, n)] if n else LETTER_CODES[:0]


def cut_read(rng, sample, pos, length, n_ref_bases):
    """(ops, codes) of a read of about `length` query bases from the sample at pos; past the end of the reference the read
    goes on with random bases (they do not count).  rng is a Pool."""
    ops, parts, p, have = [], [], pos, 0

    def block(n):
        nonlocal p, have
        inside = sample.codes[p: min(p + n, n_ref_bases)]
        parts.append(inside)
        if inside.size < n:
            parts.append(rng.letters(n - inside.size))
        kind = "M" if rng.random() < 0.8 else "=X"[rng.below(2)]
        ops.append(op(n, kind))
        p += n
        have += n

    lo, hi = np.searchsorted(sample.indel_at, [pos, pos + length])
    for k in range(lo, hi):
        at, n = int(sample.indel_at[k]), int(sample.indel_len[k])
        if at < p or have >= length:
            continue
        block(at + 1 - p)                                # up to and with the anchor
        if n > 0:
            parts.append(rng.letters(n))
            ops.append(op(n, "I"))
            have += n
        else:
            ops.append(op(-n, "D"))
            p += -n
    if have < length:
        block(length - have)
    elif OPS[ops[-1] & 15] == "D":                       # a read does not end on a deletion
        block(1)
    codes = np.concatenate(parts).astype(np.uint8)
    if rng.random() < 1 - 0.99 ** codes.size:            # about one base in a hundred is wrong
        wrong = rng.rng.integers(0, codes.size, 1 + rng.below(1 + codes.size // 50))
        codes[wrong] = ERROR_CODES[rng.rng.integers(0, len(ERROR_CODES), wrong.size)]
    return ops, codes


def random_records(n, seed, ref_len=REF_LENS, bases=None):
    """n records over the references; most are reads of the sample, with every flag, MAPQ, clip and an unplaced or empty record
    now and then, as depth_cases.random_records has them."""
    bases = references(ref_len) if bases is None else bases
    samples = [Sample(b, 1000 + r) for r, b in enumerate(bases)]
    rng = Pool(np.random.default_rng(seed))
    out = []
    for k in range(n):
        ref = rng.below(len(ref_len))
        if rng.random() < 0.5:
            ref = len(ref_len) - 1 - rng.below(min(2, len(ref_len)))                      # most on the longer ones
        length = ref_len[ref]
        how = rng.random()
        pos = rng.below(length) if how < 0.6 else max(0, length - 1 - rng.below(70)) if how < 0.9 else 0
        flag = 16 * rng.below(2) | FLAGS[rng.below(len(FLAGS))]
        read_len = rng.between(1, 90) if rng.random() < 0.97 else rng.between(600, 3000)
        ops, codes = cut_read(rng, samples[ref], pos, read_len, length)
        if rng.random() < 0.02:
            ops.insert(rng.below(len(ops) + 1), op(rng.between(1, 30), "NP"[rng.below(2)]))
        lead = rng.between(1, 9) if rng.random() < 0.2 else 0                # soft clips, odd and even
        trail = rng.between(1, 9) if rng.random() < 0.2 else 0
        ops = [op(lead, "S")] * (lead > 0) + ops + [op(trail, "S")] * (trail > 0)
        if rng.random() < 0.1:
            ops.insert(0, op(rng.between(1, 4), "H"))
        if lead or trail:
            codes = np.concatenate([rng.letters(lead), codes, rng.letters(trail)])
        if rng.random() < 0.03:
            ops, codes = [], codes[: rng.below(9)]
        if rng.random() < 0.02:
            ref, pos = -1, -1
        assert not ops or query_len(ops) == codes.size
        if ops and rng.random() < 0.05:
            codes = codes[:0]                            # no sequence: left out
        qual = QUALS[rng.rng.integers(0, len(QUALS), codes.size)].tobytes()
        out.append(rec_seq(ref, pos, flag, ops, codes, qual, b"q%d" % k, b"t" * rng.below(9), rng.below(256)))
    return out


# ---- the edge list ----
def edge_bases():
    """The bases of EDGE_REFS: ACGT repeated (the base of p is "ACGT"[p % 4]), with lower case at 100 .. 103 of the first one, N at
    104, n at 105 and R at 106; the second one starts with C; the third is g."""
    first = bytearray(b"ACGT" * 250)
    first[100:107] = b"acgtNnR"
    return [bytes(first), (b"CGTA" * 13)[:50], b"g"]


def edge_records():
    """depth_cases.edge_records() remade with a sequence, then what only the pileup tells apart; names are unique."""
    out = [with_sequence(r, k) for k, r in enumerate(depth_cases.edge_records())]
    L = rec_letters
    out += [
        # reference 0 at 600 .. 603 is A C G T: C C C C with the qualities 13 12 255 0 under min_bq 13
        L(0, 600, "4M", "CCCC", [13, 12, 255, 0], b"bq_steps"),
        L(0, 610, "4M", "GGGG", name=b"mapq_at", mapq=20), L(0, 610, "4M", "GGGG", name=b"mapq_below", mapq=19),
        L(0, 620, "3S5M", "NNNACGTA", name=b"odd_after_3S"),          # query index 3 starts the block: a low nibble first
        L(0, 630, "2M1I4M", "GTAACGT", name=b"odd_after_I"),          # 630 631 are G T; behind the I the query index is 3
        L(0, 640, "5M", "ACGTT", name=b"odd_l_seq"),
        L(0, 650, "6M", "=MRNAC", name=b"other_codes"),               # codes 0 3 5 15: N
        L(0, 660, "2I4M", "TTACGT", name=b"leading_I"), L(0, 664, "2S2I4M", "NNTTACGT", name=b"I_after_S"),
        L(0, 670, "2M2D1I3M", "GTCGTA", name=b"I_after_D"),           # the anchor is the last deleted position, 673
        L(0, 680, "2M3N1I2M", "ACTAC", name=b"I_after_MN"),           # an M came before: counts, at 684
        L(0, 690, "3N1I2M", "TGT", name=b"I_after_N_only"),           # dropped
        L(1, 48, "2M1I", "TAC", name=b"I_on_the_last_base"),          # anchor 49, the last base of reference 1
        L(1, 48, "3M1I", "TACC", name=b"I_off_the_end"),              # anchor 50: dropped, and the third M base too
        L(1, 45, "2M10D2M", "GTAA", name=b"D_over_the_end"),          # DEL at 47 48 49; the last block lies beyond
        L(0, 100, "7M", "CCCCCCC", name=b"on_odd_reference_a"), L(0, 100, "7M", "CCCCCCC", name=b"on_odd_reference_b"),
        L(0, 102, "1M2D2M", "GAA", name=b"del_on_N_a"), L(0, 102, "1M2D2M", "GAA", name=b"del_on_N_b"),
        L(2, 0, "1M", "T", name=b"one_base_t"), L(2, 0, "1M", "T", name=b"one_base_t2"), L(2, 0, "1M", "G", name=b"one_base_g"),
    ]
    # the fraction at equality: one T among four reads on an A (700), among five (704)
    for p, n in ((700, 4), (704, 5)):
        out += [L(0, p, "1M", "T" if k == 0 else "A", name=b"frac%d_%d" % (n, k)) for k in range(n)]
    names = [r[36: 36 + r[12] - 1] for r in out]
    assert len(set(names)) == len(names)
    return out


def many_ops_record(ref, pos, n_ops=60000, seed=7):
    """depth_cases.many_ops_record (1=1X ... with D, I, N and P mixed in, between clips) with a sequence."""
    return with_sequence(depth_cases.many_ops_record(ref, pos, True, n_ops), seed)


def parse_check_output(text):
    """(sites, stats, counts) of tests/cpp/pileup_check.cpp's output."""
    lines = text.split("\n")
    n = int(lines[0].split()[1])
    sites = [tuple(int(x) for x in l.split()) for l in lines[1: 1 + n]]
    assert lines[1 + n] == "stats"
    rest = lines[2 + n:]
    n_ref = sum(1 for l in rest if l.startswith("counts"))
    stats = [[int(x) for x in l.split()] for l in rest[:n_ref]]
    counts = [np.array([int(x) for x in l.split()[1:]], np.uint32).reshape(-1, 8) for l in rest[n_ref: 2 * n_ref]]
    return sites, stats, counts
