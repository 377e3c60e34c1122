"""Records for the indel tests (tests/test_indel.py without a GPU, tests/test_indel_gpu.py with one): hand-made reads that carry
one insertion or deletion at a chosen place, and the lists of edge placements.  Built with pileup_cases' record builders; every
record satisfies what bmn_add checks."""
import numpy as np

from pileup_cases import LETTER_CODES, op, rec_letters, rec_seq

ABC = "ACGT"
L = rec_letters


def ins_record(ref, pos, lead, ins, name=b"r", mapq=30):
    """lead M bases, the insertion, four M bases: the anchor is pos + lead - 1, the insertion's query offset is lead."""
    letters = (ABC * (lead // 4 + 1))[:lead] + ins + ABC
    return rec_letters(ref, pos, f"{lead}M{len(ins)}I4M", letters, name=name, mapq=mapq)


def edge_placements():
    """(ref_len, records, the number of events each gives alone)"""
    refs = [50, 30]
    cases = [
        (L(0, 5, "2I4M", "TTACGT", name=b"I_first"), 0), (L(0, 5, "2S2I4M", "NNTTACGT", name=b"I_after_S"), 0),
        (L(0, 5, "4M2I", "ACGTTT", name=b"I_last"), 0), (L(0, 5, "4M2I3S", "ACGTTTNNN", name=b"I_then_only_S"), 0),
        (L(0, 40, "5M5D", "ACGTA", name=b"D_to_the_end"), 1), (L(0, 40, "5M6D", "ACGTA", name=b"D_one_past"), 0),
        (L(0, 0, "1M1I3M", "ACGTA", name=b"anchor_0"), 1), (L(0, 48, "1M1I1M", "ACG", name=b"anchor_len_2"), 1),
        (L(0, 48, "1M1D", "A", name=b"D_on_the_last_base"), 1), (L(0, 20, "3M2I2D3M", "ACGTTACG", name=b"I_then_D"), 2),
        (L(0, 49, "3M", "ACG", name=b"pos_on_the_last_base"), 0), (L(1, 28, "1M1I1M", "ACG", name=b"other_anchor_len_2"), 1),
        (L(1, 29, "1M1I1M", "ACG", name=b"I_with_nothing_inside_behind"), 0), (L(0, 30, "2M3N1I2M", "ACTAC", name=b"I_after_MN"), 1),
        (L(0, 30, "3N1I2M", "TGT", name=b"I_after_N_only"), 0), (L(0, 10, "2M1D1I2M", "ACGTA", name=b"I_after_D"), 2),
    ]
    return refs, [r for r, _ in cases], [n for _, n in cases]


def many_indel_ops(ref, pos, n_ops, seed):
    """One record whose ops alternate 1M 1I 1M 1D ...; the inserted bases are random, so the alleles differ."""
    rng = np.random.default_rng(seed)
    ops = [op(1, "MIMD"[k % 4]) for k in range(n_ops)]
    l_seq = sum(1 for k in range(n_ops) if k % 4 != 3)
    codes = LETTER_CODES[rng.integers(0, 4, l_seq)]
    return rec_seq(ref, pos, 0, ops, codes, bytes([30]) * l_seq, b"ops%d" % n_ops)


def same_anchor_records(n_distinct, n_equal):
    """n_distinct different five-base insertions on anchor 54 of reference 0, n_equal equal ones on anchor 13 of reference 1."""
    assert n_distinct <= 4 ** 5
    out = [ins_record(0, 50, 5, "".join(ABC[(k >> (2 * j)) & 3] for j in range(5)), b"d%d" % k) for k in range(n_distinct)]
    return out + [ins_record(1, 10, 4, "GG", b"e%d" % k) for k in range(n_equal)]


def threshold_records():
    """Two reads with an inserted C on anchor 12, three on anchor 32."""
    return [ins_record(0, 10, 3, "C", b"two%d" % k) for k in range(2)] + [ins_record(0, 30, 3, "C", b"three%d" % k) for k in range(3)]


def min_frac_records():
    """One insertion among four reads that span its anchor: exactly 250 000 ppm."""
    return [ins_record(0, 10, 4, "C", b"with")] + [L(0, 10, "8M", "ACGTACGT", name=b"without%d" % k) for k in range(3)]


def homopolymer_reads(fasta_text, read_len, run=5, n_each=6):
    """(FASTQ text, reference name, the 0-based start of the run, its letter, the letter before it): reads of read_len bases
    from both strands over the first run of `run` equal letters well inside the first record of a FASTA text, each with one base
    of the run deleted -- at another place of the run from read to read, which is one and the same deletion."""
    name, seq = None, ""
    for line in fasta_text.split("\n"):
        if line.startswith(">"):
            if name is not None:
                break
            name = line[1:].split(" ")[0]
        else:
            seq += line.strip().upper()
    start = next(p for p in range(read_len, len(seq) - 2 * read_len)
                 if len(set(seq[p: p + run])) == 1 and seq[p] in "ACGT" and seq[p - 1] != seq[p] and seq[p + run] != seq[p] and seq[p - 1] in "ACGT")
    comp = str.maketrans("ACGT", "TGCA")
    out = ""
    for k in range(2 * n_each):
        first = start - 12 - 3 * (k // 2)                # the run lies well inside every read
        piece = seq[first: first + read_len + 1]
        gone = start - first + k % run
        read = piece[:gone] + piece[gone + 1:]
        if k % 2:
            read = read.translate(comp)[::-1]
        out += f"@homo{k}\n{read}\n+\n{'I' * read_len}\n"
    return out, name, start, seq[start], seq[start - 1]
