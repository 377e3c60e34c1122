"""Designed cases of the mapping statistics rule (include/bmq.h), worked out by hand.  A case takes an ENGINE --
engine(records, skip=None, **params) -> (tallies, tables) as stats_rule.run returns them -- and asserts the values; the Python
rule, host/stats.h and the device all go through the same cases (tests/test_stats.py, tests/test_stats_gpu.py).  Also the
record sets the random comparisons share."""
import struct

import numpy as np

from pileup_cases import CODE_OF, cigar_ops, many_ops_record, random_records, rec_seq
from stats_rule import T


def qrec(flag, cigar, letters, qual=None, ref=0, pos=100, mapq=30, next_ref=0, next_pos=0, tlen=0, name=b"r"):
    """A record from a CIGAR string and sequence letters (A C G T N, and = M R for other codes) with its mate fields; quality
    40 unless given."""
    qual = bytes([40] * len(letters)) if qual is None else bytes(qual)
    b = bytearray(rec_seq(ref, pos, flag, cigar_ops(cigar), [CODE_OF[ch] for ch in letters], qual, name, mapq=mapq))
    struct.pack_into("<iii", b, 24, next_ref, next_pos, tlen)
    return bytes(b)


def cells(table):
    """{(row, column): count} of the non-zero cells."""
    return {(int(r), int(c)): int(table[r, c]) for r, c in zip(*np.nonzero(table))}


def tally(t, **want):
    got = {name: int(t[T[name]]) for name in want}
    assert got == want


COMP = str.maketrans("ACGT", "TGCA")


def case_forward_and_reverse_mirror(engine):
    """One read, ACGTN with the qualities 10 .. 50, aligned 1S 2= 1X 1M: as a forward record and as the reverse record of the
    same read (sequence reverse-complemented, qualities and CIGAR reversed) it fills the same cells."""
    fwd = qrec(0, "1S2=1X1M", "ACGTN", [10, 20, 30, 40, 50])
    rev = qrec(0x10, "1M1X2=1S", "ACGTN".translate(COMP)[::-1], [50, 40, 30, 20, 10])
    want_bc = {(0, 0): 1, (1, 1): 1, (2, 2): 1, (3, 3): 1, (4, 4): 1}
    want_qc = {(0, 10): 1, (1, 20): 1, (2, 30): 1, (3, 40): 1, (4, 50): 1}
    want_mc = {(0, 4): 1, (1, 0): 1, (2, 0): 1, (3, 1): 1, (4, 2): 1}
    for one in (fwd, rev):
        t, tab = engine([one])
        assert cells(tab["BC"]) == want_bc and cells(tab["QC"]) == want_qc and cells(tab["MC"]) == want_mc
        tally(t, records=1, bases=5, bases_m=1, bases_eq=2, bases_x=1, soft_clipped_bases=1, qual_sum=150, qual_bases=5, reverse_strand=int(one is rev))
        assert cells(tab["GC"]) == {(50, 0): 1} and cells(tab["RL"]) == {(5, 0): 1}
    t, tab = engine([fwd, rev])
    assert cells(tab["BC"]) == {k: 2 for k in want_bc} and cells(tab["MC"]) == {k: 2 for k in want_mc}


def case_odd_l_seq(engine):
    """Three bases: the last one is the high nibble of a byte whose low nibble is no base."""
    t, tab = engine([qrec(0, "3M", "ACG"), qrec(0x10, "3M", "ACG")])
    assert cells(tab["BC"]) == {(0, 0): 1, (1, 1): 1, (2, 2): 1, (2, 3): 1, (1, 2): 1, (0, 1): 1}
    tally(t, bases=6, bases_m=6, bases_beyond_cycle=0)
    assert cells(tab["GC"]) == {(67, 0): 2}              # (200 * 2 + 3) / 6 = 67


def case_quality_absent(engine):
    """0xFF in some bytes and in all: no quality, so no cell of QC and nothing in the sums; BC and MC take the bases."""
    t, tab = engine([qrec(0, "3M", "AAA", [0xFF, 7, 0xFF]), qrec(0, "2M", "CC", [0xFF, 0xFF])])
    assert cells(tab["QC"]) == {(1, 7): 1}
    tally(t, qual_sum=7, qual_bases=1, bases=5)
    assert cells(tab["BC"]) == {(0, 0): 1, (1, 0): 1, (2, 0): 1, (0, 1): 1, (1, 1): 1}


def case_quality_columns(engine):
    """62 and 63 have columns of their own; 64 and 93 share 63.  The sum takes the bytes as they are."""
    t, tab = engine([qrec(0, "4M", "ACGT", [62, 63, 64, 93])])
    assert cells(tab["QC"]) == {(0, 62): 1, (1, 63): 1, (2, 63): 1, (3, 63): 1}
    tally(t, qual_sum=282, qual_bases=4)


def case_codes_that_are_no_letter(engine):
    """Codes 0, 3, 5 and 15 are `other`, on either strand; a read of them alone has no GC row and counts in reads_no_acgt."""
    t, tab = engine([qrec(0, "5M", "=MRNA"), qrec(0x10, "4M", "NNNN"), qrec(0, "2M", "NN")])
    assert cells(tab["BC"]) == {(0, 4): 3, (1, 4): 3, (2, 4): 2, (3, 4): 2, (4, 0): 1}
    assert cells(tab["GC"]) == {(0, 0): 1}
    tally(t, reads_no_acgt=2, primary=3)


def case_gc_rows_round_half_up(engine):
    """g = 1 of n = 8 is 12.5 %: row 13.  g = 1 of n = 200 is 0.5 %: row 1.  Only A C G T count in n."""
    t, tab = engine([qrec(0, "8M", "CAAAAAAA"), qrec(0, "200M", "G" + "T" * 199), qrec(0, "4M", "GCNN"), qrec(0x10, "3M", "AAT"), qrec(0, "9M", "CNAAAAAAA")])
    assert cells(tab["GC"]) == {(13, 0): 2, (1, 0): 1, (100, 0): 1, (0, 0): 1}
    tally(t, reads_no_acgt=0)


def case_records_without_an_alignment(engine):
    """l_seq == 0 with a CIGAR, no CIGAR with a sequence, and the long-CIGAR placeholder: mapped, not aligned; the placeholder is
    left_out.  Their bases still count in the read-level tables."""
    no_seq = qrec(0, "4M", "")
    no_cigar = qrec(0, "", "AC")
    placeholder = qrec(0, "3S9N", "GGG")
    not_quite = qrec(0, "3S9M", "GGG" + "A" * 9)         # an S of l_seq bases it is not: 12 bases
    t, tab = engine([no_seq, no_cigar, placeholder, not_quite])
    tally(t, records=4, mapped=4, aligned_records=1, left_out=1, bases=17, bases_m=9, soft_clipped_bases=3)
    assert cells(tab["RL"]) == {(0, 0): 1, (2, 0): 1, (3, 0): 1, (12, 0): 1}
    assert cells(tab["MC"]) == {**{(c, 4): 1 for c in range(3)}, **{(c, 2): 1 for c in range(3, 12)}}
    assert int(tab["BC"].sum()) == 17 and cells(tab["MAPQ"]) == {(30, 0): 4}


def case_indels_and_clips(engine):
    """A leading I; a D before any query base (dropped from MC, counted everywhere else); a D on a reverse record, at the cycle of
    the base before it in the record; S at both ends; a D of length 0 and an I of length 0 count nowhere; 300 and 255 share a row."""
    lead = qrec(0, "2I3M", "AAAAA")                      # I at cycles 0 1, M at 2 3 4
    d_first = qrec(0, "2D3M", "AAA")                     # qc == 0
    d_rev = qrec(0x10, "2M1D3M", "AAAAA")                # qc == 2: query index 1, cycle 5 - 1 - 1 = 3
    clips = qrec(0, "1S2M2S", "AAAAA")
    empty_ops = qrec(0, "2M0D0I1M", "AAA")
    long_ones = qrec(0, "1M300D255I1M", "A" * 257)
    t, tab = engine([lead, d_first, d_rev, clips, empty_ops, long_ones])
    tally(t, insertions=2, deletions=3, inserted_bases=257, deleted_bases=303, soft_clipped_bases=3, bases_m=3 + 3 + 5 + 2 + 3 + 2)
    assert cells(tab["ID"]) == {(2, 0): 1, (2, 1): 1, (1, 1): 1, (255, 0): 1, (255, 1): 1}
    mc = cells(tab["MC"])
    assert {k: v for k, v in mc.items() if k[1] == 5} == {(3, 5): 1, (0, 5): 1}          # d_rev, and long_ones's at query index 0
    assert {k: v for k, v in mc.items() if k[1] == 4} == {(0, 4): 1, (3, 4): 1, (4, 4): 1}
    assert mc[(0, 3)] == 1 and mc[(1, 3)] == 2 and mc[(255, 3)] == 1 and (256, 3) not in mc
    assert mc[(0, 2)] == 4 and mc[(256, 2)] == 1


def case_insert_sizes(engine):
    """tlen of -5, 0, 1, I - 1, I and I + 1 with I = 10, inward, outward and the two other orientations."""
    recs = []
    for way in (0x20, 0x10, 0x00, 0x30):
        recs += [qrec(0x41 | way, "2M", "AC", tlen=v) for v in (-5, 0, 1, 9, 10, 11)]
    recs += [qrec(0x41 | 0x20, "2M", "AC", tlen=3, next_ref=1), qrec(0x41 | 0x20 | 0x8, "2M", "AC", tlen=3), qrec(0x41 | 0x24, "2M", "AC", tlen=3),
             qrec(0x20, "2M", "AC", tlen=3), qrec(0x921, "2M", "AC", tlen=3)]   # other reference, mate unmapped, unmapped, not paired, not primary
    t, tab = engine(recs, max_insert=10)
    assert cells(tab["IS"]) == {(1, 0): 1, (9, 0): 1, (10, 0): 2, (1, 1): 1, (9, 1): 1, (10, 1): 2, (1, 2): 2, (9, 2): 2, (10, 2): 4}
    tally(t, pairs_in_is=16, mate_other_ref=1)
    assert tab["IS"].shape == (11, 3)


def case_mates_on_two_references(engine):
    t, tab = engine([qrec(0x41, "1M", "A", ref=0, next_ref=1, mapq=4, tlen=50), qrec(0x81, "1M", "A", ref=1, next_ref=0, mapq=5, tlen=50),
                     qrec(0x41, "1M", "A", ref=1, next_ref=1, mapq=0), qrec(0x41, "1M", "A", ref=0, next_ref=-1, mapq=255)])
    tally(t, both_mapped=4, mate_other_ref=3, mate_other_ref_mapq5=2, pairs_in_is=0, mapq0=1)
    assert cells(tab["MAPQ"]) == {(4, 0): 1, (5, 0): 1, (0, 0): 1, (255, 0): 1} and not tab["IS"].any()


def case_flag_bits(engine):
    """Every flag bit of the tallies alone, and combined: 0x900 is not primary, 0x1 counts on primary records only, 0x2 and 0x40
    only with 0x1."""
    flags = [0x0, 0x1, 0x2, 0x4, 0x8, 0x10, 0x40, 0x100, 0x200, 0x400, 0x800, 0x900, 0x1 | 0x2 | 0x40, 0x1 | 0x8 | 0x80, 0x1 | 0x2 | 0x4, 0x101]
    t, tab = engine([qrec(f, "1M", "A") for f in flags])
    tally(t, records=16, primary=12, secondary=3, supplementary=2, duplicates=1, qc_failed=1, mapped=14, primary_mapped=10, paired=4, read1=1, read2=1,
          properly_paired=1, both_mapped=2, singletons=1, mate_other_ref=0, mate_other_ref_mapq5=0, reverse_strand=1, mapq0=0, bases=12, bases_mapped=10,
          aligned_records=14, left_out=0, bases_m=14, qual_sum=480, qual_bases=12, pairs_in_is=0)
    assert cells(tab["MAPQ"]) == {(30, 0): 14} and cells(tab["RL"]) == {(1, 0): 12}
    assert cells(tab["BC"]) == {(0, 0): 11, (0, 3): 1} and cells(tab["MC"]) == {(0, 2): 14} and cells(tab["QC"]) == {(0, 40): 12}


def case_skip_bytes(engine):
    recs = [qrec(0, "2M", "AC"), qrec(0x10, "3M", "GGG", mapq=7), qrec(0x41 | 0x20, "1M", "T", tlen=4)]
    t, tab = engine(recs, skip=[0, 1, 0])
    want_t, want = engine([recs[0], recs[2]])
    assert list(t) == list(want_t) and all((tab[k] == want[k]).all() for k in tab)
    tally(t, records=2, bases=3, reverse_strand=0)
    t, tab = engine(recs, skip=[1, 1, 1])
    assert not any(t) and not any(tab[k].any() for k in tab)


def border_reads():
    """A 40-base read as a forward and as a reverse record, 10S 30M, letters chosen so that every border shows: with
    max_cycle = 30 the cycles 29 and 30 are the last kept and the first dropped; a window of 20 cycles in LDS ends between the
    cycles 19 and 20."""
    fwd = ["A"] * 40
    fwd[19], fwd[20], fwd[29], fwd[30] = "C", "G", "T", "C"
    rev = ["A"] * 40                                     # cycle c is query index 39 - c, complemented
    rev[39 - 19], rev[39 - 20], rev[39 - 29], rev[39 - 30] = "C", "T", "G", "C"          # sequenced: G at 19, A at 20, C at 29, G at 30
    qual = list(range(40))
    return [qrec(0, "10S30M", "".join(fwd), qual), qrec(0x10, "10S30M", "".join(rev), qual[::-1])]


def case_cycle_borders(engine):
    t, tab = engine(border_reads(), max_cycle=30)
    bc = tab["BC"]
    assert bc.shape == (30, 5) and bc.sum(axis=1).tolist() == [2] * 30 and tab["RL"].shape == (31, 1)
    assert bc[19].tolist() == [0, 1, 1, 0, 0] and bc[20].tolist() == [1, 0, 1, 0, 0] and bc[29].tolist() == [0, 1, 0, 1, 0] and bc[18].tolist() == [1, 0, 0, 1, 0]   # the reverse record's A was sequenced as T
    tally(t, bases=80, bases_beyond_cycle=20, qual_bases=80, qual_sum=2 * sum(range(40)), soft_clipped_bases=20, bases_m=60)
    assert cells(tab["RL"]) == {(30, 0): 2}
    assert cells(tab["QC"]) == {(c, c): 2 for c in range(30)}
    # forward: S at the cycles 0 .. 9, M from 10 on; reverse: its S is the query's start, the cycles 30 .. 39 -- dropped
    mc = tab["MC"]
    assert mc[:, 4].tolist() == [1] * 10 + [0] * 20 and mc[:, 2].tolist() == [1] * 10 + [2] * 20
    whole_t, whole = engine(border_reads(), max_cycle=40)
    assert whole["BC"][:30].tolist() == bc.tolist() and whole_t[T["bases_beyond_cycle"]] == 0 and whole["BC"][30].tolist() == [0, 1, 1, 0, 0]


DESIGNED = [case_forward_and_reverse_mirror, case_odd_l_seq, case_quality_absent, case_quality_columns, case_codes_that_are_no_letter,
            case_gc_rows_round_half_up, case_records_without_an_alignment, case_indels_and_clips, case_insert_sizes, case_mates_on_two_references,
            case_flag_bits, case_skip_bytes, case_cycle_borders]


# ---- record sets ----
def with_mates(records, seed):
    """The records with random mate fields: some paired flags, next_refID equal to refID or not, and template lengths around the
    borders of max_insert 8000 and of a small one."""
    rng = np.random.default_rng(seed)
    out = []
    for r in records:
        b = bytearray(r)
        flag = struct.unpack_from("<H", b, 18)[0]
        ref = struct.unpack_from("<i", b, 4)[0]
        if rng.random() < 0.7:
            flag |= 1 | int(rng.choice([0x40, 0x80])) | int(rng.choice([0, 0x20])) | (2 if rng.random() < 0.6 else 0) | (8 if rng.random() < 0.1 else 0)
        tlen = int(rng.choice([-300, 0, 1, 2, 49, 50, 51, 300, 7999, 8000, 8001, 70000, int(rng.integers(1, 600))]))
        struct.pack_into("<H", b, 18, flag)
        struct.pack_into("<iii", b, 24, ref if rng.random() < 0.85 else ref + 1, 5, tlen)
        out.append(bytes(b))
    return out


def random_set(n, seed):
    """n records of pileup_cases.random_records (every flag, MAPQ, clip, indel, quality, empty and unplaced records) with mates."""
    return with_mates(random_records(n, seed), seed + 1)


def short_reads(n, length=150, seed=3):
    """n records of `length` bases, =/X/I/D CIGARs between clips, both strands, pairs with template lengths around 400: built
    with numpy, for the sizes at which a grid-stride loop turns."""
    rng = np.random.default_rng(seed)
    codes = np.array([1, 2, 4, 8, 15], np.uint8)[rng.choice(5, (n, length), p=[0.27, 0.22, 0.22, 0.27, 0.02])]
    qual = rng.choice(np.array([2, 11, 25, 37, 40, 41, 255], np.uint8), (n, length))
    out = []
    for k in range(n):
        a, b = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        mid = length - a - b
        x = int(rng.integers(1, mid - 8))
        ops = [(a, "S")] * (a > 0) + [(x, "="), (1, "X"), (2, "D"), (3, "I"), (mid - x - 4, "="), ] + [(b, "S")] * (b > 0) if k % 3 else [(length, "M")]
        cigar = "".join(f"{l}{o}" for l, o in ops)
        rev = int(rng.integers(0, 2))
        flag = 0x1 | (0x40 if k % 2 == 0 else 0x80) | 0x2 | (0x10 if rev else 0x20) | (0x400 if k % 50 == 7 else 0)
        r = bytearray(rec_seq(k % 3, 1000 + k, flag, cigar_ops(cigar), codes[k], qual[k].tobytes(), b"s%d" % k, mapq=int(rng.choice([0, 3, 20, 60]))))
        struct.pack_into("<iii", r, 24, k % 3, 1200 + k, int(rng.integers(250, 560)) * (1 if k % 2 == 0 else -1))
        out.append(bytes(r))
    return out


def ops_record(n_ops, seed):
    return with_mates([many_ops_record(0, 17, n_ops, seed)], seed)[0]


def long_read(length=70000, seed=11, flag=0x10):
    """One record of `length` bases, 1 000 = then an X, and so on, between two clips."""
    rng = np.random.default_rng(seed)
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, length)]
    qual = rng.integers(0, 94, length).astype(np.uint8)
    ops, left = [(7, "S")], length - 7 - 5
    while left > 0:
        take = min(left, 1000)
        ops.append((take, "="))
        left -= take
        if left > 0:
            ops.append((1, "X"))
            left -= 1
    ops.append((5, "S"))
    return rec_seq(0, 0, flag, cigar_ops("".join(f"{l}{o}" for l, o in ops)), codes, qual.tobytes(), b"long", mapq=60)
