"""The mapping statistics rule of include/bmq.h in plain Python and numpy: the yardstick of tests/test_stats.py and
tests/test_stats_gpu.py.  run() counts, text() writes the file of --stats, summary_line() the line on stderr.  Nothing here
knows the C++ or the kernels; a record is the bytes of a BAM record led by its block_size."""
import struct

import numpy as np

N_TALLIES = 35
TABLES = ("MAPQ", "RL", "IS", "GC", "ID", "BC", "QC", "MC")          # BMQ_T_* in order
WIDTH = dict(MAPQ=1, RL=1, IS=3, GC=1, ID=2, BC=5, QC=64, MC=6)
DEFAULTS = dict(max_cycle=1024, max_insert=8000)                      # the command line's
NAMES = ("records", "primary", "secondary", "supplementary", "duplicates", "qc_failed", "mapped", "primary_mapped", "paired", "read1", "read2",
         "properly_paired", "both_mapped", "singletons", "mate_other_ref", "mate_other_ref_mapq5", "reverse_strand", "mapq0", "bases", "bases_mapped",
         "aligned_records", "left_out", "bases_m", "bases_eq", "bases_x", "inserted_bases", "deleted_bases", "soft_clipped_bases", "insertions",
         "deletions", "qual_sum", "qual_bases", "bases_beyond_cycle", "pairs_in_is", "reads_no_acgt")
T = {name: k for k, name in enumerate(NAMES)}
assert len(NAMES) == N_TALLIES

LETTER = np.full(16, 4, np.int64)                                      # A C G T other
LETTER[[1, 2, 4, 8]] = [0, 1, 2, 3]
COLUMN = np.full(16, -1, np.int64)                                     # of MC: = X M I S (D is 5)
COLUMN[[7, 8, 0, 1, 4]] = [0, 1, 2, 3, 4]


class Refused(Exception):
    pass


def rows(table, max_cycle, max_insert):
    return dict(MAPQ=256, RL=max_cycle + 1, IS=max_insert + 1, GC=101, ID=256, BC=max_cycle, QC=max_cycle, MC=max_cycle)[table]


def fields(r):
    """(refID, pos, l_name, mapq, n_cigar, flag, l_seq, next_refID, next_pos, tlen) of a record."""
    ref, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHIiii", r, 4)
    return ref, pos, l_name, mapq, n_cigar, flag, l_seq, next_ref, next_pos, tlen


def check(records):
    """What bmq_add refuses of the records themselves."""
    for k, r in enumerate(records):
        if len(r) < 36 or struct.unpack_from("<I", r, 0)[0] != len(r) - 4:
            raise Refused(f"record {k}: its block_size")
        _, _, l_name, _, n_cigar, _, l_seq, _, _, _ = fields(r)
        if 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq > len(r):
            raise Refused(f"record {k}: its fields lie beyond its end")
        ops = np.frombuffer(r, "<u4", n_cigar, 36 + l_name)
        if (ops & 15 > 8).any():
            raise Refused(f"record {k}: an op code above 8")
        query = int((ops >> 4)[COLUMN[ops & 15] >= 0].sum())
        if n_cigar and l_seq and query != l_seq:
            raise Refused(f"record {k}: {query} query bases, l_seq {l_seq}")


def run(records, skip=None, max_cycle=1024, max_insert=8000):
    """(tallies, tables): a list of 35 ints and a dict of int64 arrays (rows, width)."""
    C, I = max_cycle, max_insert
    if not 1 <= C <= 65535 or not 1 <= I <= 65535:
        raise Refused("max_cycle and max_insert are 1 .. 65535")
    check(records)
    t = [0] * N_TALLIES
    tab = {name: np.zeros((rows(name, C, I), WIDTH[name]), np.int64) for name in TABLES}
    for k, r in enumerate(records):
        if skip is not None and skip[k]:
            continue
        ref, _, l_name, mapq, n_cigar, flag, l_seq, next_ref, _, tlen = fields(r)
        at_cigar = 36 + l_name
        at_seq = at_cigar + 4 * n_cigar
        ops = np.frombuffer(r, "<u4", n_cigar, at_cigar).astype(np.int64)
        op, length = ops & 15, ops >> 4
        primary, mapped, reverse = not flag & 0x900, not flag & 4, bool(flag & 0x10)
        paired = primary and bool(flag & 1)
        placeholder = n_cigar == 2 and int(ops[0]) == (l_seq << 4 | 4) & 0xFFFFFFFF and int(op[1]) == 3
        aligned = mapped and n_cigar > 0 and l_seq > 0 and not placeholder
        both = paired and mapped and not flag & 8
        other_ref = both and next_ref != ref
        for name, yes in (("records", True), ("primary", primary), ("secondary", flag & 0x100), ("supplementary", flag & 0x800), ("duplicates", flag & 0x400),
                          ("qc_failed", flag & 0x200), ("mapped", mapped), ("primary_mapped", primary and mapped), ("paired", paired),
                          ("read1", paired and flag & 0x40), ("read2", paired and flag & 0x80), ("properly_paired", paired and flag & 2 and mapped),
                          ("both_mapped", both), ("singletons", paired and mapped and flag & 8), ("mate_other_ref", other_ref),
                          ("mate_other_ref_mapq5", other_ref and mapq >= 5), ("reverse_strand", mapped and reverse), ("mapq0", mapped and mapq == 0),
                          ("aligned_records", aligned), ("left_out", mapped and placeholder)):
            t[T[name]] += 1 if yes else 0
        if primary:
            t[T["bases"]] += l_seq
            tab["RL"][min(l_seq, C), 0] += 1
        if primary and mapped:
            t[T["bases_mapped"]] += l_seq
        if mapped:
            tab["MAPQ"][mapq, 0] += 1
        if both and next_ref == ref and tlen > 0:
            way = flag & 0x30
            tab["IS"][min(tlen, I), 0 if way == 0x20 else 1 if way == 0x10 else 2] += 1
            t[T["pairs_in_is"]] += 1
        cycle = np.arange(l_seq, dtype=np.int64)
        if reverse:
            cycle = l_seq - 1 - cycle
        inside = cycle < C
        if primary and l_seq > 0:
            packed = np.frombuffer(r, np.uint8, (l_seq + 1) // 2, at_seq)
            codes = np.empty(2 * packed.size, np.int64)
            codes[0::2], codes[1::2] = packed >> 4, packed & 15
            letter = LETTER[codes[:l_seq]]
            qual = np.frombuffer(r, np.uint8, l_seq, at_seq + (l_seq + 1) // 2).astype(np.int64)
            n, g = int((letter < 4).sum()), int(((letter == 1) | (letter == 2)).sum())
            sequenced = np.where(reverse & (letter < 4), 3 - letter, letter)
            np.add.at(tab["BC"], (cycle[inside], sequenced[inside]), 1)
            t[T["bases_beyond_cycle"]] += int((~inside).sum())
            has = qual != 0xFF
            t[T["qual_sum"]] += int(qual[has].sum())
            t[T["qual_bases"]] += int(has.sum())
            np.add.at(tab["QC"], (cycle[has & inside], np.minimum(qual[has & inside], 63)), 1)
            if n == 0:
                t[T["reads_no_acgt"]] += 1
            else:
                tab["GC"][(200 * g + n) // (2 * n), 0] += 1
        if aligned:
            column = COLUMN[op]
            span = np.where(column >= 0, length, 0)
            start = np.cumsum(span) - span               # the query cursor when the op is met
            of_base = np.repeat(column, span)            # l_seq of them: check() has seen to it
            np.add.at(tab["MC"], (cycle[inside], of_base[inside]), 1)
            for name, code in (("bases_m", 0), ("bases_eq", 7), ("bases_x", 8), ("inserted_bases", 1), ("deleted_bases", 2), ("soft_clipped_bases", 4)):
                t[T[name]] += int(length[op == code].sum())
            t[T["insertions"]] += int(((op == 1) & (length > 0)).sum())
            t[T["deletions"]] += int(((op == 2) & (length > 0)).sum())
            indel = ((op == 1) | (op == 2)) & (length > 0)
            np.add.at(tab["ID"], (np.minimum(length[indel], 255), (op[indel] == 2).astype(np.int64)), 1)
            before = start[(op == 2) & (length > 0) & (start > 0)] - 1
            at = cycle[before]
            np.add.at(tab["MC"], (at[at < C], 5), 1)
    return t, tab


def derived(t, tab, max_insert):
    """The four derived SN values, None where the divisor is 0."""
    inward = tab["IS"][:max_insert, 0]
    total, median = int(inward.sum()), None
    if total:
        median = int(np.argmax(2 * np.cumsum(inward) >= total))
    div = lambda a, b: a // b if b else None
    return [("error_rate_ppm", div(t[T["bases_x"]] * 10 ** 6, t[T["bases_eq"]] + t[T["bases_x"]])),
            ("mean_quality_centi", div(t[T["qual_sum"]] * 100, t[T["qual_bases"]])),
            ("mean_length_centi", div(t[T["bases"]] * 100, t[T["primary"]])),
            ("insert_size_median", median)]


def text(t, tab, max_insert):
    """The file of --stats."""
    out = ["# bucketmap --stats 1"]
    out += [f"SN\t{name}\t{int(v)}" for name, v in zip(NAMES, t)]
    out += [f"SN\t{name}\t{'.' if v is None else v}" for name, v in derived(t, tab, max_insert)]
    for section, table, head in (("MAPQ", "MAPQ", "mapq\trecords"), ("RL", "RL", "length\trecords"), ("GCF", "GC", "gc_percent\trecords"),
                                 ("ID", "ID", "length\tinsertions\tdeletions"), ("IS", "IS", "insert_size\tinward\toutward\tother")):
        out.append(f"# {section}\t{head}")
        cells = tab[table]
        out += ["\t".join([section, str(r), *[str(int(x)) for x in cells[r]]]) for r in np.flatnonzero(cells.any(axis=1)).tolist()]
    top = int(np.flatnonzero(tab["QC"].any(axis=0)).max()) + 1 if tab["QC"].any() else 0
    for section, table, head, shown in (("BCC", "BC", ["A", "C", "G", "T", "other"], 5), ("QCC", "QC", [f"q{q}" for q in range(top)], top),
                                        ("MCC", "MC", ["=", "X", "M", "I", "S", "D"], 6)):
        out.append("\t".join([f"# {section}", "cycle", *head]))
        cells = tab[table]
        last = int(np.flatnonzero(cells.any(axis=1)).max()) + 1 if cells.any() else 0
        out += ["\t".join([section, str(r + 1), *[str(int(x)) for x in cells[r, :shown]]]) for r in range(last)]
    return "\n".join(out) + "\n"


def summary_line(t):
    return (f"Stats: {t[T['records']]} records ({t[T['mapped']]} mapped, {t[T['properly_paired']]} properly paired, {t[T['duplicates']]} duplicates), "
            f"{t[T['bases']]} bases, {t[T['bases_x']]} of {t[T['bases_eq']] + t[T['bases_x']]} =/X bases mismatch")
