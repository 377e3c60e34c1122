"""The duplicate-marking rule of include/bmd.h in plain Python (dicts and sorted), over a list of BAM record bytes.

ends(records) -> (end, score, kind) lists; mark(end, score, kind) -> (dup list, counts); marked(records) -> the records with
0x400 ORed into the duplicates' flags; passes(end, score, kind) -> the radix passes the device's five sorts have to run."""
import struct

CLIP = (4, 5)
REF = (0, 2, 3, 7, 8)


def fields(rec):
    ref, pos, l_name = struct.unpack_from("<iiB", rec, 4)
    n_cigar, flag, l_seq = struct.unpack_from("<HHI", rec, 16)
    at = 36 + l_name
    cigar = struct.unpack_from(f"<{n_cigar}I", rec, at)
    at += 4 * n_cigar + (l_seq + 1) // 2
    assert at + l_seq <= len(rec)
    return ref, pos, flag, l_seq, rec[36: 36 + l_name], cigar, rec[at: at + l_seq]


def describe(rec):
    """(eligible, E, score) of one record."""
    ref, pos, flag, l_seq, _, cigar, qual = fields(rec)
    score = sum(q for q in qual if 15 <= q != 0xFF)
    ops = [(c & 15, c >> 4) for c in cigar]
    reflen = sum(n for op, n in ops if op in REF)
    lead = trail = 0
    for op, n in ops:
        if op not in CLIP:
            break
        lead += n
    for op, n in reversed(ops):
        if op not in CLIP:
            break
        trail += n
    reverse = bool(flag & 0x10)
    end5 = pos + reflen + trail - 1 if reverse else pos - lead
    placeholder = len(ops) == 2 and ops[0] == (4, l_seq) and ops[1][0] == 3
    ok = not flag & (0x4 | 0x100 | 0x800) and ref >= 0 and not placeholder and -2 ** 31 <= end5 < 2 ** 31
    return ok, (ref << 33 | (end5 + 2 ** 31) << 1 | int(reverse)) if ok else 0, score


def are_mates(a, b):
    fa, fb = struct.unpack_from("<H", a, 18)[0], struct.unpack_from("<H", b, 18)[0]
    if not (fa & 1 and fb & 1) or (fa | fb) & (0x100 | 0x800):
        return False
    if not (fa & 0x40 and not fa & 0x80 and fb & 0x80 and not fb & 0x40):
        return False
    return a[12] == b[12] and a[36: 36 + a[12]] == b[36: 36 + b[12]]


def ends(records):
    d = [describe(r) for r in records]
    n = len(records)
    kind = [1 if d[i][0] else 0 for i in range(n)]
    for i in range(n - 1):
        if d[i][0] and d[i + 1][0] and are_mates(records[i], records[i + 1]):
            kind[i], kind[i + 1] = 2, 3
    return [x[1] for x in d], [x[2] for x in d], kind


def mark(end, score, kind):
    n = len(kind)
    dup = [0] * n
    pairs = [i for i in range(n) if kind[i] == 2]
    frags = [i for i in range(n) if kind[i] == 1]
    best = {}                                            # pair key -> (the negated score, i) of the kept unit
    for i in pairs:
        key = (min(end[i], end[i + 1]), max(end[i], end[i + 1]))
        best[key] = min(best.get(key, (0, n)), (-(score[i] + score[i + 1]), i))
    for i in pairs:
        key = (min(end[i], end[i + 1]), max(end[i], end[i + 1]))
        if best[key][1] != i:
            dup[i] = dup[i + 1] = 1
    pair_ends = {end[i + k] for i in pairs for k in (0, 1)}
    best = {}
    for i in frags:
        best[end[i]] = min(best.get(end[i], (0, n)), (-score[i], i))
    for i in frags:
        if end[i] in pair_ends or best[end[i]][1] != i:
            dup[i] = 1
    counts = [len(pairs), len(frags), sum(dup[i] + dup[i + 1] for i in pairs), sum(dup[i] for i in frags)]
    return dup, counts


def marked(records):
    """(the records with the flags set, dup, counts)"""
    dup, counts = mark(*ends(records))
    out = []
    for r, d in zip(records, dup):
        if d:
            r = bytearray(r)
            r[19] |= 4
            r = bytes(r)
        out.append(r)
    return out, dup, counts


def _digits_that_differ(keys):
    return sum(1 for d in range(8) if len({(k >> (8 * d)) & 255 for k in keys}) > 1)


def passes(end, score, kind):
    """The passes of the five stable sorts of include/bmd.h's marking: a digit on which all keys of a sort agree costs none."""
    inv = lambda v: ~v & (2 ** 64 - 1)
    pairs = [i for i in range(len(kind)) if kind[i] == 2]
    frags = [i for i in range(len(kind)) if kind[i] == 1]
    total = 0
    if pairs:
        total += _digits_that_differ([inv(score[i] + score[i + 1]) for i in pairs])
        total += _digits_that_differ([min(end[i], end[i + 1]) for i in pairs])
        total += _digits_that_differ([max(end[i], end[i + 1]) for i in pairs])
    if frags:
        total += _digits_that_differ([0] * (2 * len(pairs)) + [inv(score[i]) for i in frags])
        total += _digits_that_differ([end[i + k] for i in pairs for k in (0, 1)] + [end[i] for i in frags])
    return total
