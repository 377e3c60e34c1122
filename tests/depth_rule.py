"""The coverage rule of include/bmc.h in plain Python (dicts and numpy arrays), over a list of BAM record bytes.

count(records, ref_len, skip=None) -> Result with .depth (one uint32 array per reference), .runs ([(r, start, end, depth)]) and
.stats ([[n_reads, cov_bases, sum_depth, sum_mapq, sum_qual, n_qual, n_long]] per reference).  refused(records, n_ref) names what
bmc_add refuses of the records (None: nothing).  depth_text / coverage_text are the files of --depth / --coverage."""
import struct

import numpy as np

BLOCK = (0, 7, 8)
REF = (0, 2, 3, 7, 8)
QUERY = (0, 1, 4, 7, 8)
SKIP_FLAGS = 0x4 | 0x100 | 0x200 | 0x400


def fields(rec):
    ref, pos, l_name, mapq = struct.unpack_from("<iiBB", rec, 4)
    n_cigar, flag, l_seq = struct.unpack_from("<HHI", rec, 16)
    at = 36 + l_name
    cigar = struct.unpack_from(f"<{n_cigar}I", rec, at)
    at += 4 * n_cigar + (l_seq + 1) // 2
    assert at + l_seq <= len(rec)
    return ref, pos, mapq, flag, l_seq, cigar, rec[at: at + l_seq]


def refused(records, n_ref):
    for i, rec in enumerate(records):
        ref, pos, mapq, flag, l_seq, cigar, qual = fields(rec)
        if any(c & 15 > 8 for c in cigar):
            return f"record {i}: op code"
        if cigar and l_seq and sum(c >> 4 for c in cigar if c & 15 in QUERY) != l_seq:
            return f"record {i}: query length"
        if ref >= n_ref and not flag & 4:
            return f"record {i}: reference"
    return None


class Result:
    def __init__(self, depth, runs, stats):
        self.depth, self.runs, self.stats = depth, runs, stats


def count(records, ref_len, skip=None):
    n_ref = len(ref_len)
    assert n_ref > 0 and all(l > 0 for l in ref_len) and refused(records, n_ref) is None
    diff = [{} for _ in range(n_ref)]                     # position -> the sum of the +1 and -1 there
    stats = [[0] * 7 for _ in range(n_ref)]
    for i, rec in enumerate(records):
        ref, pos, mapq, flag, l_seq, cigar, qual = fields(rec)
        if flag & SKIP_FLAGS or (skip is not None and skip[i]):
            continue
        if not (0 <= ref < n_ref and 0 <= pos < ref_len[ref]) or not cigar:
            continue
        st = stats[ref]
        if len(cigar) == 2 and cigar[0] == (l_seq << 4 | 4) and cigar[1] & 15 == 3:
            st[6] += 1
            continue
        st[0] += 1
        st[3] += mapq
        rc, qc = pos, 0
        for c in cigar:
            op, n = c & 15, c >> 4
            if op in BLOCK:
                s, e = rc, min(rc + n, ref_len[ref])
                if s < e:
                    diff[ref][s] = diff[ref].get(s, 0) + 1
                    diff[ref][e] = diff[ref].get(e, 0) - 1
                    if l_seq:
                        q = [x for x in qual[qc: qc + e - s] if x != 0xFF]
                        st[4] += sum(q)
                        st[5] += len(q)
            if op in REF:
                rc += n
            if op in QUERY:
                qc += n
    depth, runs = [], []
    for r in range(n_ref):
        d = np.zeros(ref_len[r] + 1, np.int64)
        for p, v in diff[r].items():
            d[p] += v
        d = np.cumsum(d)
        assert d[-1] == 0 and d.min() >= 0
        d = d[:-1]
        depth.append(d.astype(np.uint32))
        stats[r][1] = int(np.count_nonzero(d))
        stats[r][2] = int(d.sum())
        # the places where the depth differs from the place before (the place before the first has depth 0)
        edge = np.flatnonzero(np.diff(np.concatenate(([0], d, [0])))).tolist()
        for a, b in zip(edge, edge[1:]):
            if d[a] > 0:
                runs.append((r, a, b, int(d[a])))
    return Result(depth, runs, stats)


def depth_text(res, names):
    return "".join(f"{names[r]}\t{s}\t{e}\t{d}\n" for r, s, e, d in res.runs)


def coverage_text(res, names, ref_len):
    out = "#rname\tstartpos\tendpos\tnumreads\tcovbases\tcoverage\tmeandepth\tmeanbaseq\tmeanmapq\n"
    ratio = lambda a, b: a / b if b else 0.0
    for r, name in enumerate(names):
        n_reads, cov, total, mapq, qual, n_qual, _ = res.stats[r]
        out += "%s\t1\t%d\t%d\t%d\t%.4f\t%.4f\t%.4f\t%.4f\n" % (name, ref_len[r], n_reads, cov, ratio(100.0 * cov, ref_len[r]),
                                                               ratio(float(total), ref_len[r]), ratio(float(qual), n_qual),
                                                               ratio(float(mapq), n_reads))
    return out
