"""bmv_overlap's rule (include/bmv.h) in plain Python, column by column, on top of test_annotate.restate's forward-strand
columns and test_clip's range finder: the yardstick tests/test_overlap.py pins on hand-worked cases and the GPU tests and the
host restatement (host/overlap_clip.h) are compared with.  Nothing here is clever: every column carries its op and its g."""
from test_annotate import D, EQ, I, X, restate
from test_clip import S, _md, range_scan

NO_MATE = 2 ** 32 - 1


def columns(window, rc, query, begin, cigar):
    """(bmv_annotate's pos, the forward-strand columns as ops, the reference letters under the X and D columns)."""
    pos, _, xc, _, ref, _ = restate(window, rc, query, begin, cigar)
    return pos, [op for op, n in xc for _ in range(n)], ref


def base_range(cols, match, penalty):
    """(l, r): all columns without scores, else bmv_clip's range."""
    if match == 0 and penalty == 0:
        return 0, len(cols)
    _, l, r = range_scan([match if op == EQ else -penalty for op in cols])
    return l, r


def record(pos, cols, ref, l, r, qlen, match, penalty):
    """bmv_clipped's layout for the kept range [l, r) of one alignment."""
    none = dict(score=0, clip_left=0, clip_right=0, pos=0, ref_len=0, nm=0, xcigar=[], ref_bases=b"", md="0")
    if not cols:
        return none
    if l == r:
        return dict(none, clip_right=qlen, xcigar=[(S, qlen)] if qlen else [])
    before, kept, after = cols[:l], cols[l:r], cols[r:]
    left, right = sum(1 for op in before if op != D), sum(1 for op in after if op != D)
    ref_at = sum(1 for op in before if op in (X, D))
    k_ref = ref[ref_at: ref_at + sum(1 for op in kept if op in (X, D))]
    runs = []
    for op in kept:
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    runs = [tuple(e) for e in runs]
    assert left + sum(1 for op in kept if op != D) + right == qlen
    n_eq = sum(1 for op in kept if op == EQ)
    return dict(score=match * n_eq - penalty * (len(kept) - n_eq), clip_left=left, clip_right=right,
                pos=pos + sum(1 for op in before if op != I), ref_len=sum(1 for op in kept if op != I), nm=len(kept) - n_eq,
                xcigar=([(S, left)] if left else []) + runs + ([(S, right)] if right else []), ref_bases=k_ref, md=_md(runs, k_ref))


def positions(cols, at):
    """g per column and, last, behind the last one: the reference position of column i, or of the next one that has one."""
    gs = []
    for op in cols:
        gs.append(at)
        at += op != I
    return gs + [at]


def cut(cols, g, rng, mate, contig=None):
    """The rule on columns: cols[a] the ops of alignment a's forward-strand columns, g[a] = positions(cols[a], ...), rng[a]
    its base range (l, r).  Returns (final ranges, cut per alignment, role per alignment, m per alignment, pairs cut)."""
    n = len(cols)
    final, clipped = list(rng), [0] * n
    role, cut_at = [None] * n, [None] * n
    pairs_cut = 0
    for a in range(n):
        b = mate[a]
        if b == NO_MATE or b < a:
            continue
        assert mate[b] == a and b != a
        (la, ra), (lb, rb) = rng[a], rng[b]
        if la == ra or lb == rb or (contig is not None and contig[a] != contig[b]):
            continue
        first, second = (a, b) if (g[a][la], a) < (g[b][lb], b) else (b, a)
        (lf, rf), (ls, rs) = rng[first], rng[second]
        if g[first][rf] > g[second][rs]:
            continue                                             # containment
        o = g[first][rf] - g[second][ls]
        if o <= 0:
            continue
        m = g[second][ls] + o // 2
        keep_f = [i for i in range(lf, rf) if cols[first][i] in (EQ, X) and g[first][i] < m]
        keep_s = [i for i in range(ls, rs) if cols[second][i] in (EQ, X) and g[second][i] >= m]
        if not keep_f or not keep_s:
            continue
        r2, l2 = keep_f[-1] + 1, keep_s[0]
        final[first], final[second] = (lf, r2), (l2, rs)
        clipped[first] = sum(1 for op in cols[first][r2:rf] if op != D)
        clipped[second] = sum(1 for op in cols[second][ls:l2] if op != D)
        role[first], role[second] = "first", "second"
        cut_at[first] = cut_at[second] = m
        pairs_cut += 1
    return final, clipped, role, cut_at, pairs_cut


def overlap(alns, mate, contig=None, match=1, penalty=2):
    """alns: per alignment (window, rc, query, begin, cigar, text_start); mate: per alignment the mate's index or NO_MATE;
    contig: per alignment, or None.  Returns (records, info): per alignment bmv_clipped's record plus `cut`; info holds
    pairs_cut, bases_cut and per alignment l, r, G0, G1, role ('first', 'second' or None) and m."""
    n = len(alns)
    pos, cols, ref, rng, g = [], [], [], [], []
    for window, rc, query, begin, cigar, text_start in alns:
        p, c, rf = columns(window, rc, query, begin, cigar)
        pos.append(p)
        cols.append(c)
        ref.append(rf)
        rng.append(base_range(c, match, penalty))
        g.append(positions(c, text_start + p))
    final, clipped, role, cut_at, pairs_cut = cut(cols, g, rng, mate, contig)
    recs = []
    for a in range(n):
        rec = record(pos[a], cols[a], ref[a], *final[a], len(alns[a][2]), match, penalty)
        rec["cut"] = clipped[a]
        recs.append(rec)
    info = dict(pairs_cut=pairs_cut, bases_cut=sum(clipped), l=[x[0] for x in rng], r=[x[1] for x in rng],
                G0=[g[a][rng[a][0]] if cols[a] else 0 for a in range(n)], G1=[g[a][rng[a][1]] if cols[a] else 0 for a in range(n)],
                role=role, m=cut_at)
    return recs, info
