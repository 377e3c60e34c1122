"""ctypes binding of the MI355X alignment verifier (bmv_* in libbmf.so, C ABI in include/bmv.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _bmf_lib

BMV_OK = 0
REJECTED = -(2 ** 31)     # BMV_REJECTED: the score of an alignment beyond its edit bound (align_bounded)
BEYOND = 2 ** 32 - 1      # BMV_BEYOND: no winner (an empty group) / edits beyond best + margin (align_best)
PAIR_NONE = 2 ** 64 - 1   # BMV_PAIR_NONE: no proper combination (s1) / none at another locus (s2)
SPLIT_NONE = -(2 ** 63)   # BMV_SPLIT_NONE: a chosen segment without a competitor (s2)
SPLIT_MAX_SEGMENTS = 16   # BMV_SPLIT_MAX_SEGMENTS
NO_MATE = 2 ** 32 - 1     # BMV_NO_MATE: an alignment without a mate in the batch (overlap)


class BmvError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"bmv error {code}: {msg}")
        self.code = code


class _Params(C.Structure):
    _fields_ = [("max_query_len", C.c_uint32), ("max_text_len", C.c_uint32), ("device", C.c_int32)]


_u8p, _u32p, _u64p, _i32p, _i64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32, C.c_int64))

SYMBOLS = {
    "bmv_last_error": (C.c_char_p, []),
    "bmv_create": (C.c_int, [C.POINTER(_Params), C.POINTER(C.c_void_p)]),
    "bmv_destroy": (None, [C.c_void_p]),
    "bmv_load_genome": (C.c_int, [C.c_void_p, _u8p, C.c_uint64]),
    "bmv_load_genome_records": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_uint32]),
    "bmv_align": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, C.c_uint32, _u64p]),
    "bmv_align_long": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, C.c_uint32, _u64p]),
    "bmv_align_bounded": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, _u32p, C.c_uint32, _u64p]),
    "bmv_last_bounded_stats": (C.c_int, [C.c_void_p, _u32p, _u64p, C.POINTER(C.c_float)]),
    "bmv_align_best": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, C.c_uint32, _u32p, C.c_uint32,
                                 _u32p, _u32p, _u64p]),
    "bmv_best": (C.c_int, [C.c_void_p, _u32p, _u32p, _u32p]),
    "bmv_last_best_stats": (C.c_int, [C.c_void_p, _u32p, _u32p, _u32p, _u32p, _u32p, _u64p, C.POINTER(C.c_float),
                                      C.POINTER(C.c_float)]),
    "bmv_pair": (C.c_int, [C.c_void_p, _u64p, _u32p, _u8p, _u32p, _u32p, _u32p, _u32p, C.c_uint32, _u32p, C.c_uint32, C.c_uint32,
                           C.c_uint32]),
    "bmv_pairs": (C.c_int, [C.c_void_p, _u32p, _u8p, _u64p, _u64p, _u32p]),
    "bmv_last_pair_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p]),
    "bmv_align_paired": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, C.c_uint32, _u32p, C.c_uint32,
                                   _u32p, _u32p, _u32p, C.c_uint32, C.c_uint32, _u64p]),
    "bmv_frag_spans": (C.c_int, [C.c_void_p, _u64p, _u32p, _u8p, _u32p, _u32p, _u32p, _u32p, C.c_uint32, _u32p, C.c_uint32, C.c_uint32]),
    "bmv_frag": (C.c_int, [C.c_void_p, _u32p, _u64p]),
    "bmv_last_frag_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u32p]),
    "bmv_paired_begin": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, C.c_uint32, _u32p, C.c_uint32,
                                   _u32p, _u32p, _u32p, C.c_uint32]),
    "bmv_paired_finish": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _u64p]),
    "bmv_rescue": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u32p, _u32p, _u64p, _u64p, _u64p, _u32p, _u32p,
                             C.c_uint32, C.c_uint32, C.c_uint32]),
    "bmv_rescued": (C.c_int, [C.c_void_p, _u64p, _u32p, _u8p, _u32p, _u32p, _u8p]),
    "bmv_last_rescue_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p, _u32p]),
    "bmv_results": (C.c_int, [C.c_void_p, _i32p, _u32p, _u64p, _u32p]),
    "bmv_last_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p]),
    "bmv_annotate": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, _u32p, _u64p, _u32p, C.c_uint32,
                               _u64p, _u64p]),
    "bmv_annotations": (C.c_int, [C.c_void_p, _u32p, _u32p, _u32p, _u64p, _u32p, _u64p, _u8p]),
    "bmv_last_annotate_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p]),
    "bmv_clip": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, _u32p, _u64p, _u32p, C.c_uint32,
                           C.c_uint32, C.c_uint32, _u64p, _u64p]),
    "bmv_clipped": (C.c_int, [C.c_void_p, _i64p, _u32p, _u32p, _u32p, _u32p, _u32p, _u64p, _u32p, _u64p, _u8p]),
    "bmv_last_clip_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p]),
    "bmv_overlap": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, _u32p, _u64p, _u32p, _u32p, _u32p,
                              C.c_uint32, C.c_uint32, C.c_uint32, _u64p, _u64p]),
    "bmv_overlapped": (C.c_int, [C.c_void_p, _i64p, _u32p, _u32p, _u32p, _u32p, _u32p, _u64p, _u32p, _u64p, _u8p, _u32p]),
    "bmv_last_overlap_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p, _u64p, _u64p]),
    "bmv_realign": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, _u32p, _u64p, _u32p, C.c_uint32,
                              C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u64p]),
    "bmv_realigned": (C.c_int, [C.c_void_p, _i32p, _u32p, _u8p, _u64p, _u32p]),
    "bmv_last_realign_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p, _u32p]),
    "bmv_leftalign": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, _u32p, _u64p, _u32p, C.c_uint32, _u64p]),
    "bmv_leftaligned": (C.c_int, [C.c_void_p, _u32p, _u64p, _u32p, _u8p, _u32p]),
    "bmv_last_leftalign_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), _u64p, _u32p, _u64p, _u64p]),
    "bmv_split": (C.c_int, [C.c_void_p, _u8p, C.c_uint64, _u64p, _u32p, _u8p, _u64p, _u32p, _u32p, _u64p, _u32p, _u32p, C.c_uint32,
                            _u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "bmv_split_pick": (C.c_int, [C.c_void_p, _i64p, _u32p, _u32p, _i64p, _i64p, _u8p, _u32p, C.c_uint32, _u32p, C.c_uint32,
                                 C.c_uint32, C.c_uint32, C.c_uint32]),
    "bmv_segments": (C.c_int, [C.c_void_p, _i64p, _u32p, _u32p, _i64p, _i64p, _u32p, _u32p, _i64p]),
    "bmv_last_split_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), _u64p, _u64p]),
}
_ready = False


def lib() -> C.CDLL:
    global _ready
    L = _bmf_lib()
    if not _ready:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _ready = True
    return L


def _check(rc: int) -> None:
    if rc != BMV_OK:
        raise BmvError(rc, lib().bmv_last_error().decode(errors="replace"))


def _p(a, ty):
    return a.ctypes.data_as(ty)


def cigar_string(packed) -> str:
    return "".join(f"{int(e) >> 4}{'MID'[int(e) & 15]}" for e in packed)


def xcigar_string(packed) -> str:
    """Annotated entries (Verifier.annotate, Verifier.clip) as SAM text: BAM op codes, so M I D S = X all print."""
    return "".join(f"{int(e) >> 4}{'MIDNSHP=X'[int(e) & 15]}" for e in packed)


def md_string(xcigar, ref_bases) -> str:
    """SAM's MD tag of one alignment from its annotated entries and the reference bases under its X and D columns, as
    samtools writes it: a running count of matches; before every X base and before every D entry the count (also 0), then
    the base -- or '^' and the entry's bases --, and the count starts again; I adds nothing and neither does S
    (Verifier.clip's soft clips); the count once more at the end.  The rule of host/sam_tags.h, for users of the ABI."""
    ref = bytes(bytearray(ref_bases)).decode("ascii")
    out, run, at = [], 0, 0
    for e in xcigar:
        op, n = int(e) & 15, int(e) >> 4
        if op == 7:
            run += n
        elif op == 8:
            for x in range(n):
                out.append(f"{run}{ref[at + x]}")
                run = 0
            at += n
        elif op == 2:
            out.append(f"{run}^{ref[at: at + n]}")
            run = 0
            at += n
    if at != len(ref):
        raise ValueError(f"the entries cover {at} reference bases under X and D, {len(ref)} were given")
    return "".join(out) + str(run)


_DNA4_RANK = bytes(1 if chr(b).upper() in "CYSB" else 2 if chr(b).upper() in "GK" else 3 if chr(b).upper() in "TU" else 0
                   for b in range(256))


def left_align(window, query, text_rc, begin, cigar) -> dict:
    """bmv_leftalign's rule (include/bmv.h) for ONE alignment, in plain Python, for users of the ABI: `window` the text
    window as it lies in the genome, `query` the read as sequenced, `begin` and the packed M/I/D `cigar` as the aligner
    gave them.  Returns begin and cigar (a list) in the aligner's orientation, changed, dropped, and the compared columns
    and merges the stats count.  The rule of host/left_align.h."""
    W = bytes(window).translate(_DNA4_RANK)
    Q = bytes(query).translate(_DNA4_RANK)
    entries = [int(e) for e in cigar]
    if not entries:
        return {"begin": int(begin), "cigar": [], "changed": 0, "dropped": 0, "compared": 0, "merges": 0}
    for op in range(3):
        if sum(e >> 4 for e in entries if e & 15 == op) >= 1 << 28:
            raise ValueError(f"the {'MID'[op]} entries sum to 2^28 columns or more: a merged entry would not fit 28 bits")
    rc = bool(text_rc)
    if rc:
        Q = Q[::-1]
        entries = entries[::-1]
    ref_len = sum(e >> 4 for e in entries if e & 15 != 1)
    pos = len(W) - int(begin) - ref_len if rc else int(begin)
    p, q, dropped, compared, merges, moved = pos, 0, 0, 0, 0, False
    stack = []

    def append_m(n):
        if n == 0:
            return
        if stack and stack[-1] & 15 == 0:
            stack[-1] += n << 4
        else:
            stack.append(n << 4)

    for e in entries:
        op, L = e & 15, e >> 4
        if op == 0:
            append_m(L)
            p += L
            q += L
            continue
        p_after, q_after = p + (L if op == 2 else 0), q + (L if op == 1 else 0)
        pend, keep = 0, True
        while True:
            if not stack:
                if op == 2:
                    pos += L
                    dropped += L
                    keep = False
                break
            top_op, k = stack[-1] & 15, stack[-1] >> 4
            if top_op == 0:
                s = 0
                while s < k:
                    compared += 1
                    t = s + 1
                    if (W[p - t] != W[p - t + L]) if op == 2 else (Q[q - t] != Q[q - t + L]):
                        break
                    s += 1
                p, q, pend = p - s, q - s, pend + s
                if s < k:
                    stack[-1] = (k - s) << 4
                    break
                stack.pop()
            elif top_op == op:
                stack.pop()
                L += k
                if op == 2:
                    p -= k
                else:
                    q -= k
                merges += 1
            else:
                break
        if keep:
            stack.append(L << 4 | op)
        append_m(pend)
        moved = moved or pend != 0
        p, q = p_after, q_after
    if stack and stack[-1] & 15 == 2:
        dropped += stack.pop() >> 4
    return {"begin": len(W) - pos - (ref_len - dropped) if rc else pos, "cigar": stack[::-1] if rc else stack,
            "changed": int(moved or dropped != 0), "dropped": dropped, "compared": compared, "merges": merges}


def clip_range(window, query, text_rc, begin, cigar, match=1, penalty=2) -> dict:
    """bmv_clip's range rule (include/bmv.h) for ONE alignment, in plain Python, for users of the ABI: `window` the text
    window as it lies in the genome, `query` the read as sequenced, `begin` and the packed M/I/D `cigar` as the aligner gave
    them.  The columns are taken in forward-strand order; an = column weighs +match, an X, I or D column -penalty; the kept
    range [l, r) has the greatest sum, among equals the smallest r, then the largest l.  Returns score, clip_left, clip_right,
    pos and ref_len as bmv_clip reports them, l and r, and what bmv_split derives per alignment: q_lo and q_hi (the kept query
    interval in READ orientation), g_off_lo = pos and g_off_hi = pos + ref_len (add text_start for g_lo and g_hi)."""
    w, q = bytes(bytearray(window)), bytes(bytearray(query))
    m, rc = len(q), bool(text_rc)
    ents = [(int(e) & 15, int(e) >> 4) for e in cigar]
    if not ents:
        return {"score": 0, "clip_left": 0, "clip_right": 0, "pos": 0, "ref_len": 0, "l": 0, "r": 0, "q_lo": 0, "q_hi": m,
                "g_off_lo": 0, "g_off_hi": 0}
    ref_all = sum(n for op, n in ents if op != 1)
    ti, qi = (len(w) - int(begin) - ref_all) if rc else int(begin), 0
    if rc:
        ents.reverse()
    p, col = 0, 0
    low, low_at = 0, (0, ti, qi)                # the least prefix sum so far, at its latest border: (column, ti, qi)
    best, best_l, best_r = 0, (0, ti, qi), (0, ti, qi)
    for op, n in ents:
        for _ in range(n):
            if op == 0:
                tr = _DNA4_RANK[w[ti]]
                qr = (_DNA4_RANK[q[m - 1 - qi]] ^ 3) if rc else _DNA4_RANK[q[qi]]
                p += match if tr == qr else -penalty
                ti, qi = ti + 1, qi + 1
            elif op == 1:
                p -= penalty
                qi += 1
            else:
                p -= penalty
                ti += 1
            col += 1
            here = (col, ti, qi)
            if p - low > best:                  # (strictly: the smallest r; `low` sits at its latest border: the largest l)
                best, best_l, best_r = p - low, low_at, here
            if p <= low:
                low, low_at = p, here
    if best == 0:
        cl, cr, pos, ref_len, l, r = 0, m, 0, 0, 0, 0
    else:
        cl, cr, pos, ref_len, l, r = best_l[2], m - best_r[2], best_l[1], best_r[1] - best_l[1], best_l[0], best_r[0]
    return {"score": best, "clip_left": cl, "clip_right": cr, "pos": pos, "ref_len": ref_len, "l": l, "r": r,
            "q_lo": cr if rc else cl, "q_hi": m - (cl if rc else cr), "g_off_lo": pos, "g_off_hi": pos + ref_len}


def split_conflict(a, b, q_lo, q_hi, g_lo, g_hi, text_rc, contig, max_overlap_permille) -> tuple:
    """(dup, conflict, ovl_q) of two alignments under bmv_split's rules (include/bmv.h)."""
    ovl_q = max(0, min(int(q_hi[a]), int(q_hi[b])) - max(int(q_lo[a]), int(q_lo[b])))
    ovl_g = max(0, min(int(g_hi[a]), int(g_hi[b])) - max(int(g_lo[a]), int(g_lo[b])))
    same = (contig is None or int(contig[a]) == int(contig[b])) and bool(text_rc[a]) == bool(text_rc[b])
    dup = same and ovl_g > 0 and ovl_q > 0
    shorter = min(int(q_hi[a]) - int(q_lo[a]), int(q_hi[b]) - int(q_lo[b]))
    return dup, dup or ovl_q * 1000 > int(max_overlap_permille) * shorter, ovl_q


def select_segments(score, q_lo, q_hi, g_lo, g_hi, text_rc, group_offset, min_score, max_overlap_permille, max_segments,
                    contig=None) -> dict:
    """bmv_split's pick (include/bmv.h) over numbers, in plain Python: per group the chosen list -- while it is shorter than
    max_segments, the eligible alignment (score >= min_score) that conflicts with none of the chosen and has the greatest
    score, the lowest batch index among equals -- and per chosen one the competitor score s2.  Returns n_seg u32[n_groups],
    seg u32[n_groups, max_segments] (BEYOND in unused slots) and s2 i64[n_groups, max_segments] (SPLIT_NONE)."""
    n_groups = len(group_offset) - 1
    n_seg = np.zeros(n_groups, np.uint32)
    seg = np.full((n_groups, int(max_segments)), BEYOND, np.uint32)
    s2 = np.full((n_groups, int(max_segments)), SPLIT_NONE, np.int64)
    arrays = (q_lo, q_hi, g_lo, g_hi, text_rc, contig, max_overlap_permille)
    for g in range(n_groups):
        members = range(int(group_offset[g]), int(group_offset[g + 1]))
        chosen = []
        while len(chosen) < int(max_segments):
            top = None
            for a in members:
                if a in chosen or int(score[a]) < int(min_score) or any(split_conflict(a, c, *arrays)[1] for c in chosen):
                    continue
                if top is None or int(score[a]) > int(score[top]):
                    top = a
            if top is None:
                break
            chosen.append(top)
        n_seg[g] = len(chosen)
        for k, c in enumerate(chosen):
            seg[g, k] = c
            for a in members:
                if a in chosen or int(score[a]) <= 0:
                    continue
                dup, _, ovl_q = split_conflict(a, c, *arrays)
                if not dup and 2 * ovl_q >= int(q_hi[c]) - int(q_lo[c]):
                    s2[g, k] = max(int(s2[g, k]), int(score[a]))
    return {"n_seg": n_seg, "seg": seg, "s2": s2}


def split_mapq(s1, s2) -> int:
    """The MAPQ of a chosen segment from its score and its competitor's (host/split_pick.h; a definition by choice, like
    best_mapq): 60 without a competitor, 0 when the competitor is no worse, else (s1 - s2) * 60 / s1."""
    s1, s2 = int(s1), int(s2)
    if s2 == SPLIT_NONE:
        return 60
    if s2 >= s1 or s1 <= 0:                      # (a chosen segment has s1 >= min_score >= 1)
        return 0
    return (s1 - s2) * 60 // s1


def sa_entry(rname, pos0, reverse, xcigar, mapq, nm) -> str:
    """One entry of SAM's SA:Z tag (host/split_pick.h): rname,pos,strand,CIGAR,mapQ,NM; -- pos 1-based, the written CIGAR with
    its = and X runs merged into M."""
    out, run = [], 0
    for e in xcigar:
        op, n = int(e) & 15, int(e) >> 4
        if op in (0, 7, 8):
            run += n
            continue
        if run:
            out.append(f"{run}M")
            run = 0
        out.append(f"{n}{'MIDNSHP=X'[op]}")
    if run:
        out.append(f"{run}M")
    return f"{rname},{int(pos0) + 1},{'-' if reverse else '+'},{''.join(out)},{int(mapq)},{int(nm)};"


def select_best(d, end, group_offset, margin):
    """The contract of bmv_align_best in plain numpy, from every alignment's distance d[a] and end column end[a] (begin + M
    and D lengths of its CIGAR): returns (winner u32[n_groups], edits u32[n], end u32[n]).  winner[g] is the lowest batch
    index with the group's smallest distance (BEYOND for an empty group); edits / end are d / end where d <= best + margin[g]
    and BEYOND / 0 elsewhere."""
    d, end = np.asarray(d, np.int64), np.asarray(end, np.int64)
    off, margin = np.asarray(group_offset, np.int64), np.asarray(margin, np.int64)
    n_groups = len(off) - 1
    if len(margin) != n_groups or len(d) != len(end):
        raise ValueError("one margin per group, one end per distance")
    if n_groups < 0 or off[0] != 0 or off[-1] != len(d) or (np.diff(off) < 0).any():
        raise ValueError("group_offset must run from 0 to the number of alignments without decreasing")
    winner = np.full(n_groups, BEYOND, np.uint32)
    edits, out_end = np.full(len(d), BEYOND, np.uint32), np.zeros(len(d), np.uint32)
    for g in range(n_groups):
        a0, a1 = int(off[g]), int(off[g + 1])
        if a0 == a1:
            continue
        best = int(d[a0:a1].min())
        winner[g] = a0 + int(np.argmax(d[a0:a1] == best))
        within = d[a0:a1] <= best + int(margin[g])
        edits[a0:a1][within] = d[a0:a1][within]
        out_end[a0:a1][within] = end[a0:a1][within]
    return winner, edits, out_end


def best_mapq(winner, edits, end, text_start, text_len, text_rc, margin) -> tuple:
    """MAPQ and X0 of one group's winner (host/best_mapq.h; a definition by choice).  winner: its index in the
    group's arrays; edits / end: the group's slice of align_best's outputs; text_start / text_len / text_rc: the group's
    windows; margin: the group's M.  The other alignments within the margin (edits != BEYOND) count unless they lie at the
    winner's own locus -- the same strand and the same genome coordinate of the end: text_start + end forward,
    text_start + text_len - end reverse (overlapping windows find one alignment twice).  With e1 the winner's edits and e2
    the smallest among the others: none -> 60; e2 = e1 -> 0; else (e2 - e1) * 60 // (M + 1).  X0: distinct loci at e1, the
    winner's included.  Returns (mapq, x0)."""
    def locus(a):
        rc = int(text_rc[a]) != 0
        at = int(text_start[a]) + int(text_len[a]) - int(end[a]) if rc else int(text_start[a]) + int(end[a])
        return (rc, at)
    e1, home = int(edits[winner]), locus(winner)
    others = {}
    for a in range(len(edits)):
        if a == winner or int(edits[a]) == BEYOND or locus(a) == home:
            continue
        others[locus(a)] = min(int(edits[a]), others.get(locus(a), BEYOND))
    x0 = 1 + sum(1 for e in others.values() if e == e1)
    if not others:
        return 60, x0
    e2 = min(others.values())
    return (0 if e2 == e1 else min(60, (e2 - e1) * 60 // (int(margin) + 1))), x0


def pair_coordinates(text_start, text_len, text_rc, query_len, end):
    """L, R and the locus coordinate of every alignment as bmv_pair defines them (include/bmv.h), int64: forward R = text_start
    + end and L = R - query_len; reverse L = text_start + text_len - end and R = L + query_len; the locus is R forward, L
    reverse -- the exact one of the two."""
    ts, tl = np.asarray(text_start).astype(np.int64), np.asarray(text_len).astype(np.int64)
    rc, m, e = np.asarray(text_rc) != 0, np.asarray(query_len).astype(np.int64), np.asarray(end).astype(np.int64)
    left = np.where(rc, ts + tl - e, ts + e - m)
    right = np.where(rc, ts + tl - e + m, ts + e)
    return left, right, np.where(rc, left, right)


def select_pairs(text_start, text_len, text_rc, query_len, edits, end, group_offset, min_frag, max_frag, contig=None) -> dict:
    """The contract of bmv_pair in plain numpy (include/bmv.h): the mates of pair p are the groups 2p and 2p + 1; a combination
    of a known alignment of each (edits != BEYOND) is proper when the two lie on one contig and on different strands and, with
    f the forward and r the reverse one, L(f) <= L(r), R(f) <= R(r) and min_frag <= R(r) - L(f) <= max_frag.  The pick minimises
    (edits[i] + edits[j], i, j); s1 is its sum, s2 the smallest sum over the proper combinations that differ from it in the
    locus of either mate.  Returns a dict: pick u32[n_groups] (the group's own winner -- the lowest known index with the
    smallest edits, BEYOND when there is none -- where the pair has no proper combination), proper u8[n_pairs], s1 and s2
    u64[n_pairs] (PAIR_NONE where undefined), winner u32[n_groups]."""
    off = np.asarray(group_offset, np.int64)
    ed = np.asarray(edits).astype(np.int64)
    n, n_groups = len(ed), len(off) - 1
    if n_groups < 0 or n_groups % 2 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError("group_offset must run from 0 to the number of alignments without decreasing, over an even number of groups")
    if int(min_frag) > int(max_frag):
        raise ValueError("min_frag is larger than max_frag")
    left, right, at = pair_coordinates(text_start, text_len, text_rc, query_len, end)
    rc = np.asarray(text_rc) != 0
    ctg = np.zeros(n, np.int64) if contig is None else np.asarray(contig).astype(np.int64)
    known = ed != BEYOND
    winner = np.full(n_groups, BEYOND, np.uint32)
    for g in range(n_groups):
        a0, a1 = int(off[g]), int(off[g + 1])
        if known[a0:a1].any():
            winner[g] = a0 + int(np.argmin(np.where(known[a0:a1], ed[a0:a1], 2 ** 40)))
    pick = winner.copy()
    n_pairs = n_groups // 2
    proper = np.zeros(n_pairs, np.uint8)
    s1, s2 = np.full(n_pairs, PAIR_NONE, np.uint64), np.full(n_pairs, PAIR_NONE, np.uint64)
    for p in range(n_pairs):
        i, j = np.arange(off[2 * p], off[2 * p + 1]), np.arange(off[2 * p + 1], off[2 * p + 2])
        if len(i) == 0 or len(j) == 0:
            continue
        I, J = i[:, None], j[None, :]
        fwd_i = ~rc[I] & rc[J]                                   # i is the forward one (else j, where the strands differ)
        fl, fr = np.where(fwd_i, left[I], left[J]), np.where(fwd_i, right[I], right[J])
        rl, rr = np.where(fwd_i, left[J], left[I]), np.where(fwd_i, right[J], right[I])
        ok = known[I] & known[J] & (ctg[I] == ctg[J]) & (rc[I] != rc[J]) & (fl <= rl) & (fr <= rr) & \
            (rr - fl >= int(min_frag)) & (rr - fl <= int(max_frag))
        if not ok.any():
            continue
        total = np.where(ok, ed[I] + ed[J], 2 ** 40)
        k = int(np.argmin(total))                                # row-major: the lowest i, then the lowest j, of the minimum
        bi, bj = int(i[k // len(j)]), int(j[k % len(j)])
        pick[2 * p], pick[2 * p + 1], proper[p], s1[p] = bi, bj, 1, int(total.ravel()[k])
        other = ok & ((rc[I] != rc[bi]) | (at[I] != at[bi]) | (rc[J] != rc[bj]) | (at[J] != at[bj]))
        if other.any():
            s2[p] = int(total[other].min())
    return {"pick": pick, "proper": proper, "s1": s1, "s2": s2, "winner": winner}


FRAG_MAX_CAP = 65535


def frag_spans(text_start, text_len, text_rc, query_len, edits, end, group_offset, cap, contig=None):
    """The contract of bmv_frag_spans in plain numpy (include/bmv.h): span u32[n_groups // 2].  A group is settled when it has
    an own winner (the lowest known index with the smallest edits) and every known alignment of the group lies at the winner's
    locus; span[p] is R(r) - L(f) of the two own winners when both groups are settled and the winners are proper under
    min_frag = 1, max_frag = cap, else 0."""
    off = np.asarray(group_offset, np.int64)
    ed = np.asarray(edits).astype(np.int64)
    n, n_groups = len(ed), len(off) - 1
    if n_groups < 0 or n_groups % 2 or off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any():
        raise ValueError("group_offset must run from 0 to the number of alignments without decreasing, over an even number of groups")
    if not 1 <= int(cap) <= FRAG_MAX_CAP:
        raise ValueError(f"cap must lie in 1 .. {FRAG_MAX_CAP}")
    left, right, at = pair_coordinates(text_start, text_len, text_rc, query_len, end)
    rc = np.asarray(text_rc) != 0
    ctg = np.zeros(n, np.int64) if contig is None else np.asarray(contig).astype(np.int64)
    known = ed != BEYOND

    def settled_winner(a0, a1):
        if not known[a0:a1].any():
            return None
        w = a0 + int(np.argmin(np.where(known[a0:a1], ed[a0:a1], 2 ** 40)))
        k = known[a0:a1]
        return w if ((rc[a0:a1][k] == rc[w]) & (at[a0:a1][k] == at[w])).all() else None

    span = np.zeros(n_groups // 2, np.uint32)
    for p in range(n_groups // 2):
        i, j = settled_winner(int(off[2 * p]), int(off[2 * p + 1])), settled_winner(int(off[2 * p + 1]), int(off[2 * p + 2]))
        if i is None or j is None or rc[i] == rc[j] or ctg[i] != ctg[j]:
            continue
        f, r = (j, i) if rc[i] else (i, j)
        frag = int(right[r]) - int(left[f])
        if left[f] <= left[r] and right[f] <= right[r] and 1 <= frag <= int(cap):
            span[p] = frag
    return span


def frag_histogram(span, cap):
    """hist u64[cap + 1]: hist[s] is the number of pairs with span == s; hist[0] counts the uninformative pairs."""
    span = np.asarray(span).astype(np.int64)
    if not 1 <= int(cap) <= FRAG_MAX_CAP:
        raise ValueError(f"cap must lie in 1 .. {FRAG_MAX_CAP}")
    if len(span) and (span.min() < 0 or span.max() > int(cap)):
        raise ValueError("a span beyond cap")
    return np.bincount(span, minlength=int(cap) + 1).astype(np.uint64)


def frag_range(hist, min_pairs, fallback) -> dict:
    """The range from a histogram (host/frag_range.h; a definition by choice).  n = the sum of hist[s] over s >= 1;
    learned iff n >= max(1, min_pairs), else the fallback (min_frag, max_frag) comes back unchanged.  With v the informative
    spans in ascending order, Qk = v[k * n // 4] for k = 1, 2, 3, IQR = Q3 - Q1, slack = max(3 * IQR, ceil(Q2 / 4)),
    min_frag = max(1, Q1 - slack), max_frag = Q3 + slack.  Returns a dict: min_frag, max_frag, learned, n_informative,
    quartiles (a tuple, (0, 0, 0) when not learned)."""
    h = [int(x) for x in np.asarray(hist).tolist()]
    n = sum(h[1:])
    out = {"min_frag": int(fallback[0]), "max_frag": int(fallback[1]), "learned": False, "n_informative": n, "quartiles": (0, 0, 0)}
    if n < max(1, int(min_pairs)):
        return out
    upto = np.cumsum(np.asarray(h[1:], np.int64))               # v[i] is the first s with upto[s - 1] > i
    q = [1 +int(np.searchsorted(upto, k * n // 4, side="right")) for k in (1, 2, 3)]
    slack = max(3 * (q[2] - q[0]), -(-q[1] // 4))
    out.update({"min_frag": max(1, q[0] - slack), "max_frag": q[2] + slack, "learned": True, "quartiles": tuple(q)})
    return out


def pair_mapq(proper, s1, s2, mates) -> list:
    """MAPQ and X0 of the two mates of one pair (host/pair_mapq.h; a definition by choice).  mates: two dicts, one
    per mate, of the mate's own group -- pick and winner (indices INSIDE the group, as select_pairs / align_paired return them
    minus the group's offset), edits, end, text_start, text_len, text_rc (the group's slices) and margin.  A pair that is not
    proper: each mate gets best_mapq of its own winner.  A proper one, with M the sum of the two margins: q_pair = 60 when s2 is
    PAIR_NONE, 0 when s2 == s1, else min(60, (s2 - s1) * 60 // (M + 1)); q_single = best_mapq's value when the pick is the
    group's own winner, else 0; MAPQ = max(q_pair, q_single); X0 = the distinct loci of the mate's own group at the pick's
    edits, its own included.  Returns [(mapq, x0), (mapq, x0)]."""
    def single(m):
        return best_mapq(m["winner"], m["edits"], m["end"], m["text_start"], m["text_len"], m["text_rc"], m["margin"])
    if not proper:
        return [single(m) for m in mates]
    big_m = sum(int(m["margin"]) for m in mates)
    s1, s2 = int(s1), int(s2)
    q_pair = 60 if s2 == PAIR_NONE else 0 if s2 == s1 else min(60, (s2 - s1) * 60 // (big_m + 1))
    out = []
    for m in mates:
        pick, e = int(m["pick"]), [int(x) for x in m["edits"]]
        q_single = single(m)[0] if pick == int(m["winner"]) else 0
        loci = set()
        for a in range(len(e)):
            if e[a] == e[pick]:
                rc = int(m["text_rc"][a]) != 0
                loci.add((rc, int(m["text_start"][a]) + (int(m["text_len"][a]) - int(m["end"][a]) if rc else int(m["end"][a]))))
        out.append((max(q_pair, q_single), len(loci)))
    return out


def rescue_window(anchor_text_start, anchor_text_len, anchor_text_rc, anchor_query_len, anchor_end, contig_start, contig_end,
                  query_len, max_edits, min_frag, max_frag) -> tuple:
    """The window of bmv_rescue for one job in plain Python integers (include/bmv.h; host/pair_rescue.h is the C++ restatement):
    where a mate of query_len bases may lie beside the anchor -- a known alignment of its partner, given as bmv_pair takes one
    -- within min(max_edits, query_len) edits, cut to the contig [contig_start, contig_end).  Returns (text_start, text_len,
    text_rc) of the view the mate is aligned against."""
    ts, tl, m, end = int(anchor_text_start), int(anchor_text_len), int(query_len), int(anchor_end)
    k, c0, c1, lo, hi = min(int(max_edits), m), int(contig_start), int(contig_end), int(min_frag), int(max_frag)
    if int(anchor_text_rc):
        la = ts + tl - end
        ra = la + int(anchor_query_len)
        z_lo, z_hi = ra + m - hi, min(la + m, ra, ra + m - lo)
        ws, we, rc = max(c0, z_lo - m - k), min(c1, z_hi), 0
    else:
        ra = ts + end
        la = ra - int(anchor_query_len)
        x_lo, x_hi = max(la, ra - m, la + lo - m), la + hi - m
        ws, we, rc = max(c0, x_lo), min(c1, x_hi + m + k), 1
    return ws, max(0, we - ws), rc


def rescue_bound(rate, length) -> int:
    """(uint32_t)(rate x length) in single precision, as bucketmap_align --rescue-rate computes an edit bound."""
    return int(np.float32(rate) * np.float32(length))


def select_rescue(proper, anchor_edits, read_len, rate, rescued_edits=None, rescued_proper=None) -> dict:
    """Which rescue jobs a pair gets and which result it keeps (host/pair_rescue.h, bucketmap_align --rescue).  proper: what
    bmv_pair said of the pair; anchor_edits[i]: the edits of mate i's own winner (BEYOND: it has none); read_len[i]: mate i's
    length.  A pair that is not proper gets job i -- anchored on mate i, its query the OTHER mate, max_edits = rescue_bound(rate,
    the other's length) -- when mate i's winner is known with edits <= rescue_bound(rate, read_len[i]).  With the jobs' results
    (rescued_edits[i], rescued_proper[i] of job i; ignored where there is no job): a job counts when it came back within bound
    and proper; of two that count the smaller anchor_edits[i] + rescued_edits[i] wins, a tie goes to job 0.  Returns
    {"jobs": [bool, bool], "max_edits": [int, int], "keep": None, 0 or 1}."""
    jobs = [False, False]
    bound = [rescue_bound(rate, read_len[1]), rescue_bound(rate, read_len[0])]
    if not proper:
        for i in range(2):
            jobs[i] = int(anchor_edits[i]) != BEYOND and int(anchor_edits[i]) <= rescue_bound(rate, read_len[i])
    keep = None
    if rescued_edits is not None:
        for i in range(2):
            if not jobs[i] or int(rescued_edits[i]) == BEYOND or not int(rescued_proper[i]):
                continue
            total = int(anchor_edits[i]) + int(rescued_edits[i])
            if keep is None or total < best:
                keep, best = i, total
    return {"jobs": jobs, "max_edits": bound, "keep": keep}


class Verifier:
    """align_pairwise of the BM_ALIGN branch (bucket_locator.h:520-528,569-576) for batches, on one GPU."""

    def __init__(self, max_query_len: int = 65536, max_text_len: int = 81920, device: int = 0):
        h = C.c_void_p()
        prm = _Params(max_query_len, max_text_len, device)
        _check(lib().bmv_create(C.byref(prm), C.byref(h)))
        self._h = h

    def load_genome(self, bases) -> None:
        bases = np.ascontiguousarray(bases, np.uint8)
        _check(lib().bmv_load_genome(self._h, _p(bases, _u8p), len(bases)))

    def align(self, reads, text_start, text_len, text_rc, query_start, query_len):
        """Returns (score i32[n], begin u32[n], cigar_offset u64[n+1], cigar u32[total])."""
        return self._align(lib().bmv_align, reads, text_start, text_len, text_rc, query_start, query_len)

    def align_long(self, reads, text_start, text_len, text_rc, query_start, query_len):
        """As align, without max_query_len / max_text_len: longer alignments go through the tiled long path
        (bmv_align_long); those within the limits through align's own kernels."""
        return self._align(lib().bmv_align_long, reads, text_start, text_len, text_rc, query_start, query_len)

    def align_bounded(self, reads, text_start, text_len, text_rc, query_start, query_len, max_edits):
        """As align_long, under an edit bound per alignment (bmv_align_bounded): an alignment whose edit distance
        exceeds max_edits[a] comes back with score REJECTED, begin 0 and no CIGAR entries; every other one exactly
        as align / align_long return it."""
        return self._align(lib().bmv_align_bounded, reads, text_start, text_len, text_rc, query_start, query_len,
                           max_edits)

    def bounded_stats(self) -> dict:
        """Of the last align_bounded: rejected alignments, cells the screen evaluated, the screen's kernel ms."""
        rej, cells, ms = C.c_uint32(), C.c_uint64(), C.c_float()
        _check(lib().bmv_last_bounded_stats(self._h, C.byref(rej), C.byref(cells), C.byref(ms)))
        return {"n_rejected": rej.value, "screen_cells": cells.value, "ms_screen": ms.value}

    def align_best(self, reads, text_start, text_len, text_rc, query_start, query_len, group_offset, margin, hint=None) -> dict:
        """bmv_align_best: of every group of alignments (group g owns group_offset[g] .. group_offset[g + 1] - 1) only the
        best is aligned in full.  Returns a dict: score, begin, cigar_offset, cigar as align_long returns them for the winners
        and REJECTED / 0 / no entries for everything else; winner u32[n_groups] (BEYOND for an empty group); edits u32[n] and
        end u32[n], the distance and end column of every alignment within best + margin[g] (BEYOND / 0 elsewhere).  The
        result does not depend on hint (the index inside each group to try first)."""
        r = np.ascontiguousarray(reads, np.uint8)
        ts, tl = np.ascontiguousarray(text_start, np.uint64), np.ascontiguousarray(text_len, np.uint32)
        trc = np.ascontiguousarray(text_rc, np.uint8)
        qs, ql = np.ascontiguousarray(query_start, np.uint64), np.ascontiguousarray(query_len, np.uint32)
        off, mg = np.ascontiguousarray(group_offset, np.uint32), np.ascontiguousarray(margin, np.uint32)
        n, n_groups = len(ts), len(off) - 1
        if n_groups < 0 or len(mg) != n_groups:
            raise ValueError("group_offset holds n_groups + 1 entries, margin n_groups")
        if not (len(tl) == len(trc) == len(qs) == len(ql) == n):
            raise ValueError("one entry per alignment in every array")
        hp = None
        if hint is not None:
            hn = np.ascontiguousarray(hint, np.uint32)
            if len(hn) != n_groups:
                raise ValueError("hint must hold one index per group")
            hp = _p(hn, _u32p)
        total = C.c_uint64()
        _check(lib().bmv_align_best(self._h, _p(r, _u8p), len(r), _p(ts, _u64p), _p(tl, _u32p), _p(trc, _u8p), _p(qs, _u64p),
                                    _p(ql, _u32p), n, _p(off, _u32p), n_groups, _p(mg, _u32p), hp, C.byref(total)))
        score, begin = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        co = np.zeros(n + 1, np.uint64)
        cg = np.zeros(max(total.value, 1), np.uint32)
        _check(lib().bmv_results(self._h, _p(score, _i32p), _p(begin, _u32p), _p(co, _u64p), _p(cg, _u32p)))
        winner = np.zeros(max(n_groups, 1), np.uint32)
        edits, end = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        _check(lib().bmv_best(self._h, _p(winner, _u32p), _p(edits, _u32p), _p(end, _u32p)))
        return {"score": score, "begin": begin, "cigar_offset": co, "cigar": cg[: total.value], "winner": winner[:n_groups],
                "edits": edits[:n], "end": end[:n]}

    def _pairs(self, n_groups) -> dict:
        pick, winner = np.zeros(max(n_groups, 1), np.uint32), np.zeros(max(n_groups, 1), np.uint32)
        proper = np.zeros(max(n_groups // 2, 1), np.uint8)
        s1, s2 = np.zeros(max(n_groups // 2, 1), np.uint64), np.zeros(max(n_groups // 2, 1), np.uint64)
        _check(lib().bmv_pairs(self._h, _p(pick, _u32p), _p(proper, _u8p), _p(s1, _u64p), _p(s2, _u64p), _p(winner, _u32p)))
        return {"pick": pick[:n_groups], "proper": proper[: n_groups // 2], "s1": s1[: n_groups // 2], "s2": s2[: n_groups // 2],
                "winner": winner[:n_groups]}

    def pair(self, text_start, text_len, text_rc, query_len, edits, end, group_offset, min_frag, max_frag, contig=None) -> dict:
        """bmv_pair: the pair-aware pick over alignments given by numbers alone -- the views' text_start, text_len, text_rc and
        query_len, edits and end as align_best returns them, the contig of each (None: all on one); the mates of pair p are
        the groups 2p and 2p + 1.  Returns what select_pairs returns: pick, proper, s1, s2, winner."""
        ts, tl = np.ascontiguousarray(text_start, np.uint64), np.ascontiguousarray(text_len, np.uint32)
        trc, ql = np.ascontiguousarray(text_rc, np.uint8), np.ascontiguousarray(query_len, np.uint32)
        ed, en = np.ascontiguousarray(edits, np.uint32), np.ascontiguousarray(end, np.uint32)
        off = np.ascontiguousarray(group_offset, np.uint32)
        n, n_groups = len(ts), len(off) - 1
        if n_groups < 0 or not (len(tl) == len(trc) == len(ql) == len(ed) == len(en) == n):
            raise ValueError("one entry per alignment in every array, n_groups + 1 in group_offset")
        cp = None
        if contig is not None:
            cn = np.ascontiguousarray(contig, np.uint32)
            if len(cn) != n:
                raise ValueError("contig must hold one entry per alignment")
            cp = _p(cn, _u32p)
        _check(lib().bmv_pair(self._h, _p(ts, _u64p), _p(tl, _u32p), _p(trc, _u8p), _p(ql, _u32p), _p(ed, _u32p), _p(en, _u32p), cp, n,
                              _p(off, _u32p), n_groups, int(min_frag), int(max_frag)))
        return self._pairs(n_groups)

    def align_paired(self, reads, text_start, text_len, text_rc, query_start, query_len, group_offset, margin, min_frag, max_frag,
                     hint=None, contig=None) -> dict:
        """bmv_align_paired: align_best for pairs.  The groups 2p and 2p + 1 are the candidates of the two mates of pair p; of
        every group the PICK of select_pairs -- over the distances and end columns within best + margin of each group -- is
        aligned in full.  Returns align_best's dict (score, begin, cigar_offset, cigar for the picks, REJECTED / 0 / no entries
        elsewhere; winner, edits, end as align_best returns them) plus pick, proper, s1 and s2.  The result does not depend on
        hint."""
        r = np.ascontiguousarray(reads, np.uint8)
        ts, tl = np.ascontiguousarray(text_start, np.uint64), np.ascontiguousarray(text_len, np.uint32)
        trc = np.ascontiguousarray(text_rc, np.uint8)
        qs, ql = np.ascontiguousarray(query_start, np.uint64), np.ascontiguousarray(query_len, np.uint32)
        off, mg = np.ascontiguousarray(group_offset, np.uint32), np.ascontiguousarray(margin, np.uint32)
        n, n_groups = len(ts), len(off) - 1
        if n_groups < 0 or len(mg) != n_groups:
            raise ValueError("group_offset holds n_groups + 1 entries, margin n_groups")
        if not (len(tl) == len(trc) == len(qs) == len(ql) == n):
            raise ValueError("one entry per alignment in every array")
        hp = cp = None
        if hint is not None:
            hn = np.ascontiguousarray(hint, np.uint32)
            if len(hn) != n_groups:
                raise ValueError("hint must hold one index per group")
            hp = _p(hn, _u32p)
        if contig is not None:
            cn = np.ascontiguousarray(contig, np.uint32)
            if len(cn) != n:
                raise ValueError("contig must hold one entry per alignment")
            cp = _p(cn, _u32p)
        total = C.c_uint64()
        _check(lib().bmv_align_paired(self._h, _p(r, _u8p), len(r), _p(ts, _u64p), _p(tl, _u32p), _p(trc, _u8p), _p(qs, _u64p),
                                      _p(ql, _u32p), n, _p(off, _u32p), n_groups, _p(mg, _u32p), hp, cp, int(min_frag),
                                      int(max_frag), C.byref(total)))
        return self._paired_results(n, n_groups, total.value)

    def _paired_results(self, n, n_groups, total) -> dict:
        total = C.c_uint64(total)
        score, begin = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        co = np.zeros(n + 1, np.uint64)
        cg = np.zeros(max(total.value, 1), np.uint32)
        _check(lib().bmv_results(self._h, _p(score, _i32p), _p(begin, _u32p), _p(co, _u64p), _p(cg, _u32p)))
        winner = np.zeros(max(n_groups, 1), np.uint32)
        edits, end = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        _check(lib().bmv_best(self._h, _p(winner, _u32p), _p(edits, _u32p), _p(end, _u32p)))
        out = self._pairs(n_groups)
        out.update({"score": score, "begin": begin, "cigar_offset": co, "cigar": cg[: total.value], "winner": winner[:n_groups],
                    "edits": edits[:n], "end": end[:n]})
        return out

    def _frag(self, n_pairs, cap) -> dict:
        span, hist = np.zeros(max(n_pairs, 1), np.uint32), np.zeros(int(cap) + 1, np.uint64)
        _check(lib().bmv_frag(self._h, _p(span, _u32p), _p(hist, _u64p)))
        return {"span": span[:n_pairs], "hist": hist}

    def frag(self, n_pairs, cap) -> dict:
        """bmv_frag: span u32[n_pairs] and hist u64[cap + 1] of the last frag_spans or paired_begin with cap > 0 -- the caller
        says how large that call was."""
        return self._frag(int(n_pairs), int(cap))

    def frag_spans(self, text_start, text_len, text_rc, query_len, edits, end, group_offset, cap, contig=None) -> dict:
        """bmv_frag_spans: the fragment spans over alignments given by numbers alone, as pair takes them.  Returns span (what
        the module's frag_spans returns) and hist (frag_histogram of it)."""
        ts, tl = np.ascontiguousarray(text_start, np.uint64), np.ascontiguousarray(text_len, np.uint32)
        trc, ql = np.ascontiguousarray(text_rc, np.uint8), np.ascontiguousarray(query_len, np.uint32)
        ed, en = np.ascontiguousarray(edits, np.uint32), np.ascontiguousarray(end, np.uint32)
        off = np.ascontiguousarray(group_offset, np.uint32)
        n, n_groups = len(ts), len(off) - 1
        if n_groups < 0 or not (len(tl) == len(trc) == len(ql) == len(ed) == len(en) == n):
            raise ValueError("one entry per alignment in every array, n_groups + 1 in group_offset")
        cp = None
        if contig is not None:
            cn = np.ascontiguousarray(contig, np.uint32)
            if len(cn) != n:
                raise ValueError("contig must hold one entry per alignment")
            cp = _p(cn, _u32p)
        _check(lib().bmv_frag_spans(self._h, _p(ts, _u64p), _p(tl, _u32p), _p(trc, _u8p), _p(ql, _u32p), _p(ed, _u32p), _p(en, _u32p), cp,
                                    n, _p(off, _u32p), n_groups, int(cap)))
        return self._frag(n_groups // 2, cap)

    def frag_stats(self) -> dict:
        """Of the last frag_spans or paired_begin with cap > 0: the two kernels' ms and the informative pairs."""
        ms, inf = C.c_float(), C.c_uint32()
        _check(lib().bmv_last_frag_stats(self._h, C.byref(ms), C.byref(inf)))
        return {"ms_kernels": ms.value, "n_informative": inf.value}

    def paired_begin(self, reads, text_start, text_len, text_rc, query_start, query_len, group_offset, margin, cap, hint=None,
                     contig=None):
        """bmv_paired_begin: the first half of align_paired -- everything but the pick under a range.  cap > 0 also computes the
        fragment spans of the batch; returns frag's dict then, None for cap = 0.  The arrays are kept alive (and must stay
        unchanged) until paired_finish."""
        r = np.ascontiguousarray(reads, np.uint8)
        ts, tl = np.ascontiguousarray(text_start, np.uint64), np.ascontiguousarray(text_len, np.uint32)
        trc = np.ascontiguousarray(text_rc, np.uint8)
        qs, ql = np.ascontiguousarray(query_start, np.uint64), np.ascontiguousarray(query_len, np.uint32)
        off, mg = np.ascontiguousarray(group_offset, np.uint32), np.ascontiguousarray(margin, np.uint32)
        n, n_groups = len(ts), len(off) - 1
        if n_groups < 0 or len(mg) != n_groups:
            raise ValueError("group_offset holds n_groups + 1 entries, margin n_groups")
        if not (len(tl) == len(trc) == len(qs) == len(ql) == n):
            raise ValueError("one entry per alignment in every array")
        hn = cn = hp = cp = None
        if hint is not None:
            hn = np.ascontiguousarray(hint, np.uint32)
            if len(hn) != n_groups:
                raise ValueError("hint must hold one index per group")
            hp = _p(hn, _u32p)
        if contig is not None:
            cn = np.ascontiguousarray(contig, np.uint32)
            if len(cn) != n:
                raise ValueError("contig must hold one entry per alignment")
            cp = _p(cn, _u32p)
        _check(lib().bmv_paired_begin(self._h, _p(r, _u8p), len(r), _p(ts, _u64p), _p(tl, _u32p), _p(trc, _u8p), _p(qs, _u64p),
                                      _p(ql, _u32p), n, _p(off, _u32p), n_groups, _p(mg, _u32p), hp, cp, int(cap)))
        self._pending = (n, n_groups, (r, ts, tl, trc, qs, ql, off, mg, hn, cn))
        return self._frag(n_groups // 2, cap) if int(cap) else None

    def paired_finish(self, min_frag, max_frag) -> dict:
        """bmv_paired_finish: the pick under [min_frag, max_frag] and the picks' full alignments; returns exactly what
        align_paired with that range returns for the batch of the pending paired_begin."""
        n, n_groups, _ = getattr(self, "_pending", None) or (0, 0, None)
        total = C.c_uint64()
        try:
            _check(lib().bmv_paired_finish(self._h, int(min_frag), int(max_frag), C.byref(total)))
        except BmvError as e:
            if e.code != 1:                     # (BMV_ERR_ARG: the begin stays pending)
                self._pending = None
            raise
        self._pending = None
        return self._paired_results(n, n_groups, total.value)

    def rescue(self, reads, anchor_text_start, anchor_text_len, anchor_text_rc, anchor_query_len, anchor_end, contig_start, contig_end,
               query_start, query_len, max_edits, min_frag, max_frag) -> dict:
        """bmv_rescue: job j places the mate reads[query_start[j], +query_len[j]) beside its anchor -- a known alignment of its
        partner as bmv_pair takes one -- on the contig [contig_start[j], contig_end[j]), within max_edits[j] edits.  Returns
        text_start, text_len, text_rc (the view rescue_window gives), edits and end (BEYOND / 0 beyond the bound) and proper."""
        r = np.ascontiguousarray(reads, np.uint8)
        ats, atl = np.ascontiguousarray(anchor_text_start, np.uint64), np.ascontiguousarray(anchor_text_len, np.uint32)
        arc, aql = np.ascontiguousarray(anchor_text_rc, np.uint8), np.ascontiguousarray(anchor_query_len, np.uint32)
        aen = np.ascontiguousarray(anchor_end, np.uint32)
        c0, c1 = np.ascontiguousarray(contig_start, np.uint64), np.ascontiguousarray(contig_end, np.uint64)
        qs, ql = np.ascontiguousarray(query_start, np.uint64), np.ascontiguousarray(query_len, np.uint32)
        me = np.ascontiguousarray(max_edits, np.uint32)
        n = len(ats)
        if not (len(atl) == len(arc) == len(aql) == len(aen) == len(c0) == len(c1) == len(qs) == len(ql) == len(me) == n):
            raise ValueError("one entry per job in every array")
        _check(lib().bmv_rescue(self._h, _p(r, _u8p), len(r), _p(ats, _u64p), _p(atl, _u32p), _p(arc, _u8p), _p(aql, _u32p),
                                _p(aen, _u32p), _p(c0, _u64p), _p(c1, _u64p), _p(qs, _u64p), _p(ql, _u32p), _p(me, _u32p), n,
                                int(min_frag), int(max_frag)))
        ts, tl, trc = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8)
        edits, end, proper = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8)
        _check(lib().bmv_rescued(self._h, _p(ts, _u64p), _p(tl, _u32p), _p(trc, _u8p), _p(edits, _u32p), _p(end, _u32p),
                                 _p(proper, _u8p)))
        return {"text_start": ts[:n], "text_len": tl[:n], "text_rc": trc[:n], "edits": edits[:n], "end": end[:n],
                "proper": proper[:n]}

    def rescue_stats(self) -> dict:
        """Of the last rescue: the kernels' ms, the cells they stand for and the parts a job was cut into."""
        ms, cells, parts = C.c_float(), C.c_uint64(), C.c_uint32()
        _check(lib().bmv_last_rescue_stats(self._h, C.byref(ms), C.byref(cells), C.byref(parts)))
        return {"ms_kernels": ms.value, "cells": cells.value, "parts": parts.value}

    def pair_stats(self) -> dict:
        """Of the last pair or align_paired: the pair kernel's ms and the combinations it examined."""
        ms, combos = C.c_float(), C.c_uint64()
        _check(lib().bmv_last_pair_stats(self._h, C.byref(ms), C.byref(combos)))
        return {"ms_pair": ms.value, "combinations": combos.value}

    def best_stats(self) -> dict:
        """Of the last align_best: seeds aligned in full, alignments in the distance round, of these proven beyond the bound
        and given up on, winners aligned in full after the pick, cells of the distance round, kernel ms of both."""
        u = [C.c_uint32() for _ in range(5)]
        cells, ms_d, ms_p = C.c_uint64(), C.c_float(), C.c_float()
        _check(lib().bmv_last_best_stats(self._h, *(C.byref(x) for x in u), C.byref(cells), C.byref(ms_d), C.byref(ms_p)))
        names = ("n_seed", "n_distance", "n_beyond", "n_undecided", "n_realigned")
        return {**{k: x.value for k, x in zip(names, u)}, "distance_cells": cells.value, "ms_distance": ms_d.value,
                "ms_pick": ms_p.value}

    def _align(self, fn, reads, text_start, text_len, text_rc, query_start, query_len, max_edits=None):
        r = np.ascontiguousarray(reads, np.uint8)
        ts, tl = np.ascontiguousarray(text_start, np.uint64), np.ascontiguousarray(text_len, np.uint32)
        trc = np.ascontiguousarray(text_rc, np.uint8)
        qs, ql = np.ascontiguousarray(query_start, np.uint64), np.ascontiguousarray(query_len, np.uint32)
        n = len(ts)
        total = C.c_uint64()
        bound = []
        if max_edits is not None:
            me = np.ascontiguousarray(max_edits, np.uint32)
            if len(me) != n:
                raise ValueError("max_edits must hold one bound per alignment")
            bound = [_p(me, _u32p)]
        _check(fn(self._h, _p(r, _u8p), len(r), _p(ts, _u64p), _p(tl, _u32p), _p(trc, _u8p), _p(qs, _u64p),
                  _p(ql, _u32p), *bound, n, C.byref(total)))
        score, begin = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        off = np.zeros(n + 1, np.uint64)
        cg = np.zeros(max(total.value, 1), np.uint32)
        _check(lib().bmv_results(self._h, _p(score, _i32p), _p(begin, _u32p), _p(off, _u64p), _p(cg, _u32p)))
        return score, begin, off, cg[: total.value]

    @staticmethod
    def _annotate_args(reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar):
        r = np.ascontiguousarray(reads, np.uint8)
        ts, tl = np.ascontiguousarray(text_start, np.uint64), np.ascontiguousarray(text_len, np.uint32)
        trc = np.ascontiguousarray(text_rc, np.uint8)
        qs, ql = np.ascontiguousarray(query_start, np.uint64), np.ascontiguousarray(query_len, np.uint32)
        bg, co = np.ascontiguousarray(begin, np.uint32), np.ascontiguousarray(cigar_offset, np.uint64)
        cg = np.ascontiguousarray(cigar, np.uint32)
        n = len(ts)
        if not (len(tl) == len(trc) == len(qs) == len(ql) == len(bg) == n and len(co) == n + 1):
            raise ValueError("one entry per alignment in every array, n + 1 in cigar_offset")
        if n and int(co[n]) > len(cg):
            raise ValueError("cigar_offset runs past the CIGAR entries")
        keep = (r, ts, tl, trc, qs, ql, bg, co, cg)
        return keep, n, (_p(r, _u8p), len(r), _p(ts, _u64p), _p(tl, _u32p), _p(trc, _u8p), _p(qs, _u64p), _p(ql, _u32p),
                         _p(bg, _u32p), _p(co, _u64p), _p(cg, _u32p), n)

    def annotate(self, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar):
        """bmv_annotate on alignments given with their begin and M/I/D CIGAR (what align* returned, or hand-made): returns
        (nm u32[n], pos u32[n], ref_len u32[n], xcigar_offset u64[n+1], xcigar u32[..], ref_offset u64[n+1], ref_bases
        u8[..]) in forward-strand coordinates; see include/bmv.h.  Leaves the results of the last align* untouched."""
        _keep, n, args = self._annotate_args(reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset,
                                             cigar)
        n_x, n_r = C.c_uint64(), C.c_uint64()
        _check(lib().bmv_annotate(self._h, *args, C.byref(n_x), C.byref(n_r)))
        nm, pos, ref_len = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        xo, ro = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        xc, rb = np.zeros(max(n_x.value, 1), np.uint32), np.zeros(max(n_r.value, 1), np.uint8)
        _check(lib().bmv_annotations(self._h, _p(nm, _u32p), _p(pos, _u32p), _p(ref_len, _u32p), _p(xo, _u64p), _p(xc, _u32p),
                                     _p(ro, _u64p), _p(rb, _u8p)))
        return nm, pos, ref_len, xo, xc[: n_x.value], ro, rb[: n_r.value]

    def annotate_stats(self) -> dict:
        """Of the last annotate: kernel ms (count pass, prefix sums, write pass) and the alignment columns walked."""
        ms, cols = C.c_float(), C.c_uint64()
        _check(lib().bmv_last_annotate_stats(self._h, C.byref(ms), C.byref(cols)))
        return {"ms_kernels": ms.value, "columns": cols.value}

    def clip(self, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar, match=1,
             penalty=2) -> dict:
        """bmv_clip on the alignments annotate takes: of each, the contiguous range of columns that scores best under
        +match per = column and -penalty per X, I or D column is kept and the rest of the query soft-clipped (include/bmv.h).
        Returns a dict of annotate's seven arrays by name -- nm, pos, ref_len, xcigar_offset, xcigar (with S entries),
        ref_offset, ref_bases, all of the kept part -- plus score i64[n], clip_left u32[n] and clip_right u32[n].  Leaves the
        results of the last align* and of the last annotate untouched."""
        _keep, n, args = self._annotate_args(reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset,
                                             cigar)
        n_x, n_r = C.c_uint64(), C.c_uint64()
        _check(lib().bmv_clip(self._h, *args, int(match), int(penalty), C.byref(n_x), C.byref(n_r)))
        score = np.zeros(n, np.int64)
        left, right, nm, pos, ref_len = (np.zeros(n, np.uint32) for _ in range(5))
        xo, ro = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        xc, rb = np.zeros(max(n_x.value, 1), np.uint32), np.zeros(max(n_r.value, 1), np.uint8)
        _check(lib().bmv_clipped(self._h, _p(score, _i64p), _p(left, _u32p), _p(right, _u32p), _p(nm, _u32p), _p(pos, _u32p),
                                 _p(ref_len, _u32p), _p(xo, _u64p), _p(xc, _u32p), _p(ro, _u64p), _p(rb, _u8p)))
        return {"score": score, "clip_left": left, "clip_right": right, "nm": nm, "pos": pos, "ref_len": ref_len,
                "xcigar_offset": xo, "xcigar": xc[: n_x.value], "ref_offset": ro, "ref_bases": rb[: n_r.value]}

    def clip_stats(self) -> dict:
        """Of the last clip: kernel ms (range pass, count pass, prefix sums, write pass) and the alignment columns walked."""
        ms, cols = C.c_float(), C.c_uint64()
        _check(lib().bmv_last_clip_stats(self._h, C.byref(ms), C.byref(cols)))
        return {"ms_kernels": ms.value, "columns": cols.value}

    def overlap(self, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar, mate, contig=None,
                match=1, penalty=2) -> dict:
        """bmv_overlap on the alignments clip takes: clip's record (all columns kept when match == penalty == 0), and where
        the two mates of a pair -- mate[a] the batch index of a's mate, or NO_MATE -- overlap on one contig without
        containment, both soft-clipped at one cut so that no reference base lies under both (include/bmv.h).  Returns clip's
        dict plus cut u32[n] (the query bases the cut clipped), pairs_cut and bases_cut.  Leaves the results of every other
        call untouched."""
        _keep, n, args = self._annotate_args(reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset,
                                             cigar)
        mt = np.ascontiguousarray(mate, np.uint32)
        ct = None if contig is None else np.ascontiguousarray(contig, np.uint32)
        if len(mt) != n or (ct is not None and len(ct) != n):
            raise ValueError("one mate (and one contig) per alignment")
        n_x, n_r = C.c_uint64(), C.c_uint64()
        _check(lib().bmv_overlap(self._h, *args[:-1], _p(mt, _u32p), None if ct is None else _p(ct, _u32p), n, int(match),
                                 int(penalty), C.byref(n_x), C.byref(n_r)))
        score = np.zeros(n, np.int64)
        left, right, nm, pos, ref_len, cut = (np.zeros(n, np.uint32) for _ in range(6))
        xo, ro = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        xc, rb = np.zeros(max(n_x.value, 1), np.uint32), np.zeros(max(n_r.value, 1), np.uint8)
        _check(lib().bmv_overlapped(self._h, _p(score, _i64p), _p(left, _u32p), _p(right, _u32p), _p(nm, _u32p), _p(pos, _u32p),
                                    _p(ref_len, _u32p), _p(xo, _u64p), _p(xc, _u32p), _p(ro, _u64p), _p(rb, _u8p), _p(cut, _u32p)))
        st = self.overlap_stats()
        return {"score": score, "clip_left": left, "clip_right": right, "nm": nm, "pos": pos, "ref_len": ref_len,
                "xcigar_offset": xo, "xcigar": xc[: n_x.value], "ref_offset": ro, "ref_bases": rb[: n_r.value], "cut": cut,
                "pairs_cut": st["pairs_cut"], "bases_cut": st["bases_cut"]}

    def overlap_stats(self) -> dict:
        """Of the last overlap: kernel ms (all passes and the prefix sums), the alignment columns walked, the pairs cut and the
        query bases the cuts clipped."""
        ms, cols, pairs, bases = C.c_float(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().bmv_last_overlap_stats(self._h, C.byref(ms), C.byref(cols), C.byref(pairs), C.byref(bases)))
        return {"ms_kernels": ms.value, "columns": cols.value, "pairs_cut": pairs.value, "bases_cut": bases.value}

    def _segments(self, n, n_groups, max_segments) -> dict:
        score, g_lo, g_hi = (np.zeros(max(n, 1), np.int64) for _ in range(3))
        q_lo, q_hi = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        slots = n_groups * max_segments
        n_seg, seg, s2 = np.zeros(max(n_groups, 1), np.uint32), np.zeros(max(slots, 1), np.uint32), np.zeros(max(slots, 1), np.int64)
        _check(lib().bmv_segments(self._h, _p(score, _i64p), _p(q_lo, _u32p), _p(q_hi, _u32p), _p(g_lo, _i64p), _p(g_hi, _i64p),
                                  _p(n_seg, _u32p), _p(seg, _u32p), _p(s2, _i64p)))
        return {"score": score[:n], "q_lo": q_lo[:n], "q_hi": q_hi[:n], "g_lo": g_lo[:n], "g_hi": g_hi[:n], "n_seg": n_seg[:n_groups],
                "seg": seg[:slots].reshape(n_groups, max_segments), "s2": s2[:slots].reshape(n_groups, max_segments)}

    @staticmethod
    def _contig_arg(contig, n):
        if contig is None:
            return None, None
        cn = np.ascontiguousarray(contig, np.uint32)
        if len(cn) != n:
            raise ValueError("contig must hold one entry per alignment")
        return cn, _p(cn, _u32p)

    def split(self, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar, group_offset,
              match=1, penalty=2, min_score=40, max_overlap_permille=500, max_segments=8, contig=None) -> dict:
        """bmv_split on the alignments clip takes, grouped by read as align_best takes them: per alignment the stretch clip
        would keep (score i64[n], q_lo / q_hi u32[n] in read orientation, g_lo / g_hi i64[n] in genome coordinates), per group
        the non-conflicting stretches in chosen order, primary first (n_seg u32[n_groups], seg u32[n_groups, max_segments] with
        BEYOND in unused slots) and their competitor scores (s2 i64[n_groups, max_segments], SPLIT_NONE); include/bmv.h has
        the contract, clip_range and select_segments restate it.  Leaves the results of every other call untouched."""
        _keep, n, args = self._annotate_args(reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset,
                                             cigar)
        off = np.ascontiguousarray(group_offset, np.uint32)
        n_groups = len(off) - 1
        if n_groups < 0:
            raise ValueError("n_groups + 1 entries in group_offset")
        _cn, cp = self._contig_arg(contig, n)
        _check(lib().bmv_split(self._h, *args[:-1], cp, n, _p(off, _u32p), n_groups, int(match), int(penalty), int(min_score),
                               int(max_overlap_permille), int(max_segments)))
        return self._segments(n, n_groups, int(max_segments))

    def split_pick(self, score, q_lo, q_hi, g_lo, g_hi, text_rc, group_offset, min_score=40, max_overlap_permille=500,
                   max_segments=8, contig=None) -> dict:
        """bmv_split_pick: split's pick alone over alignments given by numbers, as pair is.  Returns what split returns."""
        sc, gl, gh = (np.ascontiguousarray(x, np.int64) for x in (score, g_lo, g_hi))
        ql, qh = np.ascontiguousarray(q_lo, np.uint32), np.ascontiguousarray(q_hi, np.uint32)
        trc, off = np.ascontiguousarray(text_rc, np.uint8), np.ascontiguousarray(group_offset, np.uint32)
        n, n_groups = len(sc), len(off) - 1
        if n_groups < 0 or not (len(gl) == len(gh) == len(ql) == len(qh) == len(trc) == n):
            raise ValueError("one entry per alignment in every array, n_groups + 1 in group_offset")
        _cn, cp = self._contig_arg(contig, n)
        _check(lib().bmv_split_pick(self._h, _p(sc, _i64p), _p(ql, _u32p), _p(qh, _u32p), _p(gl, _i64p), _p(gh, _i64p), _p(trc, _u8p),
                                    cp, n, _p(off, _u32p), n_groups, int(min_score), int(max_overlap_permille), int(max_segments)))
        return self._segments(n, n_groups, int(max_segments))

    def split_stats(self) -> dict:
        """Of the last split or split_pick: the range kernel's and the pick kernel's ms, the alignment columns walked and
        the segments chosen."""
        ms_r, ms_p, cols, segs = C.c_float(), C.c_float(), C.c_uint64(), C.c_uint64()
        _check(lib().bmv_last_split_stats(self._h, C.byref(ms_r), C.byref(ms_p), C.byref(cols), C.byref(segs)))
        return {"ms_range": ms_r.value, "ms_pick": ms_p.value, "columns": cols.value, "n_segments": segs.value}

    def realign(self, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar, match=1,
                mismatch=4, gap_open=6, gap_extend=1, band=16) -> dict:
        """bmv_realign on the alignments annotate takes: each is aligned again under affine gap costs inside the band of
        `band` columns either side of its given path (include/bmv.h: the contract); one with a D entry longer than
        63 - 2 band, or with an empty CIGAR, is passed through with the given path's affine score.  Returns a dict: score
        i32[n], begin u32[n], realigned u8[n], cigar_offset u64[n+1], cigar u32[..] -- the shape of align's results, ready
        for annotate or clip.  Leaves the results of every other call untouched."""
        _keep, n, args = self._annotate_args(reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset,
                                             cigar)
        total = C.c_uint64()
        _check(lib().bmv_realign(self._h, *args, int(match), int(mismatch), int(gap_open), int(gap_extend), int(band),
                                 C.byref(total)))
        score, out_begin, flag = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        off = np.zeros(n + 1, np.uint64)
        cg = np.zeros(max(total.value, 1), np.uint32)
        _check(lib().bmv_realigned(self._h, _p(score, _i32p), _p(out_begin, _u32p), _p(flag, _u8p), _p(off, _u64p), _p(cg, _u32p)))
        return {"score": score, "begin": out_begin, "realigned": flag, "cigar_offset": off, "cigar": cg[: total.value]}

    def realign_stats(self) -> dict:
        """Of the last realign: kernel ms (forward, traceback, scan and gather), 64 x the query rows of the realigned
        alignments, and the alignments passed through."""
        ms, cells, passed = C.c_float(), C.c_uint64(), C.c_uint32()
        _check(lib().bmv_last_realign_stats(self._h, C.byref(ms), C.byref(cells), C.byref(passed)))
        return {"ms_kernels": ms.value, "cells": cells.value, "n_passed_through": passed.value}

    def leftalign(self, reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset, cigar) -> dict:
        """bmv_leftalign on the alignments annotate takes: every I and D entry moved to its leftmost equivalent place on the
        forward strand, same-op gaps that meet merged, a D that reaches either end dropped (include/bmv.h: the contract).
        Returns a dict: begin u32[n], cigar_offset u64[n+1], cigar u32[..] -- the shape of align's results, ready for
        annotate or clip --, changed u8[n], dropped u32[n].  Leaves the results of every other call untouched."""
        _keep, n, args = self._annotate_args(reads, text_start, text_len, text_rc, query_start, query_len, begin, cigar_offset,
                                             cigar)
        total = C.c_uint64()
        _check(lib().bmv_leftalign(self._h, *args, C.byref(total)))
        out_begin, changed, dropped = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        off = np.zeros(n + 1, np.uint64)
        cg = np.zeros(max(total.value, 1), np.uint32)
        _check(lib().bmv_leftaligned(self._h, _p(out_begin, _u32p), _p(off, _u64p), _p(cg, _u32p), _p(changed, _u8p), _p(dropped, _u32p)))
        return {"begin": out_begin, "cigar_offset": off, "cigar": cg[: total.value], "changed": changed, "dropped": dropped}

    def leftalign_stats(self) -> dict:
        """Of the last leftalign: kernel ms (walk, scan and gather), the columns compared, the alignments changed, the
        merges and the dropped bases."""
        ms, compared, changed, merges, dropped = C.c_float(), C.c_uint64(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(lib().bmv_last_leftalign_stats(self._h, C.byref(ms), C.byref(compared), C.byref(changed), C.byref(merges),
                                              C.byref(dropped)))
        return {"ms_kernels": ms.value, "compared": compared.value, "n_changed": changed.value, "merges": merges.value,
                "dropped": dropped.value}

    def stats(self) -> dict:
        ms, cells = C.c_float(), C.c_uint64()
        _check(lib().bmv_last_stats(self._h, C.byref(ms), C.byref(cells)))
        return {"ms_kernels": ms.value, "cells": cells.value}

    def close(self) -> None:
        if self._h:
            lib().bmv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
