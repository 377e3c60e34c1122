"""The read-backed phasing rule of include/bmk.h in plain Python, big integers, no wrap; written from the header's text.  The
counted records and the walk are bmp.h's (tests/pileup_rule.py, tests/depth_rule.py).

sites_of(called) -> the phase sites [(call index, ref, pos, a0, a1)] among calls of 24 words, refusing what the ABI refuses.
observed(rec, ...) -> [(site, allele)] of one record.  links(records, ref_len, called, skip, **params) -> (sites, link, n_obs)
with link an (H, reach, 4) int64 array.  phase(sites, link, **params) -> the 8 words of every site, roots found by plainly
following parents.  run(...) does all of it and adds the four sums.  phased_vcf turns the file of --vcf into the file of
--vcf --vcf-phase, unphased_vcf does the reverse by text alone; summary_line is the line on stderr."""
import bisect
import re

import numpy as np

from depth_rule import BLOCK, QUERY, REF, SKIP_FLAGS, fields, refused  # noqa: F401
from genotype_rule import LETTER_OF_CODE, VARIANT
from pileup_rule import sequence_of

DEFAULTS = dict(min_mapq=0, min_bq=13, min_links=2, min_frac_ppm=800000, reach=4)
OUT_WORDS, N_STATS, MAX_REACH = 8, 4, 8
PHASED, ROOT = 1, 2
W_CALL, W_ROOT, W_ROOT_POS, W_HAP, W_FLAGS, W_D, W_CIS, W_TRANS = range(8)
PPM = 1000000


class Refused(ValueError):
    pass


def check_params(pr):
    if not 1 <= pr["reach"] <= MAX_REACH or pr["min_links"] < 1 or not 500001 <= pr["min_frac_ppm"] <= PPM:
        raise Refused(f"parameters {pr}")


def sites_of(called, ref_len):
    out = []
    for i, c in enumerate(called):
        if not c[3] & VARIANT or c[4] == c[5]:
            continue
        if c[0] >= len(ref_len) or c[1] >= ref_len[c[0]] or c[4] > 3 or c[5] > 3:
            raise Refused(f"call {i}")
        if out and (c[0], c[1]) <= (out[-1][1], out[-1][2]):
            raise Refused(f"call {i} does not ascend")
        out.append((i, c[0], c[1], c[4], c[5]))
    return out


def counted(rec, n_ref, ref_len, skipped, min_mapq):
    ref, pos, mapq, flag, l_seq, cigar, qual = fields(rec)
    if flag & SKIP_FLAGS or skipped:
        return False
    if not (0 <= ref < n_ref and 0 <= pos < ref_len[ref]) or not cigar:
        return False
    if l_seq == 0 or (len(cigar) == 2 and cigar[0] == (l_seq << 4 | 4) and cigar[1] & 15 == 3):
        return False
    return mapq >= min_mapq


def observed(rec, ref_len, sites, keys, min_bq):
    """[(site, allele)] of a counted record; keys is [(ref, pos)] of the sites."""
    ref, pos, mapq, flag, l_seq, cigar, qual = fields(rec)
    packed = sequence_of(rec)
    out, rc, qc = [], pos, 0
    for word in cigar:
        op, length = word & 15, word >> 4
        if op in BLOCK and length and rc < ref_len[ref]:
            end = min(rc + length, ref_len[ref])
            for s in range(bisect.bisect_left(keys, (ref, rc)), bisect.bisect_left(keys, (ref, end))):
                at = qc + keys[s][1] - rc
                q = qual[at]
                letter = int(LETTER_OF_CODE[(packed[at >> 1] >> (0 if at & 1 else 4)) & 15])
                if (q == 0xFF or q >= min_bq) and letter < 4 and letter in sites[s][3:5]:
                    out.append((s, 0 if letter == sites[s][3] else 1))      # a0 != a1
        if op in REF:
            rc += length
        if op in QUERY:
            qc += length
    return out


def links(records, ref_len, called, skip=None, **params):
    pr = {**DEFAULTS, **params}
    check_params(pr)
    assert len(ref_len) > 0 and all(l > 0 for l in ref_len) and refused(records, len(ref_len)) is None
    sites = sites_of(called, ref_len)
    keys = [(s[1], s[2]) for s in sites]
    link = np.zeros((len(sites), pr["reach"], 4), np.int64)
    n_obs = 0
    for i, rec in enumerate(records):
        if not sites or not counted(rec, len(ref_len), ref_len, skip is not None and skip[i], pr["min_mapq"]):
            continue
        seen = observed(rec, ref_len, sites, keys, pr["min_bq"])
        n_obs += len(seen)
        for y, (j, a_j) in enumerate(seen):              # seen ascends: the earlier sites within reach are the last few
            for i_, a_i in seen[max(0, y - pr["reach"]): y]:
                if j - i_ <= pr["reach"]:
                    link[i_, j - i_ - 1, 2 * a_i + a_j] += 1
    assert int(link.max(initial=0)) < 2 ** 32
    return sites, link, n_obs


def decisive(cell, pr):
    """(cis, trans) if the link is decisive, else None."""
    cis, trans = int(cell[0]) + int(cell[3]), int(cell[1]) + int(cell[2])
    big = max(cis, trans)
    return (cis, trans) if big >= pr["min_links"] and big * PPM >= pr["min_frac_ppm"] * (cis + trans) else None


def phase(sites, link, **params):
    """(the 8 words of every site, [H, phased, blocks])."""
    pr = {**DEFAULTS, **params}
    check_params(pr)
    H = len(sites)
    parent, flip, how = list(range(H)), [0] * H, [(0, 0, 0)] * H
    for j in range(H):
        for d in range(1, pr["reach"] + 1):
            if j - d < 0 or sites[j - d][1] != sites[j][1]:
                continue
            won = decisive(link[j - d, d - 1], pr)
            if won:
                parent[j], flip[j], how[j] = j - d, int(won[1] > won[0]), (d, *won)
                break
    root, hap = [], []
    for j in range(H):                                   # plainly: walk up from every site
        at, h = j, 0
        while parent[at] != at:
            h ^= flip[at]
            at = parent[at]
        root.append(at)
        hap.append(h)
    size = [root.count(r) for r in range(H)] if H < 2000 else np.bincount(np.asarray(root, np.int64), minlength=H).tolist()
    out = [(sites[j][0], root[j], sites[root[j]][2], hap[j], (PHASED if size[root[j]] >= 2 else 0) | (ROOT if root[j] == j else 0), *how[j]) for j in range(H)]
    return out, [H, sum(1 for w in out if w[W_FLAGS] & PHASED), sum(1 for r in range(H) if size[r] >= 2)]


def run(records, ref_len, called, skip=None, **params):
    """(sites, link, words, the four sums)"""
    sites, link, n_obs = links(records, ref_len, called, skip, **params)
    words, sums = phase(sites, link, **params)
    return sites, link, words, sums + [n_obs]


def longest(words, called):
    return max((called[w[W_CALL]][1] - w[W_ROOT_POS] + 1 for w in words if w[W_FLAGS] & PHASED), default=0)


def summary_line(words, sums, called):
    return f"Phase: {sums[1]} of {sums[0]} het SNVs phased in {sums[2]} blocks (longest {longest(words, called)} bases, {sums[3]} observations)"


PS_HEAD = "##FORMAT=<ID=PS,Number=1,Type=Integer,"


def phased_vcf(text, called, words):
    """The file of --vcf-phase from the file without it: the SNV line of a PHASED site is rewritten, the header gains a line."""
    by_place = {(called[w[W_CALL]][0], called[w[W_CALL]][1]): (called[w[W_CALL]], w) for w in words if w[W_FLAGS] & PHASED}
    names, out = [], []
    for line in text.split("\n"):
        if line.startswith("##contig=<ID="):
            names.append(line[len("##contig=<ID="):].rsplit(",length=", 1)[0])
        f = line.split("\t")
        if line.startswith("#") or len(f) < 10 or len(f[3]) != 1 or any(len(x) != 1 for x in f[4].split(",")):
            out.append(line)
            if line.startswith("##FORMAT=<ID=PL,"):
                out.append(None)                         # the PS line: its text is the writer's, only its place and head are the rule's
            continue
        hit = by_place.get((names.index(f[0]), int(f[1]) - 1))
        if hit is None:
            out.append(line)
            continue
        c, w = hit
        alleles = [c[2]] + [x for x in sorted({c[4], c[5]}) if x != c[2]]
        g = [alleles.index(c[4]), alleles.index(c[5])]
        h1, h2 = (g[1], g[0]) if w[W_HAP] else (g[0], g[1])
        sample = f[9].split(":")
        assert sample[0] == f"{min(g)}/{max(g)}"
        sample[0] = f"{h1}|{h2}"
        out.append("\t".join(f[:8] + [f[8] + ":PS", ":".join(sample) + f":{w[W_ROOT_POS] + 1}"]))
    return out


def same_as_phased(text, want):
    """text is the lines of phased_vcf(...), the PS header line matched by its head."""
    got = text.split("\n")
    assert len(got) == len(want), (len(got), len(want))
    for a, b in zip(got, want):
        assert (a.startswith(PS_HEAD) and a.endswith(">")) if b is None else a == b, (a, b)


def unphased_vcf(text):
    """By text alone: a|b back into min/max, :PS, its value and the header line dropped."""
    out = []
    for line in text.split("\n"):
        if line.startswith(PS_HEAD):
            continue
        f = line.split("\t")
        if not line.startswith("#") and len(f) >= 10 and f[8].endswith(":PS"):
            f[8] = f[8][: -len(":PS")]
            sample = f[9].split(":")[:-1]
            a, b = (int(x) for x in re.fullmatch(r"(\d)\|(\d)", sample[0]).groups())
            sample[0] = f"{min(a, b)}/{max(a, b)}"
            f[9] = ":".join(sample)
            line = "\t".join(f)
        out.append(line)
    return "\n".join(out)
