"""The indel normalisation pass without a GPU: a plain-Python restatement of bmv_leftalign's rule (include/bmv.h) that
tests/test_leftalign_gpu.py compares the device against, the hand-worked cases on both strands, a second, independent
formulation held against it (single one-column moves on a string of column ops), the contract's invariants, the ABI surface,
the tools' option, host/left_align.h as a sanitized stand-alone program, and `bucketmap_align --affine --left-align` through
the oracle-backed tool, whose verifier takes alignment_verifier::left_align's default (host/left_align.h)."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_annotate import D, I, M, rank, restate
from test_realign import COMP, TOOLS, check_affine_records, sam_records

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def restate_leftalign(window, rc, query, begin, cigar):
    """bmv_leftalign's outputs for one alignment, and what its stats count: a dict of begin, cigar ((op, length) pairs, the
    aligner's orientation), changed, dropped, merges and compared.  window: the text window as it lies in the genome; query:
    the read as sequenced; begin and cigar as the aligner gave them."""
    if not cigar:
        return dict(begin=begin, cigar=[], changed=0, dropped=0, merges=0, compared=0)
    W = [rank(c) for c in window]
    Qf = [rank(c) for c in (reversed(query) if rc else query)]       # ranks along the forward strand; nothing is complemented
    entries = list(reversed(cigar)) if rc else list(cigar)
    ref_len = sum(n for op, n in entries if op != I)
    pos = len(W) - begin - ref_len if rc else begin
    p, q, stack = pos, 0, []
    dropped = merges = compared = moved = 0

    def append_m(n):
        if n and stack and stack[-1][0] == M:
            stack[-1][1] += n
        elif n:
            stack.append([M, n])

    for g, L in entries:
        if g == M:
            append_m(L)
            p, q = p + L, q + L
            continue
        after = (p + (L if g == D else 0), q + (L if g == I else 0))
        pend, keep = 0, True
        while True:
            if not stack:                                        # (1)
                if g == D:
                    pos, dropped, keep = pos + L, dropped + L, False
                break
            top, k = stack[-1]
            if top == M:                                         # (2)
                s = 0
                while s < k:
                    compared += 1
                    t = s + 1
                    if (W[p - t] != W[p - t + L]) if g == D else (Qf[q - t] != Qf[q - t + L]):
                        break
                    s += 1
                p, q, pend = p - s, q - s, pend + s
                stack[-1][1] = k - s
                if s < k:
                    break
                stack.pop()
            elif top == g:                                       # (3)
                stack.pop()
                L += k
                if g == D:
                    p -= k
                else:
                    q -= k
                merges += 1
            else:                                                # (4)
                break
        if keep:
            stack.append([g, L])
        append_m(pend)
        moved += pend
        p, q = after
    if stack and stack[-1][0] == D:
        dropped += stack.pop()[1]
    out = [tuple(e) for e in stack]
    return dict(begin=len(W) - pos - (ref_len - dropped) if rc else pos, cigar=out[::-1] if rc else out,
                changed=int(moved > 0 or dropped > 0), dropped=dropped, merges=merges, compared=compared)


def by_single_moves(window, rc, query, begin, cigar):
    """The same by another formulation, with no stack and no lengths: the forward-strand path as a string of column ops.  A
    maximal run of I or of D columns whose left neighbour is an M column may swap places with that column when the base that
    leaves the gap's far end equals the one that enters at its near end; runs that touch ARE one run.  The leftmost run that
    can move moves one column, until none can (leftmost first: a run that waits for its left neighbour to settle sees the
    neighbour's final place, as the walk does); then the D columns at either end go.  Returns begin, cigar and dropped."""
    if not cigar:
        return dict(begin=begin, cigar=[], dropped=0)
    W = [rank(c) for c in window]
    Qf = [rank(c) for c in (reversed(query) if rc else query)]
    entries = list(reversed(cigar)) if rc else list(cigar)
    ref_len = sum(n for op, n in entries if op != I)
    pos = len(W) - begin - ref_len if rc else begin
    cols = [op for op, n in entries for _ in range(n)]
    while True:
        p, q, i, moved = pos, 0, 0, False
        while i < len(cols):
            if cols[i] == M:
                p, q, i = p + 1, q + 1, i + 1
                continue
            g, j = cols[i], i
            while j < len(cols) and cols[j] == g:
                j += 1
            L = j - i
            if i > 0 and cols[i - 1] == M and ((W[p - 1] == W[p - 1 + L]) if g == D else (Qf[q - 1] == Qf[q - 1 + L])):
                cols[i - 1], cols[j - 1] = g, M
                moved = True
                break
            p, q, i = p + (L if g == D else 0), q + (L if g == I else 0), j
        if not moved:
            break
    dropped = 0
    while cols and cols[0] == D:
        cols.pop(0)
        pos, dropped = pos + 1, dropped + 1
    while cols and cols[-1] == D:
        cols.pop()
        dropped += 1
    out = []
    for op in cols:
        if out and out[-1][0] == op:
            out[-1][1] += 1
        else:
            out.append([op, 1])
    out = [tuple(e) for e in out]
    return dict(begin=len(W) - pos - (ref_len - dropped) if rc else pos, cigar=out[::-1] if rc else out, dropped=dropped)


def parse(text):
    return [("MID".index(op), int(n)) for n, op in re.findall(r"(\d+)([MID])", text)]


def check_invariants(window, rc, query, begin, cigar, got, what=""):
    """What include/bmv.h says follows from the rule, for one alignment and its result."""
    ops = got["cigar"]
    assert sum(n for op, n in ops if op != D) == len(query), f"{what}: M + I lengths are not query_len"
    assert got["begin"] + sum(n for op, n in ops if op != I) <= len(window), f"{what}: the result leaves its window"
    assert all(x[0] != y[0] for x, y in zip(ops, ops[1:])), f"{what}: adjacent entries share an op"
    assert not ops or (ops[0][0] != D and ops[-1][0] != D), f"{what}: the result begins or ends with D"
    assert all(n > 0 for _, n in ops) and len(ops) <= len(cigar) + sum(op != M for op, _ in cigar), f"{what}: too many entries"
    assert got["changed"] == int(got["begin"] != begin or ops != list(cigar)), f"{what}: changed"
    nm_in, nm_out = restate(window, rc, query, begin, cigar)[3], restate(window, rc, query, got["begin"], ops)[3]
    assert nm_out == nm_in - got["dropped"], f"{what}: NM {nm_in} -> {nm_out} with {got['dropped']} dropped"
    again = restate_leftalign(window, rc, query, got["begin"], ops)
    assert (again["begin"], again["cigar"], again["changed"], again["dropped"], again["merges"]) == (got["begin"], ops, 0, 0, 0), \
        f"{what}: the pass is not idempotent"


# ------------------------------------------------------------------------------------------------ hand-worked cases

HAND = [  # window, query, given, result, pos of the result, dropped, merges
    (b"ACGTAAAAAAGTCC", b"ACGTAAAAGTCC", "8M2D4M", "4M2D8M", 0, 0, 0),
    (b"GGCAGCAGCAGTT", b"GGCAGCAGCAGCAGTT", "11M3I2M", "1M3I12M", 0, 0, 0),
    (b"CGTAAAAAAAAGC", b"CGTAAAAAAGC", "4M1D2M1D5M", "3M2D8M", 0, 0, 1),
    (b"AAAAACGT", b"AAACGT", "2M2D4M", "6M", 2, 2, 0),
    (b"AAAAGG", b"AAAAAGG", "4M1I2M", "1I6M", 0, 0, 0),
    (b"CCAAAAGG", b"CCTAAGG", "2M1I2D4M", "2M1I2D4M", 0, 0, 0),
    (b"GATATATC", b"GATATC", "5M2D1M", "1M2D5M", 0, 0, 0),
    (b"GACATATC", b"GACATC", "5M2D1M", "3M2D3M", 0, 0, 0),
]


@pytest.mark.parametrize("case", HAND, ids=[str(k + 1) for k in range(len(HAND))])
def test_hand_worked_cases_on_both_strands(case):
    """The table of include/bmv.h's rule.  On the reverse strand the read is the reverse complement, the entries come
    reversed and begin counts from the window's other end; the forward view, and so the event's place, is the same."""
    from bucket_map_amd import verify
    window, query, given, result, pos, dropped, merges = case
    given, result = parse(given), parse(result)
    ref = sum(n for op, n in result if op != I)
    for f in (restate_leftalign, by_single_moves):
        got = f(window, 0, query, 0, given)
        assert (got["begin"], got["cigar"], got["dropped"]) == (pos, result, dropped), f.__name__
        got = f(window, 1, query.translate(COMP)[::-1], 0, given[::-1])
        assert (got["begin"], got["cigar"], got["dropped"]) == (len(window) - pos - ref, result[::-1], dropped), f.__name__
    for rc, q, cg in ((0, query, given), (1, query.translate(COMP)[::-1], given[::-1])):
        got = restate_leftalign(window, rc, q, 0, cg)
        assert got["merges"] == merges and got["changed"] == int(result != given or pos != 0)
        check_invariants(window, rc, q, 0, cg, got)
        mine = verify.left_align(window, q, rc, 0, [(n << 4) | op for op, n in cg])      # the ABI users' copy of the rule
        assert [(e & 15, e >> 4) for e in mine.pop("cigar")] == got["cigar"]
        assert mine == {k: v for k, v in got.items() if k != "cigar"}


def test_an_empty_cigar_and_odd_letters():
    assert restate_leftalign(b"ACGT", 1, b"ACG", 2, []) == dict(begin=2, cigar=[], changed=0, dropped=0, merges=0, compared=0)
    # ranks decide: a, N and R are A; y is C
    got = restate_leftalign(b"CGTAnaRAAAGC", 0, b"cgtAAAAAgc", 0, parse("8M2D2M"))
    assert got["cigar"] == parse("3M2D7M") and got["compared"] == 6
    got = restate_leftalign(b"GGCAGCAGTT", 0, b"GGCAGyaGCAGTT", 0, parse("8M3I2M"))
    assert got["cigar"] == parse("1M3I9M")


def random_case(rng, letters=b"AC"):
    """A valid alignment with a random path over a small alphabet, where most gaps can move."""
    cigar, last = [], None
    for _ in range(int(rng.integers(1, 8))):
        op = int(rng.choice([o for o in (M, I, D) if o != last]))
        cigar.append((op, int(rng.integers(1, 12 if op == M else 5))))
        last = op
    begin = int(rng.integers(0, 4))
    window = bytes(rng.choice(list(letters), begin + sum(n for op, n in cigar if op != I) + int(rng.integers(0, 4))).astype(np.uint8))
    query = bytes(rng.choice(list(letters), sum(n for op, n in cigar if op != D)).astype(np.uint8))
    return window, int(rng.integers(0, 2)), query, begin, cigar


def test_the_two_formulations_agree_and_the_invariants_hold():
    """2 000 random paths over a two-letter alphabet and 500 over three letters: begin, entries and dropped agree between
    the walk and the single moves; every invariant holds, idempotence included; the ABI users' copy agrees too."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(91)
    changed = merged = dropped = 0
    for k in range(2500):
        window, rc, query, begin, cigar = random_case(rng, b"AC" if k < 2000 else b"ACG")
        got = restate_leftalign(window, rc, query, begin, cigar)
        other = by_single_moves(window, rc, query, begin, cigar)
        assert {x: got[x] for x in other} == other, (window, rc, query, begin, cigar)
        check_invariants(window, rc, query, begin, cigar, got, str((window, rc, query, begin, cigar)))
        if k % 5 == 0:
            mine = verify.left_align(window, query, rc, begin, [(n << 4) | op for op, n in cigar])
            assert [(e & 15, e >> 4) for e in mine.pop("cigar")] == got["cigar"] and mine == {x: v for x, v in got.items() if x != "cigar"}
        changed, merged, dropped = changed + got["changed"], merged + (got["merges"] > 0), dropped + (got["dropped"] > 0)
    assert changed > 1500 and merged >= 30 and dropped >= 100, (changed, merged, dropped)
    assert changed, "hardly any path changed: the comparison shows little"


# ------------------------------------------------------------------------------------------------ ABI and options

NAMES = ("bmv_leftalign", "bmv_leftaligned", "bmv_last_leftalign_stats")


def test_header_and_binding_agree_on_the_new_symbols():
    from bucket_map_amd import verify
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmv.h")).read(), flags=re.S)
    L = verify.lib()
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
        n_args = len(re.search(rf"\b{name}\s*\((.*?)\)", text, flags=re.S).group(1).split(","))
        assert n_args == len(verify.SYMBOLS[name][1]), name
    assert callable(verify.Verifier.leftalign) and callable(verify.Verifier.leftalign_stats) and callable(verify.left_align)


def test_entry_points_fail_cleanly_without_a_context():
    from bucket_map_amd import verify
    L = verify.lib()
    total = C.c_uint64()
    assert L.bmv_leftalign(None, None, 0, None, None, None, None, None, None, None, None, 0, C.byref(total)) == 1
    assert b"bmv_leftalign" in L.bmv_last_error()
    assert L.bmv_leftaligned(None, None, None, None, None, None) == 1
    assert b"bmv_leftaligned" in L.bmv_last_error()
    assert L.bmv_last_leftalign_stats(None, None, None, None, None, None) == 1
    assert b"bmv_last_leftalign_stats" in L.bmv_last_error()


def test_the_option_belongs_to_bucketmap_align(tmp_path):
    def run(tool, *extra):
        return subprocess.run([TOOLS[tool], "-i", "idx", *extra], cwd=str(tmp_path), capture_output=True, text=True)
    for ok in (["--left-align"], ["--affine", "--left-align"], ["--left-align", "--clip", "--best"]):
        r = run("bucketmap_align", *ok)                          # parsed; what fails next is the missing genome
        assert r.returncode != 0 and "Unknown option" not in r.stderr and "BM_GENOME_FILE is not found" in r.stderr, r.stderr
    r = run("bucketmap", "--left-align")
    assert r.returncode != 0 and "belongs to bucketmap_align" in r.stderr and "BM_GENOME_FILE" not in r.stderr, r.stderr


# ------------------------------------------------------------------------------------------------ the sanitized host restatement

def test_the_host_restatement_under_sanitizers(tmp_path):
    """tests/cpp/left_align_check.cpp, a program of its own around host/left_align.h, built with -fsanitize=address,undefined
    and run: the hand cases and 400 seeded random paths, clean, and every line it prints is what the restatement here gives."""
    exe = str(tmp_path / "left_align_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "left_align_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 2 * len(HAND) + 400
    for line in lines:
        window, query, rc, begin, given, _, out_begin, result, changed, dropped = line.split(" ")
        want = restate_leftalign(window.encode(), int(rc), query.encode(), int(begin), parse(given))
        assert (int(out_begin), parse(result), int(changed), int(dropped)) == (want["begin"], want["cigar"], want["changed"], want["dropped"]), line


# ------------------------------------------------------------------------------------------------ the oracle-backed tool

SITE_D, SITE_I, N_AWAY = 10_000, 25_000, 40           # (CAG) x 8 begins at SITE_D, A x 10 at SITE_I
ARGS = ["-i", "idx", "--genome", "g.fa", "--bucket-len", "4096", "-r", "150", "-f", "1", "-q", "reads.fastq"]


def make_site_job(d):
    """A 40-kbp record with (CAG) x 8 behind a T and A x 10 behind a C.  Fourteen reads of 150 bases over each site, every
    other one from the reverse strand: those over the first lack one CAG, those over the second carry two more A.  Forty
    reads elsewhere with 2 % substitutions."""
    rng = np.random.default_rng(111)
    bases = np.frombuffer(b"ACGT", np.uint8)
    g = bases[rng.integers(0, 4, 40_000)]
    g[SITE_D - 1: SITE_D + 25] = np.frombuffer(b"T" + b"CAG" * 8 + b"T", np.uint8)
    g[SITE_I - 1: SITE_I + 11] = np.frombuffer(b"C" + b"A" * 10 + b"G", np.uint8)
    with open(d / "g.fa", "w") as f:
        f.write(f">chrA\n{bytes(g).decode()}\n")
    with open(d / "reads.fastq", "w") as f:
        def put(name, s, k):
            s = bytes(s)
            if k % 2:
                s = s.translate(COMP)[::-1]
            f.write(f"@{name}\n{s.decode()}\n+\n{'I' * len(s)}\n")
        for k in range(14):
            p = SITE_D - 35 - 6 * k                              # the repeat lies 35 .. 113 bases into the read
            put(f"del{k}", np.concatenate([g[p: SITE_D + 6], g[SITE_D + 9: p + 153]]), k)
            p = SITE_I - 35 - 7 * k
            put(f"ins{k}", np.concatenate([g[p: SITE_I + 4], bases[[0, 0]], g[SITE_I + 4: p + 148]]), k)
        for k in range(N_AWAY):
            p = int(rng.integers(0, 40_000 - 150))
            while abs(p - SITE_D) < 400 or abs(p - SITE_I) < 400:
                p = int(rng.integers(0, 40_000 - 150))
            s = g[p: p + 150].copy()
            hit = rng.random(150) < 0.02
            s[hit] = bases[rng.integers(0, 4, int(hit.sum()))]
            put(f"away{k}", s, k)


@pytest.fixture(scope="module")
def site_job(tmp_path_factory):
    d = tmp_path_factory.mktemp("leftalign")
    make_site_job(d)
    return d


def _tool(d, out, *extra):
    env = dict(os.environ, BM_VERIFY_BLOCK_READS="17")
    r = subprocess.run([TOOLS["bucketmap_align"], *ARGS, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def gaps_of(f):
    """(op, 0-based forward coordinate, length) of every I and D entry of a record."""
    at, out = int(f[3]) - 1, []
    for n, op in re.findall(r"(\d+)([=XIDS])", f[5]):
        if op in "ID":
            out.append((op, at, int(n)))
        if op in "=XD":
            at += int(n)
    return out


def check_site_records(recs):
    """Every record over a site carries its gap at the one leftmost forward coordinate, on either strand."""
    over_d, over_i = [f for f in recs if f[0].startswith("del")], [f for f in recs if f[0].startswith("ins")]
    assert len(over_d) == len(over_i) == 14 and {int(f[1]) & 16 for f in over_d} == {int(f[1]) & 16 for f in over_i} == {0, 16}
    assert all(gaps_of(f) == [("D", SITE_D, 3)] for f in over_d), [(f[0], f[1], gaps_of(f)) for f in over_d]
    assert all(gaps_of(f) == [("I", SITE_I, 2)] for f in over_i), [(f[0], f[1], gaps_of(f)) for f in over_i]


def test_the_oracle_backed_tool_with_left_align(site_job):
    """--affine --left-align through alignment_verifier::left_align's default.  This test fails without the feature: the
    option does not exist there."""
    from test_annotate_gpu import _fasta, _fastq
    d = site_job
    _tool(d, "plain.sam")
    _tool(d, "ann.sam", "--annotate")
    _tool(d, "aff.sam", "--affine")
    _tool(d, "la.sam", "--affine", "--left-align")
    _tool(d, "la_only.sam", "--left-align")
    aff, la, la_only = sam_records(d / "aff.sam"), sam_records(d / "la.sam"), sam_records(d / "la_only.sam")
    key = lambda f: (f[0], f[1], f[2], f[4], f[9], f[10])
    assert [key(f) for f in aff] == [key(f) for f in la] == [key(f) for f in la_only] and len(la) >= 28 + N_AWAY * 3 // 4
    # without the pass the two strands disagree on where the events are
    assert len({tuple(gaps_of(f)) for f in aff if f[0].startswith("del")}) > 1
    assert len({tuple(gaps_of(f)) for f in aff if f[0].startswith("ins")}) > 1
    check_site_records(la)
    check_site_records(la_only)
    ref, reads = _fasta(d / "g.fa"), _fastq(d / "reads.fastq")
    check_affine_records(la, ref, reads)                         # NM and MD against the FASTA, AS:i recomputed
    assert all(len(f) == 13 for f in la_only) and not any(t.startswith("AS:") for f in la_only for t in f[11:])
    # nothing merged or dropped here, so AS:i is bmv_realign's score
    assert [[t for t in f[11:] if t.startswith("AS:")] for f in la] == [[t for t in f[11:] if t.startswith("AS:")] for f in aff]
    away = lambda recs: [f for f in recs if f[0].startswith("away")]
    assert away(la) == away(aff) and len(away(la)) >= N_AWAY * 3 // 4
    # without the option every byte is as before: the digests are those of the parent commit's tool on this job
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "leftalign_parent_sha256.json")))
    for name in ("plain.sam", "ann.sam", "aff.sam"):
        assert hashlib.sha256((d / name).read_bytes()).hexdigest() == want[name], name


def test_the_affine_score_of_written_entries_is_realigns_when_nothing_merges(site_job):
    """host/sam_tags.h's affine_score over the written entries equals bmv_realign's score whenever nothing merged or dropped:
    under other scores and a narrow band too, every record of --affine --left-align has the gap lengths and the AS:i of the
    --affine run, though half the records over the sites moved; NM, MD and AS:i hold against the FASTA."""
    from test_annotate_gpu import _fasta, _fastq
    d = site_job
    ref, reads = _fasta(d / "g.fa"), _fastq(d / "reads.fastq")
    extra = ["--affine-scores", "2,3,5,2", "--affine-band", "8"]
    _tool(d, "s_aff.sam", *extra)
    _tool(d, "s_la.sam", *extra, "--left-align")
    aff, la = sam_records(d / "s_aff.sam"), sam_records(d / "s_la.sam")
    tags = lambda recs: [(f[0], f[1], [t for t in f[11:] if t.startswith("AS:")]) for f in recs]
    assert tags(aff) == tags(la) and len(la) > 50
    assert all(sorted(x[2] for x in gaps_of(f)) == sorted(x[2] for x in gaps_of(g)) for f, g in zip(aff, la)), "a gap merged or was dropped"
    check_affine_records(la, ref, reads, (2, 3, 5, 2))
    check_site_records(la)
    assert sum(f[5] != g[5] for f, g in zip(aff, la)) >= 14, "hardly any record changed: the run shows little"
