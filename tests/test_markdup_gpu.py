"""bmd_ends / bmd_mark / bmd_mark_sort_deflate on the MI355X against the rule in plain Python (tests/markdup_rule.py), the fused
call against the BGZF rule of tests/bgzf_rule.py over the Python-sorted marked stream, and the product tools' --markdup files
against the oracle-backed tools' (whose marking is host/markdup.h): the rule is exact, so the files are equal.
Every tool run has its own time limit; nothing is retried."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bgzf_rule as R
import markdup_rule as M
from test_bamsort import offsets_of, pair_of, sort_reference
from test_sam_golden import TOOLS

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 63, 64, 65, 257, 1025, 70001]
OPS = "MIDNSHP=X"


@pytest.fixture(scope="module")
def m():
    from bucket_map_amd import markdup
    c = markdup.Marker(0)
    yield c
    c.close()


# ---- records with real CIGAR, sequence and quality bytes ----
def rec(ref, pos, flag=0, cigar="", qual=b"", name=b"r", tags=b""):
    ops = []
    num = ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            ops.append(int(num) << 4 | OPS.index(ch))
            num = ""
    return rec_ops(ref, pos, flag, ops, qual, name, tags)


def rec_ops(ref, pos, flag, ops, qual, name=b"r", tags=b""):
    l_seq = len(qual)
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name) + 1, 30, 4680, len(ops), flag, l_seq, -1, -1, 0) + name + b"\0"
    body += struct.pack(f"<{len(ops)}I", *ops) + bytes((17 * k + 1) & 255 for k in range((l_seq + 1) // 2)) + bytes(qual) + tags
    return struct.pack("<I", len(body)) + body


CIGARS = ["10M", "5S10M", "3H2S10M", "10M4S", "10M2S3H", "4M2D4M", "4M100N6M", "5=1X4=", "4M2I4M", "3M1P2I5M", "", "6S", "2H5S"]
QUALS = np.array([0, 14, 15, 40, 93, 255], np.uint8)


def random_records(n, seed, spread=40):
    """n records: pairs (adjacent, one name) and single records on a few positions of two references, so that keys collide."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        qual = lambda: QUALS[rng.integers(0, 6, int(rng.integers(0, 40)))].tobytes()
        place = lambda: (int(rng.integers(0, 2)), int(rng.integers(0, spread)), 16 * int(rng.integers(0, 2)))
        name = b"q%d" % len(out)
        if n - len(out) >= 2 and rng.random() < 0.5:
            for first in (0x40, 0x80):
                ref, pos, rev = place()
                pos %= 3                                  # pairs on few places: their two-ended keys have to collide too
                flag = 1 | first | rev | (4 if rng.random() < 0.05 else 0)
                out.append(rec(ref, pos, flag, CIGARS[int(rng.integers(0, len(CIGARS)))], qual(), name, rng.bytes(int(rng.integers(0, 9)))))
        else:
            ref, pos, rev = place()
            flag = rev | int(rng.choice([0, 0, 0, 0, 0, 4, 0x100, 0x800, 1 | 0x40, 1 | 0x80]))
            if rng.random() < 0.03:
                ref, pos = -1, -1
            out.append(rec(ref, pos, flag, CIGARS[int(rng.integers(0, len(CIGARS)))], qual(), name, rng.bytes(int(rng.integers(0, 9)))))
    return out


def check_ends(m, recs):
    want = M.ends(recs)
    end, score, kind = m.ends(b"".join(recs), offsets_of(recs))
    assert kind.tolist() == want[2]
    assert score.tolist() == want[1]
    assert end.tolist() == want[0]
    return want


def check_mark(m, end, score, kind):
    want_dup, want_counts = M.mark(end, score, kind)
    dup, counts = m.mark(end, score, kind)
    assert dup.tolist() == want_dup and counts == want_counts
    assert m.n_passes == M.passes(end, score, kind)
    return want_dup, want_counts


def check_records(m, recs, fused=True):
    dup, counts = check_mark(m, *check_ends(m, recs))
    if fused:
        marked = M.marked(recs)[0]
        perm, stream, so = sort_reference(marked)
        got, got_perm, got_so, got_dup, got_counts = m.mark_sort_deflate(b"".join(recs), offsets_of(recs))
        assert got_dup.tolist() == dup and got_counts == counts
        assert got_perm.tolist() == perm and got_so.tolist() == so
        assert got == (R.deflate(stream)[0] if recs else b"")
    return dup, counts


@pytest.mark.parametrize("n", SIZES)
def test_sizes(m, n):
    recs = random_records(n, 100 + n, spread=40 if n < 5000 else 4000)
    dup, counts = check_records(m, recs, fused=n <= 1025)
    if n >= 63:
        assert counts[0] and counts[1] and counts[3] and (counts[2] or n < 257) and 0 in M.ends(recs)[2]


def test_fused_call_of_many_records_sets_exactly_the_flags(m):
    """70 001 records: the blocks inflate to the Python-sorted stream with the rule's flags set."""
    import gzip
    recs = random_records(70001, 7, spread=4000)
    marked, dup, counts = M.marked(recs)
    got, perm, so, got_dup, got_counts = m.mark_sort_deflate(b"".join(recs), offsets_of(recs))
    want_perm, stream, want_so = sort_reference(marked)
    assert got_dup.tolist() == dup and got_counts == counts and sum(dup) > 100
    assert perm.tolist() == want_perm and so.tolist() == want_so
    assert gzip.decompress(got) == stream
    assert m.ms_ends > 0 and m.ms_mark > 0 and m.ms_deflate > 0 and m.ms_gather > 0


# ---- field edges ----
def edge_records():
    out = []
    for k in range(64):                                  # lengths over every residue mod 16, l_seq 0, 1, odd, even
        out.append(rec(0, 100 + k % 3, 0, "3S%dM" % (k + 1) if k % 2 else "", bytes([15 + k % 70]) * k, b"e%d" % k, b"t" * (k % 5)))
    out.append(rec(0, 50, 0, "4M", bytes([14, 15, 93, 255])))
    out.append(rec(0, 50, 0, "4M", bytes([14, 15, 93, 255])))
    out.append(rec(0, 50, 0, "6M", bytes([255] * 6)))
    out.append(rec(0, 50, 16, "", b"\x20\x20"))                      # no CIGAR: reflen 0, end5 = pos - 1
    out.append(rec(0, 51, 16, "6S", bytes([30] * 6)))               # all clips: both runs
    out.append(rec(0, 45, 16, "2H4S", bytes([30] * 4)))
    out.append(rec(0, 56, 0, "2H4S", bytes([30] * 4)))
    out.append(rec(0, 55, 0, "3H2S10M", bytes([30] * 12)))          # H before S; unclipped 50 like the 4M reads
    out.append(rec(0, 50, 0, "2M1D1N1=1X2I1P2M", bytes([30] * 8)))
    out.append(rec(0, 41, 16, "2M1D1N1=1X2I1P2M3S2H", bytes([31] * 11)))   # reflen 8, trailing 5: end5 = 53
    out.append(rec(0, 46, 16, "8M", bytes([29] * 8)))                # end5 = 53 too
    out.append(rec(0, 0, 0, "5S3M", bytes([40] * 8)))                # end5 = -5
    out.append(rec(0, 2, 0, "7S3M", bytes([41] * 10)))               # end5 = -5
    out.append(rec(0, -1, 0, "2H3M", bytes([41] * 3)))
    for name in (b"", b"a", b"x" * 253):                              # l_read_name 1, 2, 254
        out.append(rec(1, 7, 0x41, "5M", bytes([33] * 5), name))
        out.append(rec(1, 90, 0x91, "5M", bytes([33] * 5), name))
    out.append(rec(1, 7, 0x41, "5M", bytes([33] * 5), b"x" * 252 + b"y"))   # names equal but for the last byte: no pair
    out.append(rec(1, 90, 0x91, "5M", bytes([33] * 5), b"x" * 252 + b"z"))
    out.append(rec(1, 7, 0x81, "5M", bytes([34] * 5), b"swap"))      # 0x80 before 0x40: no pair
    out.append(rec(1, 90, 0x51, "5M", bytes([34] * 5), b"swap"))
    out.append(rec(1, 7, 0x41, "5M", bytes([35] * 5), b"three"))     # 0x40, 0x80, 0x40 with one name
    out.append(rec(1, 90, 0x91, "5M", bytes([35] * 5), b"three"))
    out.append(rec(1, 7, 0x41, "5M", bytes([36] * 5), b"three"))
    out.append(rec(1, 7, 0x41, "5M", bytes([35] * 5), b"half"))      # a pair whose mate is unmapped: a fragment and nothing
    out.append(rec(1, 7, 0x85, "", bytes([35] * 5), b"half"))
    out.append(rec(1, 7, 0x800, "2S3M", bytes([35] * 5), b"sup"))
    out.append(rec(1, 7, 0x100, "5M", bytes([35] * 5), b"sec"))
    out.append(rec_ops(1, 7, 0, [5 << 4 | 4, 900 << 4 | 3], bytes([35] * 5), b"placeholder"))
    out.append(rec_ops(1, 7, 0, [4 << 4 | 4, 900 << 4 | 3], bytes([35] * 5), b"no placeholder"))
    out.append(rec(-1, -1, 4, "", bytes([35] * 5), b"nowhere"))
    out.append(rec(2 ** 31 - 1, 2 ** 31 - 1, 0, "1M", b"\x30", b"far"))
    out.append(rec(3, 2 ** 31 - 1, 16, "2M", b"\x30\x30", b"beyond"))       # end5 = 2^31: not eligible
    out.append(rec(3, -(2 ** 31), 0, "1S1M", b"\x30\x30", b"below"))        # end5 = -2^31 - 1: not eligible
    return out


def test_field_edges(m):
    recs = edge_records()
    assert {len(r) % 16 for r in recs} == set(range(16))
    end, score, kind = M.ends(recs)
    by_name = {r[36: 36 + r[12] - 1]: k for r, k in zip(recs, kind)}
    assert by_name[b"placeholder"] == 0 and by_name[b"no placeholder"] == 1 and by_name[b"beyond"] == 0 and by_name[b"below"] == 0
    assert by_name[b"far"] == 1 and by_name[b"sup"] == 0 and by_name[b"swap"] == 1 and kind.count(2) == 4
    assert score[64] == score[65] == 108 and score[66] == 0
    dup, counts = check_records(m, recs)
    assert counts[2] == 6 and counts[3] > 5
    for size in (1, 7, 70):                              # the same records as the first, the middle and the last of a stream
        check_records(m, recs[:size], fused=False)
        check_records(m, recs[-size:], fused=False)


def test_one_long_record_between_short_ones(m):
    rng = np.random.default_rng(9)
    ops = [(1 + k % 3) << 4 | (7, 8, 0, 1, 2)[k % 5] for k in range(59994)]
    ops = [2 << 4 | 5, 3 << 4 | 4, *ops, 4 << 4 | 4, 1 << 4 | 5, 7 << 4 | 4, 9 << 4 | 5]
    assert len(ops) == 60000
    qual = rng.integers(0, 94, 200001).astype(np.uint8)
    qual[::1000] = 255
    short = random_records(300, 12)
    for flag in (0, 16):
        long = rec_ops(1, 1000, flag, ops, qual.tobytes(), b"long", b"NMi" + bytes(4))
        recs = short[:150] + [long] + short[150:] + [long]
        end, score, kind = check_ends(m, recs)
        assert score[150] > 2 ** 22 and kind[150] == 1
        dup, counts = check_mark(m, end, score, kind)
        assert dup[150] == 0 and dup[-1] == 1
    pair = [rec_ops(1, 5, 0x41, ops, qual.tobytes(), b"lp"), rec_ops(1, 900, 0x91, ops, qual.tobytes(), b"lp")]
    end, score, kind = check_ends(m, short[:10] + pair + short[10:20] + pair)
    assert kind[10:12] == [2, 3] and score[10] + score[11] > 2 ** 24
    dup, _ = check_mark(m, end, score, kind)
    assert dup[10:12] == [0, 0] and dup[-2:] == [1, 1]


# ---- marking patterns, on descriptors ----
def E(ref, end5, reverse=0):
    return ref << 33 | (end5 + 2 ** 31) << 1 | reverse


def units(pairs, frags):
    """Descriptors from [(E1, E2, score1, score2)] and [(E, score)], interleaved: a pair, a fragment, a pair ..."""
    end, score, kind = [], [], []
    for k in range(max(len(pairs), len(frags))):
        if k < len(pairs):
            end += pairs[k][:2]
            score += pairs[k][2:]
            kind += [2, 3]
        if k < len(frags):
            end.append(frags[k][0])
            score.append(frags[k][1])
            kind.append(1)
        if k % 7 == 0:
            end.append(0), score.append(k), kind.append(0)
    return end, score, kind


@pytest.mark.parametrize("n", [65, 257, 1025, 5000])
@pytest.mark.parametrize("name", ["one key", "distinct", "top byte", "strand bit", "high scores", "tied scores", "frag on first end",
                                  "frag on second end", "equal ends"])
def test_marking_patterns(m, name, n):
    rng = np.random.default_rng(n)
    a, b = E(1, 100), E(1, 300, 1)
    if name == "one key":
        pairs = [(a, b, int(rng.integers(0, 50)), int(rng.integers(0, 50))) if k % 2 else (b, a, int(rng.integers(0, 50)), 3) for k in range(n)]
        frags = [(E(2, 5), int(rng.integers(0, 9))) for _ in range(n)]
    elif name == "distinct":
        pairs = [(E(1, 10 * k), E(1, 10 * k + 5, 1), 7, 7) for k in range(n)]
        frags = [(E(2, 3 * k), 7) for k in range(n)]
    elif name == "top byte":
        pairs = [(E(int(rng.integers(0, 4)) << 22, 100), b, 5, k % 3) for k in range(n)]
        frags = [(E(int(rng.integers(0, 4)) << 22, 100), k % 3) for k in range(n)]
    elif name == "strand bit":
        pairs = [(E(1, 100, int(rng.integers(0, 2))), E(1, 300, int(rng.integers(0, 2))), 5, k % 3) for k in range(n)]
        frags = [(E(4, 100, int(rng.integers(0, 2))), k % 3) for k in range(n)]
    elif name == "high scores":
        pairs = [(a, b, int(rng.integers(0, 4)) << 33 | 9, int(rng.integers(0, 4)) << 33 | 9) for _ in range(n)]
        frags = [(E(2, 5), int(rng.integers(0, 4)) << 40) for _ in range(n)]
    elif name == "tied scores":
        pairs = [(a, b, 20, 22) if k % 2 else (a, b, 22, 20) for k in range(n)]
        frags = [(E(2, 5 + k % 2), 42) for k in range(n)]
    elif name == "frag on first end":
        pairs = [(E(1, 10 * k), E(1, 10 * k + 5, 1), 7, 7) for k in range(n)]
        frags = [(E(1, 10 * int(rng.integers(0, 2 * n))), 1000) for _ in range(n)]
    elif name == "frag on second end":
        pairs = [(E(1, 10 * k), E(1, 10 * k + 5, 1), 7, 7) for k in range(n)]
        frags = [(E(1, 10 * int(rng.integers(0, 2 * n)) + 5, 1), 1000) for _ in range(n)]
    else:
        pairs = [(E(1, k % 5), E(1, k % 5), k % 4, 1) for k in range(n)]
        frags = [(E(1, k % 10), 99) for k in range(n)]
    end, score, kind = units(pairs, frags)
    dup, counts = check_mark(m, end, score, kind)
    assert counts[:2] == [n, n]
    if name == "one key":
        assert counts[2] == 2 * (n - 1) and counts[3] == n - 1
    if name == "distinct":
        assert counts[2:] == [0, 0] and m.n_passes == M.passes(end, score, kind) > 0
    if name == "tied scores":
        assert dup[:2] == [0, 0] and counts[2] == 2 * (n - 1) and counts[3] == n - 2
    if name.startswith("frag on"):
        assert counts[2] == 0 and 0 < counts[3] < n
    if name == "equal ends":
        assert counts[2] == 2 * (n - 5) and counts[3] == n - 5


def test_mark_on_concatenated_descriptors(m):
    recs = random_records(3001, 21)
    cuts = [0, 1000, 1002, 3001]
    assert all(M.ends(recs)[2][c - 1] != 2 for c in cuts[1:-1]), "a cut between mates"
    parts = [m.ends(b"".join(recs[a:b]), offsets_of(recs[a:b])) for a, b in zip(cuts, cuts[1:])]
    end, score, kind = (np.concatenate([p[k] for p in parts]) for k in range(3))
    whole = check_ends(m, recs)
    assert (end.tolist(), score.tolist(), kind.tolist()) == whole
    dup, counts = m.mark(end, score, kind)
    assert (dup.tolist(), counts) == M.mark(*whole)


# ---- a context used again ----
def test_small_after_large_and_a_refusal_between(m):
    from bucket_map_amd import markdup
    check_records(m, random_records(20001, 31, spread=1000), fused=False)
    small = random_records(70, 32)
    bad = offsets_of(small)
    bad[5] += 1
    for call in (m.ends, m.mark_sort_deflate):
        with pytest.raises(markdup.BmdError) as e:
            call(b"".join(small), bad)
        assert e.value.code == markdup.BMD_ERR_ARG
    with pytest.raises(markdup.BmdError) as e:
        m.mark([0, 0], [0, 0], [3, 2])
    assert e.value.code == markdup.BMD_ERR_ARG
    check_records(m, small)


def test_large_after_small_on_a_fresh_context():
    from bucket_map_amd import markdup
    fresh = markdup.Marker(0)
    try:
        check_records(fresh, random_records(70, 32))
        check_records(fresh, random_records(20001, 31, spread=1000), fused=False)
        assert [x.tolist() for x in fresh.ends(b"", [0])] == [[], [], []]
        assert fresh.mark([], [], [])[1] == [0, 0, 0, 0]
        got = fresh.mark_sort_deflate(b"", [0])
        assert (got[0], got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4]) == (b"", [], [0], [], [0, 0, 0, 0])
    finally:
        fresh.close()


# ---- the tools ----
def run(exe, d, args, out, extra=(), env=None, limit=120):
    r = subprocess.run([exe, *args, "-o", out, *extra], cwd=str(d), capture_output=True, text=True, timeout=limit,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return r.stderr


@pytest.fixture(scope="module")
def jobs(tmp_path_factory):
    from test_markdup import markdup_jobs
    return markdup_jobs(tmp_path_factory)


@pytest.mark.parametrize("k", [0, 1])
def test_gpu_tool_writes_the_oracle_tools_marked_files(jobs, k):
    from test_markdup import parse_counts
    name, which, d, args, extra = jobs[k]
    err = run(TOOLS[(which, "oracle")], d, args, f"{name}.go.bam", [*extra, "--markdup"])
    want, want_counts = pair_of(d, f"{name}.go"), parse_counts(err)
    assert want_counts[0] > 0
    err = run(TOOLS[(which, "gpu")], d, args, f"{name}.g.bam", [*extra, "--markdup"])
    assert "in 1 run(s)" in err and parse_counts(err) == want_counts
    assert pair_of(d, f"{name}.g") == want
    run(TOOLS[(which, "gpu")], d, args, f"{name}.gg.bam", [*extra, "--markdup", "--gpus", "0,0"])
    assert pair_of(d, f"{name}.gg") == want
    err = run(TOOLS[(which, "gpu")], d, args, f"{name}.gr.bam", [*extra, "--markdup"], env=dict(BM_SORT_RUN_BYTES="2000"))
    assert "in 1 run(s)" not in err and parse_counts(err) == want_counts
    assert pair_of(d, f"{name}.gr") == want
