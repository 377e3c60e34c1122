"""Mate rescue without a GPU: the surface of bmv_rescue, the window and the job rule restated in Python (verify.rescue_window,
verify.select_rescue; host/pair_rescue.h is the C++ restatement) against hand-worked cases, and the tools' --rescue through the
oracle-backed tool, whose verifier takes alignment_verifier::rescue's default (plan on the host, align every view in full)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_pair import ARGS, BASES, PLAIN_TOOL, TOOL, _revcomp, make_paired_fixture, records, ref_len, run_tool

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_header_binding_and_python_surface():
    from bucket_map_amd import verify
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmv.h")).read(), flags=re.S)
    L = verify.lib()
    for name in ("bmv_rescue", "bmv_rescued", "bmv_last_rescue_stats"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), f"include/bmv.h does not declare {name}"
        assert name in verify.SYMBOLS and hasattr(L, name)
    decl = re.search(r"bmv_rescue\s*\((.*?)\)", text, flags=re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "ctx", "reads", "n_read_bytes", "anchor_text_start", "anchor_text_len", "anchor_text_rc", "anchor_query_len", "anchor_end",
        "contig_start", "contig_end", "query_start", "query_len", "max_edits", "n", "min_frag", "max_frag"]
    for fn in ("rescue", "rescue_stats"):
        assert callable(getattr(verify.Verifier, fn))
    assert callable(verify.rescue_window) and callable(verify.select_rescue)
    assert L.bmv_rescue(None, None, 0, None, None, None, None, None, None, None, None, None, None, 0, 1, 1000) == 1
    assert b"bmv_rescue" in L.bmv_last_error()
    assert L.bmv_rescued(None, None, None, None, None, None, None) == 1 and L.bmv_last_rescue_stats(None, None, None, None) == 1


# ---- the window and the job rule, by hand ----
# anchor forward: view (1000, 165), end 155, 150 bases: Ra = 1155, La = 1005
FWD = dict(anchor_text_start=1000, anchor_text_len=165, anchor_text_rc=0, anchor_query_len=150, anchor_end=155)
# anchor reverse: view (5000, 165), end 160, 150 bases: La = 5000 + 165 - 160 = 5005, Ra = 5155
REV = dict(anchor_text_start=5000, anchor_text_len=165, anchor_text_rc=1, anchor_query_len=150, anchor_end=160)


def test_rescue_window_by_hand():
    from bucket_map_amd.verify import rescue_window as w
    # forward anchor, mate of 150 within 15, 300..800: x_lo = max(1005, 1155 - 150, 1005 + 300 - 150) = 1155,
    # x_hi = 1005 + 800 - 150 = 1655, we = 1655 + 150 + 15
    assert w(**FWD, contig_start=0, contig_end=100_000, query_len=150, max_edits=15, min_frag=300, max_frag=800) == (1155, 665, 1)
    # reverse anchor, mate of 100 within 10: z_lo = 5155 + 100 - 800 = 4455, z_hi = min(5105, 5155, 5155 + 100 - 300) = 4955,
    # ws = 4455 - 100 - 10
    assert w(**REV, contig_start=0, contig_end=100_000, query_len=100, max_edits=10, min_frag=300, max_frag=800) == (4345, 610, 0)
    # max_edits beyond the query's length counts as the length: k = 100
    assert w(**REV, contig_start=0, contig_end=100_000, query_len=100, max_edits=4000, min_frag=300, max_frag=800) == (4255, 700, 0)
    # cut at the contig's right and left border
    assert w(**FWD, contig_start=0, contig_end=1500, query_len=150, max_edits=15, min_frag=300, max_frag=800) == (1155, 345, 1)
    assert w(**REV, contig_start=4400, contig_end=100_000, query_len=100, max_edits=10, min_frag=300, max_frag=800) == (4400, 555, 0)
    # ... and cut to nothing: the text_start is still ws
    assert w(**FWD, contig_start=0, contig_end=1100, query_len=150, max_edits=15, min_frag=300, max_frag=800) == (1155, 0, 1)
    assert w(**REV, contig_start=5000, contig_end=100_000, query_len=100, max_edits=10, min_frag=300, max_frag=800) == (5000, 0, 0)
    # min_frag = max_frag = 500: one admissible left end, 1005 + 500 - 150, and m + k columns behind it
    assert w(**FWD, contig_start=0, contig_end=100_000, query_len=150, max_edits=15, min_frag=500, max_frag=500) == (1355, 165, 1)
    assert w(**REV, contig_start=0, contig_end=100_000, query_len=150, max_edits=15, min_frag=500, max_frag=500) == (4640, 165, 0)
    # a negative x_lo: the anchor's estimated left end lies before the genome (view (0, 60), end 50: Ra = 50, La = -100)
    near = dict(anchor_text_start=0, anchor_text_len=60, anchor_text_rc=0, anchor_query_len=150, anchor_end=50)
    assert w(**near, contig_start=0, contig_end=5000, query_len=150, max_edits=15, min_frag=1, max_frag=1000) == (0, 915, 1)
    # ... and a negative z_lo - m - k (La = 100, Ra = 250: z_lo = -600, z_hi = min(250, 250, 399))
    near = dict(anchor_text_start=100, anchor_text_len=165, anchor_text_rc=1, anchor_query_len=150, anchor_end=165)
    assert w(**near, contig_start=0, contig_end=5000, query_len=150, max_edits=15, min_frag=1, max_frag=1000) == (0, 250, 0)


def test_select_rescue_by_hand():
    from bucket_map_amd.verify import BEYOND, rescue_bound, select_rescue
    assert rescue_bound(0.1, 150) == 15 and rescue_bound(0.1, 99) == 9 and rescue_bound(0.0, 150) == 0
    # a proper pair gets nothing
    assert select_rescue(1, [0, 0], [150, 150], 0.1)["jobs"] == [False, False]
    # one mate without a winner: the other anchors, and the bound is the QUERY's
    got = select_rescue(0, [3, BEYOND], [150, 100], 0.1)
    assert got == {"jobs": [True, False], "max_edits": [10, 15], "keep": None}
    # an anchor beyond the rate does not anchor
    assert select_rescue(0, [16, 15], [150, 150], 0.1)["jobs"] == [False, True]
    # what comes back: within bound and proper counts; the smaller sum wins, a tie goes to job 0
    both = lambda e, pr: select_rescue(0, [3, 2], [150, 150], 0.1, e, pr)["keep"]        # noqa: E731
    assert both([5, 4], [1, 1]) == 1 and both([4, 5], [1, 1]) == 0 and both([4, 4], [1, 1]) == 1
    assert both([4, 5], [0, 1]) == 1 and both([BEYOND, BEYOND], [0, 0]) is None and both([4, BEYOND], [1, 0]) == 0
    # a result where there was no job is not looked at
    assert select_rescue(0, [3, BEYOND], [150, 150], 0.1, [BEYOND, 0], [0, 1])["keep"] is None


# ---- the tool ----
N_LOST, READ = 14, 150


def make_rescue_fixture(d, seed=23):
    """chrA: 40 kbp of random bases, chrB: 6 kbp.  Pairs of 150-base reads from fragments of 350 .. 700 bases of chrA; ONE mate
    of each carries qualities of '!' throughout, so no k-mer of it passes the filter and it has NO candidate; it carries 0 .. 6
    substitutions (within 0.1 x 150 edits).  Pairs alternate in which mate is lost and in which is the forward read.  The last
    two pairs: one whose lost mate carries 40 substitutions (beyond the rate), one whose lost mate lies 3 000 bases away (beyond
    the range).  Returns per pair (lost mate 0 / 1, 1-based POS of mate 1, of mate 2, rescuable?)."""
    rng = np.random.default_rng(seed)
    a = BASES[rng.integers(0, 4, 40_000)]
    b = BASES[rng.integers(0, 4, 6_000)]
    with open(d / "g.fa", "w") as f:
        f.write(f">chrA\n{bytes(a).decode()}\n>chrB\n{bytes(b).decode()}\n")
    truth = []
    with open(d / "lost.fastq", "w") as f:
        for p in range(N_LOST + 2):
            frag = int(rng.integers(350, 701))
            left = int(rng.integers(1_000, 38_000))
            right = left + frag - READ if p != N_LOST + 1 else left + 3_000
            fwd, rev = np.array(a[left: left + READ]), np.array(a[right: right + READ])
            lost, flip = p % 2, (p // 2) % 2                   # flip: mate 1 is the reverse read
            damaged = rev if lost != flip else fwd             # the lost mate, on the forward strand
            n_sub = 40 if p == N_LOST else int(rng.integers(0, 7))
            for at in rng.choice(READ, n_sub, replace=False):
                damaged[at] = BASES[(int(np.searchsorted(BASES, damaged[at])) + 1 + int(rng.integers(0, 3))) % 4]
            mates = [bytes(fwd), _revcomp(rev)]
            pos = [left + 1, right + 1]
            if flip:
                mates, pos = mates[::-1], pos[::-1]
            quals = ["I" * READ, "I" * READ]
            quals[lost] = "!" * READ
            truth.append((lost, pos[0], pos[1], p < N_LOST))
            f.write(f"@r{p}/1\n{mates[0].decode()}\n+\n{quals[0]}\n@r{p}/2\n{mates[1].decode()}\n+\n{quals[1]}\n")
    return truth


@pytest.fixture(scope="module")
def lost(tmp_path_factory):
    d = tmp_path_factory.mktemp("rescue")
    return d, make_rescue_fixture(d)


def check_rescued(recs, truth):
    """The records of lost.fastq under --rescue against the truth: every rescuable pair has both records, the lost mate's with
    XR:i:1 at the true POS, both with 0x2, mutual PNEXT and the right TLEN; the other pairs are what --paired makes of them."""
    by_name = {}
    for r in recs:
        by_name.setdefault(r[0], []).append(r)
    n_xr = 0
    for p, (lost_mate, pos1, pos2, rescuable) in enumerate(truth):
        got = by_name.get(f"r{p}", [])
        if not rescuable:
            assert len(got) == 1 and int(got[0][1]) & 0x8 and not int(got[0][1]) & 0x2 and "XR:i:1" not in got[0], (p, got)
            continue
        assert len(got) == 2, (p, got)
        m1, m2 = got
        assert int(m1[1]) & 0x40 and int(m2[1]) & 0x80
        for m, mate, pos, mate_pos in ((m1, m2, pos1, pos2), (m2, m1, pos2, pos1)):
            flag = int(m[1])
            assert flag & 0x3 == 0x3 and not flag & 0x8, (p, m[:9])
            assert bool(flag & 0x20) == bool(int(mate[1]) & 0x10)
            assert m[2] == "chrA" and int(m[3]) == pos and m[6] == "=" and int(m[7]) == mate_pos, (p, m[:9])
        assert bool(int(m1[1]) & 0x10) != bool(int(m2[1]) & 0x10)
        lo, hi = min(pos1, pos2), max(pos1 + ref_len(m1[5]), pos2 + ref_len(m2[5]))
        assert int(m1[8]) == (hi - lo if pos1 < pos2 else lo - hi) and int(m2[8]) == -int(m1[8])
        rescued, anchor = (m1, m2) if lost_mate == 0 else (m2, m1)
        assert rescued[-1] == "XR:i:1" and rescued[-2] == "X0:i:1" and "XR:i:1" not in anchor, (p, rescued[11:], anchor[11:])
        assert rescued[4] == anchor[4] == "60", "the rescued mate carries its anchor's MAPQ"
        assert any(t.startswith("NM:i:") and int(t[5:]) <= 6 for t in rescued[11:])
        n_xr += 1
    assert n_xr >= N_LOST
    assert sum("XR:i:1" in r for r in recs) == n_xr


def test_tool_rescues_the_mate_without_a_candidate(lost):
    d, truth = lost
    # the precondition: under --paired the lost mate of every pair has no record, and its partner says so
    run_tool(TOOL, d, "lost.fastq", "paired.sam", "--paired")
    paired = records(d / "paired.sam")
    assert [r[0] for r in paired] == [f"r{p}" for p in range(N_LOST + 2)]
    assert all(int(r[1]) & 0x8 and not int(r[1]) & 0x2 for r in paired)
    run_tool(TOOL, d, "lost.fastq", "rescue.sam", "--rescue")
    check_rescued(records(d / "rescue.sam"), truth)
    # --rescue-rate alone implies the rest; blocks of any size are cut between pairs
    run_tool(TOOL, d, "lost.fastq", "rate.sam", "--rescue-rate", "0.1", block="2")
    assert open(d / "rate.sam").read() == open(d / "rescue.sam").read()
    # a rate that admits no edit rescues only the mates without one
    run_tool(TOOL, d, "lost.fastq", "exact.sam", "--rescue-rate", "0")
    exact = records(d / "exact.sam")
    assert 0 < sum("XR:i:1" in r for r in exact) < N_LOST
    assert all("NM:i:0" in r for r in exact if "XR:i:1" in r)
    # --max-edit-rate applies to a rescued mate as to any winner: its record goes, and its anchor says 0x8 again
    run_tool(TOOL, d, "lost.fastq", "bounded.sam", "--rescue", "--max-edit-rate", "0.02")
    bounded = records(d / "bounded.sam")
    assert 0 < sum("XR:i:1" in r for r in bounded) < N_LOST
    for r in bounded:
        assert any(t.startswith("NM:i:") and int(t[5:]) <= 3 for t in r[11:])
        assert (int(r[1]) & 0x2 != 0) == (int(r[1]) & 0x8 == 0) == (sum(x[0] == r[0] for x in bounded) == 2)
    # a range no fragment falls into rescues nothing
    run_tool(TOOL, d, "lost.fastq", "narrow.sam", "--rescue", "--frag-range", "1,100")
    assert open(d / "narrow.sam").read() == open(d / "paired.sam").read()


def test_tool_leaves_proper_pairs_alone(tmp_path):
    """Already-proper pairs: --rescue writes the bytes --paired writes."""
    make_paired_fixture(tmp_path)
    frag = ["--frag-range", "300,800"]
    run_tool(TOOL, tmp_path, "pairs.fastq", "paired.sam", *frag)
    run_tool(TOOL, tmp_path, "pairs.fastq", "rescue.sam", *frag, "--rescue")
    assert open(tmp_path / "rescue.sam").read() == open(tmp_path / "paired.sam").read()
    assert len(records(tmp_path / "rescue.sam")) == 48


def test_tool_refusals(lost):
    d, _ = lost
    for bad in (["--rescue-rate", "x"], ["--rescue-rate", "-0.5"], ["--rescue-rate", "2"]):
        r = run_tool(TOOL, d, "lost.fastq", "never.sam", *bad, ok=False)
        assert "Value parse failed for --rescue-rate" in r.stderr and not os.path.exists(d / "never.sam")
    for flag in (["--rescue"], ["--rescue-rate", "0.1"]):
        r = run_tool(PLAIN_TOOL, d, "lost.fastq", "never2.sam", *flag, ok=False)
        assert r.returncode == 255 and "belongs to bucketmap_align" in r.stderr and not os.path.exists(d / "never2.sam")
