"""Mate rescue on the GPU: bmv_rescue against its contract restated in Python -- verify.rescue_window for the view,
Verifier.align_long on that view for (d, end), the d <= k rule, and select_pairs' proper between the anchor and the rescued mate --
exactly, for every number of parts a job is cut into; the fallback for queries beyond 512 bases; what the call leaves alone; the
refusals; and the tool against the oracle-backed tool."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_best_gpu import _mutate, _reference, _revcomp
from test_pair import ARGS, records
from test_rescue import N_LOST, check_rescued, make_rescue_fixture

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GPU_TOOL = os.path.join(ROOT, "bucket-map_amd", "bucketmap_align")
ORACLE_TOOL = os.path.join(ROOT, "tests", "cpp", "bucketmap_align_oracle")
PARTS = (1, 2, 8, 64, None)                                    # None: the host's own choice
KEYS = ("text_start", "text_len", "text_rc", "edits", "end", "proper")
ODD = np.frombuffer(b"NRYKMacgtn", np.uint8)                   # N, IUPAC and lower case: all fold to a rank


FOLD = np.full(256, ord("A"), np.uint8)                       # the dna4 folding of include/bmf.h: every letter to A, C, G or T
for _letters, _to in (("CcYySsBb", "C"), ("GgKk", "G"), ("TtUu", "T")):
    FOLD[list(_letters.encode())] = ord(_to)


def walk(genome, start, n, rc):
    """the view [start, start + n) as the aligner walks it on strand rc, folded to A C G T"""
    view = FOLD[genome[start: start + n]]
    return _revcomp(view) if rc else view


def make_genome(rng, n):
    g = rng.choice(list(b"ACGT"), n).astype(np.uint8)
    at = rng.choice(n, n // 50, replace=False)
    g[at] = ODD[rng.integers(0, len(ODD), len(at))]
    return g


def spoil(rng, q):
    """a few letters of a read replaced by N / IUPAC / lower case"""
    q = np.array(q, np.uint8)
    if len(q) >= 20:
        at = rng.choice(len(q), len(q) // 40 + 1, replace=False)
        q[at] = ODD[rng.integers(0, len(ODD), len(at))]
    return q


class Jobs:
    def __init__(self):
        self.reads, self.at, self.rows = [], 0, []

    def add(self, query, anchor, contig, max_edits):
        """anchor: (text_start, text_len, text_rc, query_len, end); contig: (start, end)"""
        self.reads.append(np.asarray(query, np.uint8))
        self.rows.append((*anchor, *contig, self.at, len(query), max_edits))
        self.at += len(query)

    def add_view(self, query, start, n, rc, max_edits):
        """A job whose view is exactly [start, start + n) on strand rc under the range 1 .. 5 000: an anchor 100 bases beyond
        the view's near side, and the contig cut to the view (n <= 1 400, start >= 300)."""
        la = start - 200 if rc else start + n + 100
        self.add(query, (la - 5, 110, 0 if rc else 1, 100, 105), (start, start + n), max_edits)

    def args(self, count=None):
        rows = self.rows[:count]
        cols = list(zip(*rows)) if rows else [[]] * 10
        reads = np.concatenate(self.reads) if self.at else np.zeros(0, np.uint8)
        types = (np.uint64, np.uint32, np.uint8, np.uint32, np.uint32, np.uint64, np.uint64, np.uint64, np.uint32, np.uint32)
        return (reads, *(np.array(c, t) for c, t in zip(cols, types)))


def expected(v, args, lo, hi):
    """The contract: the Python-planned view, bmv_align_long on it, d <= k, select_pairs' proper."""
    from bucket_map_amd import verify
    reads, ats, atl, arc, aql, aen, c0, c1, qs, ql, me = args
    n = len(ats)
    view = [verify.rescue_window(ats[j], atl[j], arc[j], aql[j], aen[j], c0[j], c1[j], ql[j], me[j], lo, hi) for j in range(n)]
    out = {"text_start": np.array([w[0] for w in view], np.uint64), "text_len": np.array([w[1] for w in view], np.uint32),
           "text_rc": np.array([w[2] for w in view], np.uint8), "edits": np.full(n, verify.BEYOND, np.uint32),
           "end": np.zeros(n, np.uint32), "proper": np.zeros(n, np.uint8)}
    real = np.flatnonzero((out["text_len"] > 0) & (ql > 0))
    if len(real):
        _, d, end = _reference(v, (reads, out["text_start"][real], out["text_len"][real], out["text_rc"][real], qs[real], ql[real]))
        for j, dj, ej in zip(real, d, end):
            if dj > min(int(me[j]), int(ql[j])):
                continue
            out["edits"][j], out["end"][j] = dj, ej
            pair = verify.select_pairs([int(ats[j]), view[j][0]], [int(atl[j]), view[j][1]], [int(arc[j]), view[j][2]],
                                       [int(aql[j]), int(ql[j])], [0, int(dj)], [int(aen[j]), int(ej)], [0, 1, 2], lo, hi)
            out["proper"][j] = pair["proper"][0]
    return out


def check(v, monkeypatch, args, lo, hi, what, parts=PARTS, want=None):
    want = expected(v, args, lo, hi) if want is None else want
    for p in parts:
        if p is None:
            monkeypatch.delenv("BMV_RESCUE_PARTS", raising=False)
        else:
            monkeypatch.setenv("BMV_RESCUE_PARTS", str(p))
        got = v.rescue(*args, lo, hi)
        for key in KEYS:
            bad = np.flatnonzero(got[key] != want[key])
            assert bad.size == 0, f"{what}, parts {p}: {key} differs at jobs {bad[:8]}: got {got[key][bad[:8]]}, want {want[key][bad[:8]]}"
        stats = v.rescue_stats()
        assert p is None or stats["parts"] == p
        assert stats["parts"] in (1, 2, 4, 8, 16, 32, 64)
    monkeypatch.delenv("BMV_RESCUE_PARTS", raising=False)
    return want


@pytest.fixture(scope="module")
def ground():
    """A 60-kbp genome with odd letters, in which the 100 bases from 40 200 stand again at 40 900, and a verifier that holds it."""
    from bucket_map_amd import verify
    rng = np.random.default_rng(20251101)
    genome = make_genome(rng, 60_000)
    genome[40_000:41_300] = rng.choice(list(b"ACGT"), 1_300).astype(np.uint8)
    genome[40_900:41_000] = genome[40_200:40_300]
    v = verify.Verifier()
    v.load_genome(genome)
    return v, genome


def _planted(rng, genome, start, n, rc, m, edits):
    """a read of m bases out of the view [start, start + n) as walked on strand rc, with a few edits and odd letters"""
    walked = walk(genome, start, n, rc)
    if n >= m + 8:
        at = int(rng.integers(0, n - m - 7))
        q = _mutate(rng, walked[at: at + m + 8], edits / max(m, 1), 0.004, 0.004)[:m]
    else:
        q = _mutate(rng, walked, 0.02, 0, 0)[:m]
    if len(q) < m:
        q = np.concatenate([q, rng.choice(list(b"ACGT"), m - len(q)).astype(np.uint8)])
    return spoil(rng, q)


@pytest.mark.gpu
def test_query_lengths_view_lengths_and_bounds(ground, monkeypatch):
    """Every word count of the lane kernel at its borders, views around one and two fetches of 64 columns and one of 1 300, both
    strands; each under max_edits 0, d - 1, d and m, d taken from the reference."""
    v, genome = ground
    rng = np.random.default_rng(20251102)
    shapes = [(m, n, rc) for m in (1, 63, 64, 65, 129, 150, 300, 511, 512) for n in (63, 64, 65, 127, 128, 129, 1300) for rc in (0, 1)]
    probe, queries = Jobs(), []
    for x, (m, n, rc) in enumerate(shapes):
        start = 1_000 + 53 * x
        queries.append(_planted(rng, genome, start, n, rc, m, 3))
        probe.add_view(queries[-1], start, n, rc, m)
    d = expected(v, probe.args(), 1, 5000)["edits"].astype(np.int64)
    assert (d <= [s[0] for s in shapes]).all()
    jobs = Jobs()
    for x, (m, n, rc) in enumerate(shapes):
        for bound in (0, max(int(d[x]) - 1, 0), int(d[x]), m):
            jobs.add_view(queries[x], 1_000 + 53 * x, n, rc, bound)
    want = check(v, monkeypatch, jobs.args(), 1, 5000, "lengths and bounds")
    within = want["edits"] != 2 ** 32 - 1
    assert within.sum() > len(shapes) and (~within).sum() > len(shapes) // 2 and want["proper"].sum() > 20
    assert (want["text_len"].reshape(-1, 4)[:, 0] == [s[1] for s in shapes]).all(), "the views are not the shapes meant"


def _natural_jobs(rng, genome, count):
    """Jobs with windows as a tool would ask for them: an anchor somewhere, its mate sampled from a fragment of 200 .. 900 bases
    (sometimes from elsewhere), contigs that contain the window, cut it on either side, or miss it."""
    jobs = Jobs()
    for x in range(count):
        m, aql = int(rng.integers(30, 301)), int(rng.integers(50, 301))
        frag = int(rng.integers(max(m, aql) + 1, 900))
        left = int(rng.integers(3_000, 35_000))
        anchor_fwd = x % 2 == 0
        if anchor_fwd:                                         # the anchor at the fragment's left end, the mate reverse at its right
            a_l, q_l = left, left + frag - m
        else:
            a_l, q_l = left + frag - aql, left
        src = genome[q_l: q_l + m + 8] if x % 7 else genome[50_000: 50_000 + m + 8]
        q = _mutate(rng, src, 0.03, 0.005, 0.005)[:m]
        q = spoil(rng, q if anchor_fwd is False else _revcomp(_mutate(rng, genome[q_l: q_l + m], 0.03, 0, 0)))
        slack = int(rng.integers(0, 12))
        if anchor_fwd:
            anchor = (a_l - slack, aql + 2 * slack + 1, 0, aql, aql + slack)
        else:
            anchor = (a_l - slack, aql + 2 * slack + 1, 1, aql, aql + slack + 1)
        kind = x % 5
        contig = ((0, len(genome)), (left + 150, len(genome)), (0, left + frag - 60), (left - 2_000, left - 1_000), (0, len(genome)))[kind]
        jobs.add(q, anchor, contig, int(rng.integers(0, m // 5 + 2)) if x % 11 else 4_000_000_000)
    return jobs


@pytest.mark.gpu
def test_job_counts_strands_and_contig_cuts(ground, monkeypatch):
    """0, 1, 65 and 200 jobs with natural windows on both anchor strands, contigs that cut the view or leave nothing of it."""
    from bucket_map_amd import verify
    v, genome = ground
    jobs = _natural_jobs(np.random.default_rng(20251103), genome, 200)
    for count, lo, hi in ((200, 1, 1000), (65, 300, 600), (1, 1, 1000), (200, 500, 500)):
        want = check(v, monkeypatch, jobs.args(count), lo, hi, f"{count} jobs, range {lo}..{hi}")
        if count == 200 and lo == 1:
            assert want["proper"].sum() > 40 and (want["text_len"] == 0).sum() > 20 and (want["edits"] == verify.BEYOND).sum() > 40
    empty = v.rescue(*jobs.args(0), 1, 1000)
    assert all(len(empty[k]) == 0 for k in KEYS)
    # an empty query is beyond, whatever its view
    one = Jobs()
    one.add_view(np.zeros(0, np.uint8), 5_000, 300, 0, 5)
    one.add_view(genome[7_000:7_100], 7_000, 300, 0, 5)
    want = check(v, monkeypatch, one.args(), 1, 5000, "an empty query")
    assert want["edits"].tolist() == [verify.BEYOND, 0] and want["end"].tolist() == [0, 100]


@pytest.mark.gpu
def test_part_borders_and_ties(ground, monkeypatch):
    """A view of 1 280 columns is cut at 640 by 2 parts, at multiples of 160 by 8 and of 20 by 64: an exact placement ending one
    column before, at and one column behind the borders 160 and 640, on both strands, with and without edits to spare; and two
    equally good placements in different parts, of which the later column wins."""
    v, genome = ground
    jobs, ends = Jobs(), []
    for rc in (0, 1):
        start = 20_000 + 2_000 * rc
        walked = walk(genome, start, 1280, rc)
        for border in (160, 640):
            for end in (border - 1, border, border + 1):
                for k in (0, 5):
                    jobs.add_view(walked[end - 100: end], start, 1280, rc, k)
                    ends.append(end)
    want = check(v, monkeypatch, jobs.args(), 1, 5000, "part borders")
    assert want["edits"].tolist() == [0] * len(ends) and want["end"].tolist() == ends
    # the copy: ends 300 and 1 000 of the view from 40 000, both exact; then with one edit each
    ties = Jobs()
    q = genome[40_200:40_300]
    ties.add_view(q, 40_000, 1280, 0, 0)
    ties.add_view(q, 40_000, 1280, 0, 7)
    hurt = q.copy()
    hurt[50] = ord("A") if hurt[50] != ord("A") else ord("C")
    ties.add_view(hurt, 40_000, 1280, 0, 7)
    ties.add_view(_revcomp(q), 40_000, 1280, 1, 0)             # walked backwards: the ends are 1 280 - 200 and 1 280 - 900
    want = check(v, monkeypatch, ties.args(), 1, 5000, "ties")
    assert want["edits"].tolist() == [0, 0, 1, 0] and want["end"].tolist() == [1000, 1000, 1000, 1080]
    # a best placement that ends before the first admissible end: reported with its distance, not proper.  The anchor reverse
    # with La = 26 000, Ra = 26 100; a mate of 100 within 10 under 300 .. 600: z_lo = 25 600, the view begins at 25 490
    early = Jobs()
    early.add(genome[25_490:25_590], (25_995, 110, 1, 100, 105), (0, len(genome)), 10)
    early.add(genome[25_500:25_600], (25_995, 110, 1, 100, 105), (0, len(genome)), 10)
    want = check(v, monkeypatch, early.args(), 300, 600, "before the first admissible end")
    assert want["text_start"].tolist() == [25_490, 25_490] and want["edits"].tolist() == [0, 0]
    assert want["end"].tolist() == [100, 110] and want["proper"].tolist() == [0, 1]


def _read_results(v, n):
    from bucket_map_amd import verify
    L = verify.lib()
    score, begin, off = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint64)
    cigar = np.zeros(1 << 16, np.uint32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))            # noqa: E731
    assert L.bmv_results(v._h, p(score, C.c_int32), p(begin, C.c_uint32), p(off, C.c_uint64), p(cigar, C.c_uint32)) == 0
    ms, cells = C.c_float(), C.c_uint64()
    assert L.bmv_last_stats(v._h, C.byref(ms), C.byref(cells)) == 0
    return score, begin, off, cigar[: int(off[n])].copy(), cells.value


@pytest.mark.gpu
def test_long_query_fallback_and_what_the_call_leaves_alone(ground, monkeypatch):
    """A 513-base query is one word more than a lane holds: it is aligned in full on its planned view and meets the same contract;
    bmv_results, bmv_best and bmv_pairs return after the call what they returned before it."""
    from bucket_map_amd import verify
    v, genome = ground
    rng = np.random.default_rng(20251104)
    # something for bmv_results, bmv_best and bmv_pairs to hold
    reads = np.concatenate([genome[9_000:9_150], _revcomp(genome[9_400:9_550])])
    batch = (reads, np.array([8_990, 9_390], np.uint64), np.array([170, 170], np.uint32), np.array([0, 1], np.uint8),
             np.array([0, 150], np.uint64), np.array([150, 150], np.uint32))
    off = np.array([0, 1, 2], np.uint32)
    jobs = Jobs()
    for rc in (0, 1):
        for m in (513, 700, 150):
            start = 30_000 + 3_000 * rc
            walked = walk(genome, start, 1300, rc)
            q = _mutate(rng, walked[200: 200 + m + 8], 0.02, 0.003, 0.003)[:m]
            for bound in (0, 3, 60, m):
                jobs.add_view(q, start, 1300, rc, bound)
    jobs.add_view(genome[100:613], 12_000, 0, 0, 513)          # an empty view on the fallback's way
    want = expected(v, jobs.args(), 1, 5000)
    before = v.align_paired(*batch, off, np.array([7, 7], np.uint32), 1, 1000)
    assert before["proper"].tolist() == [1]
    results = _read_results(v, 2)
    check(v, monkeypatch, jobs.args(), 1, 5000, "the fallback", parts=(1, 8, None), want=want)
    assert (want["edits"] != verify.BEYOND).sum() >= 12 and (want["edits"] == verify.BEYOND).sum() >= 6
    after = _read_results(v, 2)
    for x, y in zip(results, after):
        assert np.array_equal(x, y), "bmv_results / bmv_last_stats changed across bmv_rescue"
    pairs = v._pairs(2)
    for key in ("pick", "proper", "s1", "s2", "winner"):
        assert np.array_equal(pairs[key], before[key]), f"bmv_pairs: {key} changed across bmv_rescue"
    L = verify.lib()
    winner, edits, end = np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))      # noqa: E731
    assert L.bmv_best(v._h, p(winner), p(edits), p(end)) == 0
    assert np.array_equal(winner, before["winner"]) and np.array_equal(edits, before["edits"]) and np.array_equal(end, before["end"])


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(ground, monkeypatch):
    from bucket_map_amd import verify
    v, genome = ground
    jobs = _natural_jobs(np.random.default_rng(20251105), genome, 12)
    args = jobs.args()
    good = v.rescue(*args, 1, 1000)
    names = ("reads", "anchor_text_start", "anchor_text_len", "anchor_text_rc", "anchor_query_len", "anchor_end", "contig_start",
             "contig_end", "query_start", "query_len", "max_edits")

    def refused(change, words, lo=1, hi=1000):
        bad = [a.copy() for a in args]
        for name, value in change.items():
            bad[names.index(name)][5] = value
        with pytest.raises(verify.BmvError) as e:
            v.rescue(*bad, lo, hi)
        assert e.value.code == 1 and all(w in str(e.value) for w in words), str(e.value)

    refused({}, ("min_frag", "job"), 900, 800)
    refused({"contig_start": 70_000, "contig_end": 60_000}, ("job 5", "contig"))
    refused({"contig_end": 60_001}, ("job 5", "contig"))
    refused({"anchor_end": int(args[2][5]) + 1}, ("job 5", "anchor_end"))
    refused({"anchor_text_start": 59_990}, ("job 5", "anchor", "genome"))
    refused({"anchor_text_start": 2 ** 62}, ("job 5", "anchor_text_start"))
    refused({"query_start": len(args[0]) - 3}, ("job 5", "query"))
    again = v.rescue(*args, 1, 1000)
    for key in KEYS:
        assert np.array_equal(good[key], again[key]), f"{key} differs after the refusals"


@pytest.mark.gpu
def test_tool_equals_the_oracle_backed_tool(tmp_path):
    """bucketmap_align --rescue writes, byte for byte, what the oracle-backed tool writes on the CPU test's files -- whose
    verifier plans on the host and aligns every view in full --; --gpus 0,0 writes the same bytes; with --clip the rescued mates
    go through the clipping pass with the other picks."""
    d = tmp_path
    truth = make_rescue_fixture(d)

    def tool(exe, out, *extra):
        env = dict(os.environ, BM_VERIFY_BLOCK_READS="6")
        r = subprocess.run([exe, *ARGS, "-q", "lost.fastq", "-o", out, *extra], cwd=str(d), capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr
        return (d / out).read_bytes(), r.stderr

    for name, extra in (("rescue", ["--rescue"]), ("rate", ["--rescue-rate", "0.02", "--frag-range", "200,900"]),
                        ("bounded", ["--rescue", "--max-edit-rate", "0.02"])):
        cpu, _ = tool(ORACLE_TOOL, f"cpu_{name}.sam", *extra)
        gpu, err = tool(GPU_TOOL, f"gpu_{name}.sam", *extra)
        assert "GPU mate rescue" in err
        assert gpu == cpu, extra
    check_rescued(records(d / "gpu_rescue.sam"), truth)
    two, _ = tool(GPU_TOOL, "gpu2.sam", "--rescue", "--gpus", "0,0")
    assert two == (d / "gpu_rescue.sam").read_bytes(), "--gpus 0,0 differs from --gpus 0"
    tool(GPU_TOOL, "clip.sam", "--rescue", "--clip")
    clip = records(d / "clip.sam")
    assert sum("XR:i:1" in r for r in clip) >= N_LOST and all(any(t.startswith("AS:i:") for t in r[11:]) for r in clip)
