"""host/lists_cells_rule.h: whether the lists vote counts cells of buckets first, decided once per index load from NB, S, F
and the length-weighted mean list length.  The header's lines as a program of their own (tests/cpp/lists_cells_check.cpp)
under ASan + UBSan; no GPU."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, S, F = 26413, 15, 6                  # the headline shape: k12 q9 S15 F6 on the Egu-like index


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lists_cells_check") / "lists_cells_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                        "-o", exe, os.path.join(ROOT, "tests", "cpp", "lists_cells_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def ask(*queries):
        """[(choice, lambda, p)] for queries (nb, S, F, density): the density is turned into the mean units the load sees"""
        args = []
        for nb, s, f, density in queries:
            args += [str(nb), str(s), str(f), repr((density * nb + 3.5) / 8.0)]      # (3.5 padding ids in the last unit)
        out = subprocess.run([exe] + args, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-3000:]
        return [(int(a), float(b), float(c)) for a, b, c in (line.split() for line in out.stdout.splitlines())]
    return ask


def poisson_tail(lam, t):
    return 1.0 - sum(math.exp(-lam) * lam ** i / math.factorial(i) for i in range(t))


def test_the_headline_takes_cells_of_eight(rule):
    (choice, lam, p), = rule((NB, S, F, 0.014))
    assert choice == 3
    assert lam == pytest.approx(15 * 8 * 0.014)
    assert p == pytest.approx(poisson_tail(lam, 10) * math.ceil(NB / 8), rel=1e-6) and 0.02 < p < 0.05


def test_denser_lists_take_cells_of_four_and_then_none(rule):
    (two, lam2, p2), (none, _, p3) = rule((NB, S, F, 0.02), (NB, S, F, 0.03))
    assert two == 2 and lam2 == pytest.approx(15 * 4 * 0.02) and p2 <= 0.05
    assert p2 == pytest.approx(poisson_tail(lam2, 10) * math.ceil(NB / 4), rel=1e-6)
    assert none == 0 and p3 > 0.05


def test_what_the_byte_fields_cannot_hold_stays_full_width(rule):
    """S = 32: a cell of 8 could sum to 256.  F > S: t < 1, every bucket qualifies without a hit."""
    for s, f in ((32, 6), (64, 26), (15, 16), (0, 0)):
        (choice, _, _), = rule((NB, s, f, 0.001))
        assert choice == 0, (s, f)
    (choice, _, _), = rule((NB, 31, 12, 0.001))
    assert choice == 3


def test_p_grows_with_the_density(rule):
    densities = [0.0, 1e-5, 1e-4, 0.001, 0.005, 0.01, 0.014, 0.02, 0.03, 0.05, 0.1, 0.3, 0.6, 1.0, 2.0]
    for s, f in ((15, 6), (15, 1), (31, 12), (1, 1)):
        got = rule(*[(NB, s, f, d) for d in densities])
        choices = [c for c, _, _ in got]
        for shift in (3, 2):
            # the p reported is that of the last form considered: cells of 8 where they are taken, else cells of 4
            ps = [p for c, _, p in got if (c == 3) == (shift == 3)]
            assert all(a <= b * (1 + 1e-12) for a, b in zip(ps, ps[1:])), (s, f, shift, ps)
        assert choices == sorted(choices, key=lambda c: {3: 0, 2: 1, 0: 2}[c]), (s, f, choices)      # 8, then 4, then none
        assert choices[0] == 3 and choices[-1] == 0
