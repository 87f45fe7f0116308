"""Where the host entry points cut a batch into uploads: make_runs / rebase of cbird_amd/csrc/cbh_runs.h, compiled alone
with the host compiler (tests/cpp/staging_runs.cpp, no library behind it) against a restatement of the rule and against
the rule's invariants.  The GPU tests only see that a chunked call's results are right, not where the cuts fall."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("staging_runs") / "staging_runs")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "cbird_amd", "csrc"), "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "staging_runs.cpp")])
    return out


def runs_of(off, end, budget, max_m):
    """the rule: a run starts with one image and takes the next while it has fewer than max_m and still spans <= budget"""
    runs, i0 = [], 0
    while i0 < len(off):
        m, lo, hi = 1, off[i0], end[i0]
        while i0 + m < len(off) and m < max_m:
            lo2, hi2 = min(lo, off[i0 + m]), max(hi, end[i0 + m])
            if hi2 - lo2 > budget:
                break
            m, lo, hi = m + 1, lo2, hi2
        runs.append((i0, m, lo, hi))
        i0 += m
    return runs


def program_runs(exe, cases):
    """[(i0, m, lo, hi, rel)] per case, from one run of the program"""
    text = "".join(f"{len(off)} {budget} {max_m}\n" + " ".join(f"{a} {b}" for a, b in zip(off, end)) + "\n"
                   for off, end, budget, max_m in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    got = []
    for ln in lines:
        runs = []
        for part in filter(None, (p.strip() for p in ln.split("|"))):
            v = [int(x) for x in part.split()]
            runs.append((v[0], v[1], v[2], v[3], v[4:]))
        got.append(runs)
    return got


def check(case, got):
    off, end, budget, max_m = case
    n = len(off)
    assert [r[:4] for r in got] == runs_of(off, end, budget, max_m)
    at = 0
    for i0, m, lo, hi, rel in got:
        assert i0 == at and m >= 1  # the runs partition [0, n) in order
        at += m
        assert lo == min(off[i0: i0 + m]) and hi == max(end[i0: i0 + m])
        assert m <= max_m
        assert hi - lo <= budget or m == 1
        if at < n and m < max_m:  # maximal: the next image would not have fitted
            assert max(hi, end[at]) - min(lo, off[at]) > budget
        assert rel == [o - lo for o in off[i0: i0 + m]]
    assert at == n


def image(off, size):
    return off, off + size


def make_case(images, budget, max_m):
    return [o for o, _ in images], [e for _, e in images], budget, max_m


def test_named_cases(exe):
    cases = {
        "none": make_case([], 100, 4),
        "one": make_case([image(7, 50)], 100, 4),
        "one_over_budget": make_case([image(7, 500)], 100, 4),
        # a large image between two small ones: three runs, the middle one over budget
        "large_between": make_case([image(0, 10), image(10, 500), image(510, 10)], 100, 1 << 20),
        "span_equals_budget": make_case([image(0, 40), image(40, 60)], 100, 1 << 20),
        "span_one_more": make_case([image(0, 40), image(40, 61)], 100, 1 << 20),
        # offsets that decrease: lo moves, and the span counts from the lowest offset to the highest end
        "descending": make_case([image(300, 30), image(200, 30), image(100, 30), image(0, 30)], 250, 1 << 20),
        "descending_then_far": make_case([image(90, 10), image(50, 10), image(0, 10), image(1000, 10), image(960, 10)], 100,
                                         1 << 20),
        # the cap before the budget
        "cap_1": make_case([image(10 * i, 10) for i in range(5)], 1 << 30, 1),
        "cap_4": make_case([image(10 * i, 10) for i in range(10)], 1 << 30, 4),
        "cap_32768": make_case([image(2 * i, 2) for i in range(40000)], 1 << 30, 32768),
        "offsets_past_2_32": make_case([image((1 << 33) + 100 * i, 100) for i in range(6)], 250, 1 << 20),
    }
    got = dict(zip(cases, program_runs(exe, list(cases.values()))))
    for name, case in cases.items():
        check(case, got[name])
    shape = {name: [(r[0], r[1]) for r in runs] for name, runs in got.items()}
    assert shape["none"] == [] and shape["one"] == [(0, 1)] and shape["one_over_budget"] == [(0, 1)]
    assert shape["large_between"] == [(0, 1), (1, 1), (2, 1)] and got["large_between"][1][3] - got["large_between"][1][2] == 500
    assert shape["span_equals_budget"] == [(0, 2)] and shape["span_one_more"] == [(0, 1), (1, 1)]
    assert shape["descending"] == [(0, 3), (3, 1)] and got["descending"][0][2:4] == (100, 330)
    assert shape["descending_then_far"] == [(0, 3), (3, 2)] and got["descending_then_far"][1][4] == [40, 0]
    assert shape["cap_1"] == [(i, 1) for i in range(5)]
    assert shape["cap_4"] == [(0, 4), (4, 4), (8, 2)]
    assert shape["cap_32768"] == [(0, 32768), (32768, 40000 - 32768)]
    assert shape["offsets_past_2_32"] == [(0, 2), (2, 2), (4, 2)]


def test_random_cases(exe):
    rng = np.random.default_rng(20240607)
    cases = []
    for _ in range(400):
        n = int(rng.integers(1, 41))
        budget = int(rng.integers(1, 400))
        sizes = rng.integers(1, int(rng.choice([20, 150, 600])), n)
        if rng.random() < 0.5:  # packed one after the other, or anywhere (overlaps and decreasing offsets included)
            offs = np.concatenate([[0], np.cumsum(sizes[:-1] + rng.integers(0, 8, n - 1))]) + int(rng.integers(0, 1000))
        else:
            offs = rng.integers(0, int(rng.choice([200, 2000])), n)
        images = [image(int(o), int(s)) for o, s in zip(offs, sizes)]
        cases.append(make_case(images, budget, int(rng.choice([1, 2, 4, 7, 32768]))))
    got = program_runs(exe, cases)
    for case, runs in zip(cases, got):
        check(case, runs)
    assert sum(len(r) > 1 for r in got) > 300 and sum(any(m > 1 for _, m, *_ in r) for r in got) > 200
