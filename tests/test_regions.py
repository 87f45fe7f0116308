"""The launch plan of the callers that hash autocropped images and the packing of a chunk's resized images
(cbird_amd/csrc/cbh_regions.h), compiled alone with the host compiler (tests/cpp/regions.cpp, no library and no device
behind it) and compared with the rule restated here."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A, B, C, D = (0, 20, 160, 100), (30, 0, 130, 120), (0, 0, 160, 120), (8, 8, 150, 110)  # A < B, C < D lexicographically
# kept regions whose sizeLongestSide result is square, wide, tall, and rejected (one side truncates to 0)
SQUARE, WIDE, TALL, THIN = (10, 10, 110, 110), (0, 40, 200, 90), (40, 0, 90, 200), (0, 7, 1000, 8)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("regions") / "regions")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "cbird_amd", "csrc"), "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "regions.cpp")])
    return out


def ask(exe, commands):
    """the program's output lines for a list of command lines"""
    out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.split("\n")[:-1]


def rects_arg(seq):
    return f"{len(seq)} " + " ".join(" ".join(str(v) for v in r) for r in seq)


def parse_runs(line):
    """[(first, count, rect)] of 'n | first count l t r b | ...'"""
    parts = line.split("|")
    runs = [tuple(int(x) for x in p.split()) for p in parts[1:]]
    assert int(parts[0]) == len(runs)
    return [(r[0], r[1], r[2:]) for r in runs]


# ---- the rule, restated -----------------------------------------------------------------------------------------


def model_runs(seq):
    runs = []
    for i, r in enumerate(seq):
        if runs and runs[-1][2] == r:
            runs[-1] = (runs[-1][0], runs[-1][1] + 1, r)
        else:
            runs.append((i, 1, r))
    return runs


def model_plan(seq, mode_first):
    runs = model_runs(seq)
    if not mode_first or not seq:
        return runs
    count = {r: seq.count(r) for r in seq}
    mode = min(count, key=lambda r: (-count[r], r))  # the most frequent; of several the lexicographically smallest
    n_odd = len(seq) - count[mode]
    if not 1 + n_odd < len(runs):
        return runs
    return [(0, len(seq), mode)] + [(i, 1, r) for i, r in enumerate(seq) if r != mode]


def model_dims(w, h, size):
    aspect = np.float32(w) / np.float32(h)
    if w > h:
        return size, int(np.float32(size) / aspect)
    return int(aspect * np.float32(size)), size


def model_kept(rect, size):
    dw, dh = model_dims(rect[2] - rect[0], rect[3] - rect[1], size)
    return (0, 0) if dw <= 0 or dh <= 0 or dw > size or dh > size else (dw, dh)


def model_pack(plan, m, size):
    ws, hs, off, base, cur = [0] * m, [0] * m, [0] * m, [], 0
    for first, count, rect in plan:
        dw, dh = model_kept(rect, size)
        cur = (cur + 15) // 16 * 16
        base.append(cur)
        for t in range(count):
            ws[first + t], hs[first + t], off[first + t] = dw, dh, cur + t * dw * dh
        cur += count * dw * dh
    return cur, base, ws, hs, off


def check_plan(seq, plan, mode_first):
    m = len(seq)
    runs = model_runs(seq)
    covered = set()
    for first, count, rect in plan:
        assert count >= 1 and first + count <= m
        covered |= set(range(first, first + count))
    assert covered == set(range(m))  # every image is covered
    if plan == runs:
        for (f0, c0, r0), (f1, c1, r1) in zip(plan, plan[1:]):
            assert f1 == f0 + c0 and r0 != r1  # in order, and maximal: neighbours differ
        assert all(seq[i] == r for f, c, r in plan for i in range(f, f + c))
        return "runs"
    assert mode_first
    first, count, mode = plan[0]
    assert (first, count) == (0, m)  # the first entry spans the chunk ...
    odd = [i for i in range(m) if seq[i] != mode]
    assert [(f, c, r) for f, c, r in plan[1:]] == [(i, 1, seq[i]) for i in odd]  # ... each odd image once, ascending
    return "mode"


PLAN_CASES = [
    ([A], "runs"),
    ([A, A, A, A], "runs"),  # one run: mode-first must not trigger
    ([A, B, A], "mode"),
    ([A, A, B, B], "runs"),
    ([A, B, A, B], "mode"),  # a tie, and 1 + 2 < 4
    ([B, A, B, A], "mode"),
    ([A, B, C, A], "mode"),
    ([A, B, C, D], "runs"),
]


def test_named_plans(exe):
    seqs = [s for s, _ in PLAN_CASES]
    got = [parse_runs(ln) for ln in ask(exe, [f"plan 1 {rects_arg(s)}" for s in seqs])]
    plain = [parse_runs(ln) for ln in ask(exe, [f"plan 0 {rects_arg(s)}" for s in seqs])]
    only_runs = [parse_runs(ln) for ln in ask(exe, [f"runs {rects_arg(s)}" for s in seqs])]
    for (seq, kind), g, p, r in zip(PLAN_CASES, got, plain, only_runs):
        assert g == model_plan(seq, True), seq
        assert p == r == model_runs(seq), seq
        assert check_plan(seq, g, True) == kind, seq
        assert check_plan(seq, p, False) == "runs"
    by_seq = {tuple(s): g for (s, _), g in zip(PLAN_CASES, got)}
    assert by_seq[(A,)] == [(0, 1, A)]
    assert by_seq[(A, A, A, A)] == [(0, 4, A)]
    assert by_seq[(A, B, A)] == [(0, 3, A), (1, 1, B)]
    assert by_seq[(A, A, B, B)] == [(0, 2, A), (2, 2, B)]
    # A B A B: two of each, four runs, 1 + 2 < 4: mode-first, and the tie goes to the lexicographically smaller
    # rectangle whichever comes first in the chunk
    assert A < B
    assert by_seq[(A, B, A, B)] == [(0, 4, A), (1, 1, B), (3, 1, B)]
    assert by_seq[(B, A, B, A)] == [(0, 4, A), (0, 1, B), (2, 1, B)]
    assert by_seq[(A, B, C, A)] == [(0, 4, A), (1, 1, B), (2, 1, C)]
    assert by_seq[(A, B, C, D)] == [(i, 1, r) for i, r in enumerate((A, B, C, D))]  # 1 + 3 is not less than 4


def test_random_plans_equal_the_model(exe):
    rng = np.random.default_rng(300)
    seqs = [[(A, B, C)[int(k)] for k in rng.integers(0, 3, int(rng.integers(1, 13)))] for _ in range(300)]
    got = [parse_runs(ln) for ln in ask(exe, [f"plan 1 {rects_arg(s)}" for s in seqs])]
    plain = [parse_runs(ln) for ln in ask(exe, [f"plan 0 {rects_arg(s)}" for s in seqs])]
    kinds = set()
    for seq, g, p in zip(seqs, got, plain):
        assert g == model_plan(seq, True), seq
        assert p == model_runs(seq), seq
        kinds.add(check_plan(seq, g, True))
        check_plan(seq, p, False)
    assert kinds == {"runs", "mode"}  # both branches occur


def test_fill_whole(exe):
    assert ask(exe, ["whole 3 160 120", "whole 0 4 4"]) == ["0 0 160 120 0 0 160 120 0 0 160 120", ""]


def test_longest_side_dims(exe):
    """the pairs tests/test_prestage.py lists for the oracle, and the reject rule on kept regions"""
    cases = {(4000, 3000, 400): (400, 300), (3000, 4000, 400): (300, 400), (300, 500, 400): (240, 400),
             (500, 500, 400): (400, 400), (1000, 3, 400): (400, 1), (1000, 1, 400): (400, 0)}
    got = [tuple(int(x) for x in ln.split()) for ln in ask(exe, ["dims %d %d %d" % c for c in cases])]
    assert got == list(cases.values()) == [model_dims(*c) for c in cases]
    kept = [(r, s) for r in (SQUARE, WIDE, TALL, THIN, A, B, C, D, (0, 0, 1, 1000), (0, 0, 3, 1000)) for s in (32, 400)]
    got = [tuple(int(x) for x in ln.split()) for ln in ask(exe, ["kept %d %d %d %d %d" % (*r, s) for r, s in kept])]
    for (r, s), (ok, dw, dh) in zip(kept, got):
        assert (dw, dh) == model_kept(r, s) and ok == (dw != 0), (r, s)
    by = {k: g for k, g in zip(kept, got)}
    assert by[(SQUARE, 32)] == (1, 32, 32) and by[(WIDE, 400)] == (1, 400, 100) and by[(TALL, 400)] == (1, 100, 400)
    assert by[(THIN, 400)] == by[(THIN, 32)] == (0, 0, 0) and by[((0, 0, 1, 1000), 400)] == (0, 0, 0)


def test_packing_of_the_resized_images(exe):
    shapes = (SQUARE, WIDE, TALL, THIN)
    seqs = []
    for seq, _ in PLAN_CASES:  # the plans above, over every assignment of result shapes that keeps them distinct
        for rot in range(4):
            name = {A: shapes[rot], B: shapes[(rot + 1) % 4], C: shapes[(rot + 2) % 4], D: shapes[(rot + 3) % 4]}
            seqs.append([name[r] for r in seq])
    cases = [(mf, rs, s) for s in seqs for rs in (32, 400) for mf in (0, 1)]
    lines = ask(exe, [f"pack {mf} {rs} {rects_arg(s)}" for mf, rs, s in cases])
    rejected = modes = 0
    for (mf, rs, seq), ln in zip(cases, lines):
        m = len(seq)
        head, base, per = ln.split("|")
        used, base = int(head), [int(x) for x in base.split()]
        per = [int(x) for x in per.split()]
        ws, hs, off = per[0::3], per[1::3], per[2::3]
        plan = model_plan(seq, bool(mf))
        assert (used, base, ws, hs, off) == model_pack(plan, m, rs), (mf, rs, seq)
        modes += mf and plan != model_runs(seq)
        assert all(b % 16 == 0 for b in base)  # every run starts on a multiple of 16
        assert used <= 2 * m * (rs * rs + 16)  # the size d_res is allocated with
        # what the launches of the plan write, in order, does not overlap ...
        end = 0
        for (first, count, rect), b in zip(plan, base):
            dw, dh = model_kept(rect, rs)
            assert b >= end
            end = b + count * dw * dh
        assert end == used
        # ... and neither do the final slots of distinct images, each the image's own kept region resized
        slots = []
        for i in range(m):
            assert (ws[i], hs[i]) == model_kept(seq[i], rs)
            if ws[i] == 0:
                assert hs[i] == 0  # rejected images report 0 x 0
                rejected += 1
                continue
            assert off[i] + ws[i] * hs[i] <= used
            slots.append((off[i], off[i] + ws[i] * hs[i]))
        slots.sort()
        assert all(a[1] <= b[0] for a, b in zip(slots, slots[1:])), (mf, rs, seq)
    assert rejected > 0 and modes > 0
