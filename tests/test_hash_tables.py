"""The image hash's host-only tables and sizing rules (cbird_amd/csrc/dcthash_tables.h), compiled alone with the host
compiler (tests/cpp/hash_tables.cpp, no library and no device behind it): the INTER_AREA tables against the oracle's,
and the conditions that the kernels read from the derived tables without checking them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hash_tables") / "hash_tables")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "cbird_amd", "csrc"), "-o", out,
                           os.path.join(ROOT, "tests", "cpp", "hash_tables.cpp")])
    return out


def ask(exe, commands):
    """the program's output lines for a list of command lines"""
    out = subprocess.run([exe], input="\n".join(commands) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.split("\n")[:-1]


def f32(words):
    return np.array([int(x, 16) for x in words], np.uint32).view(np.float32)


def parse_tab(words):
    """(si, di, alpha) of 'si di alphabits' triples"""
    return (np.array(words[0::3], np.int64), np.array(words[1::3], np.int64), f32(words[2::3]))


def orc_tab(orc, ssize):
    """(si, di, alpha, first[33]) of the oracle's computeResizeAreaTab(ssize, 32)"""
    si, di, al = np.zeros(ssize + 70, np.int32), np.zeros(ssize + 70, np.int32), np.zeros(ssize + 70, np.float32)
    f = orc.L.orc_resize_area_tab
    f.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    f.restype = C.c_int
    k = f(ssize, 32, si.ctypes.data, di.ctypes.data, al.ctypes.data)
    assert 0 < k <= ssize + 70
    si, di, al = si[:k].astype(np.int64), di[:k].astype(np.int64), al[:k]
    return si, di, al, np.searchsorted(di, np.arange(33))


def test_area_tables_equal_the_oracles(exe, orc):
    sizes = [33, 47, 100, 257, 600, 1000, 1366, 1568, 2976, 4000, 8191]
    for s, ln in zip(sizes, ask(exe, [f"area {s}" for s in sizes])):
        head, body = ln.split("|")
        si, di, al = parse_tab(body.split())
        wsi, wdi, wal, _ = orc_tab(orc, s)
        assert int(head) == len(wsi) == len(si), s
        assert (si == wsi).all() and (di == wdi).all(), s
        assert (al.view(np.uint32) == wal.view(np.uint32)).all(), s  # bit for bit


def test_area_fast_equals_the_oracles(exe, orc):
    f = orc.L.orc_resize_area_fast
    f.argtypes = [C.c_int, C.c_int]
    f.restype = C.c_int
    cases = [(32 * m, 96) for m in range(1, 257)]
    cases += [(32 * m + d, 96) for m in (1, 2, 20, 49, 60, 93, 256) for d in (-1, 1)]
    cases += [(96, 32 * m) for m in (1, 49, 50, 93, 98, 100)] + [(1568, 1568), (256, 256), (100, 64)]
    got = [int(x) for x in ask(exe, [f"fast {w} {h}" for w, h in cases])]
    want = [f(w, h) for w, h in cases]
    assert got == want
    assert 0 < sum(want[:256]) < 256  # both answers occur among the multiples of 32 (m = 49, 93, 98 ... miss by an ulp)


def test_yrows_replay_the_y_table(exe, orc):
    heights = [33, 47, 100, 300, 1080, 3000]
    pad = 8
    for h, ln in zip(heights, ask(exe, [f"yrow {h}" for h in heights])):
        head, body = ln.split("|")
        w = body.split()
        assert int(head) == h + 2 * pad == len(w) // 4, h  # a table exists: never more than two entries per source row
        a0, a1, k0 = f32(w[0::4]), f32(w[1::4]), f32(w[3::4])
        info = np.array(w[2::4], np.int64)
        for sl in (slice(0, pad), slice(h + pad, h + 2 * pad)):  # the neutral entries before and behind the rows
            assert (a0[sl] == 0).all() and (a1[sl] == 0).all() and (info[sl] == 0).all() and (k0[sl] == 1).all()
        a0, a1, k0, info = a0[pad:-pad], a1[pad:-pad], k0[pad:-pad], info[pad:-pad]
        si, di, al, first = orc_tab(orc, h)
        # replaying the rows in order gives the table's entries in order: (si, di, alpha), one or two per source row
        replay, opened, closed = [], [], []
        for y in range(h):
            d = int(info[y]) & 0xff
            replay.append((y, d, a0[y]))
            if info[y] & 0x100:
                opened.append(d)
            if info[y] & 0x200:
                closed.append(d)
            assert k0[y] == (0.0 if info[y] & 0x100 else 1.0)
            if info[y] & 0x400:
                replay.append((y, d + 1, a1[y]))
                if info[y] & 0x800:
                    opened.append(d + 1)
                if info[y] & 0x1000:
                    closed.append(d + 1)
            else:
                assert not info[y] & 0x1800 and a1[y] == 0
        replay.sort(key=lambda e: (e[1], e[0]))  # the table's order: by cell, then by source row
        assert [e[0] for e in replay] == si.tolist() and [e[1] for e in replay] == di.tolist(), h
        assert (np.array([e[2] for e in replay], np.float32).view(np.uint32) == al.view(np.uint32)).all(), h
        # the opens / closes bits partition the 32 cells: each opened once and closed once, in order
        assert opened == list(range(32)) and closed == list(range(32)), h


def band_rule(w, xs, tile, plain):
    """the B operand of one 16-column tile, restated: [64][4] words of four i8 weights"""
    lane, j = np.meshgrid(np.arange(64), np.arange(16), indexing="ij")
    k = 16 * (lane >> 4) + j
    col = xs + 16 * tile - 8 + (k & 31)
    xo = xs + 16 * tile + (lane & 15)
    if plain:
        wgt = (np.abs(col - xo) <= 3).astype(np.int64)
    else:
        wgt = np.zeros_like(col)
        for dd in range(-3, 4):
            p = xo + dd
            p = np.where(p < 0, -p, p)
            p = np.where(p >= w, 2 * (w - 1) - p, p)
            wgt += (p == col)
        wgt = np.where((col >= 0) & (col < w) & (xo < w), wgt, 0)
    wgt = np.where(k >= 32, -wgt, wgt) & 0xff
    return (wgt.reshape(64, 4, 4) << (8 * np.arange(4))).sum(axis=2).astype(np.uint32)


def test_band_area_strips_keep_what_the_kernel_assumes(exe, orc):
    widths = list(range(64, 1921))
    lines = iter(ask(exe, [f"strips {w}" for w in widths]))
    with_list = {}
    for w in widths:
        n, T, amax, RS = (int(x) for x in next(lines).split())
        strips = []
        for _ in range(n):
            head, cells = next(lines).split("|")
            strips.append(([int(x) for x in head.split()], [int(x) for x in cells.split()]))
        if not n:
            continue
        with_list[w] = strips
        si, di, al, first = orc_tab(orc, w)
        assert 2 <= T <= 15 and n >= 2, w
        cps = strips[0][0][3]
        assert (cps, RS) in ((16, 4), (11, 4), (8, 2), (4, 1)), w  # RS follows the cells per strip
        at = 0
        for (xs, sT, cell0, ncell, s_amax, s_amin, tp, rotm), si0 in strips:
            assert cell0 == at and 1 <= ncell <= cps and len(si0) == ncell, w  # the cells partition 0..31 in order
            assert ncell == min(cps, 32 - cell0), w
            at += ncell
            assert sT == T and (xs == 0 or xs >= 8) and xs + 16 * T <= w, w
            entries = np.diff(first)[cell0: cell0 + ncell]
            assert s_amax == entries.max() and s_amin == entries.min() and s_amax - s_amin <= 3 and s_amin >= 2, w
            for c in range(ncell):
                assert si0[c] == si[first[cell0 + c]] - xs, w
                assert 0 <= si0[c] and si0[c] + entries[c] <= 16 * T, w
            assert tp >= 16 * T + 8, w  # the images' planes do not overlap
            # interior tiles equal the plain band: no tap of their sixteen columns reaches past an image edge
            if T > 2:
                assert xs + 16 - 3 >= 0 and xs + 16 * (T - 2) + 15 + 3 <= w - 1, w
        assert at == 32, w
        assert strips[0][0][0] == 0 and strips[-1][0][0] + 16 * T == w, w  # the last strip ends at column w - 1
        assert amax == max(s[0][4] for s in strips), w
    # a test of the builder, not of an empty set (it makes a list for 1853 of the 1857 widths: all but 1915 and 1917-1919)
    assert len(with_list) > len(widths) // 2
    # the band matrices themselves, entry for entry against the rule, every tile of every strip: a sample of the widths
    sample = [w for w in (64, 100, 160, 257, 400, 533, 640, 800, 1000, 1024, 1366, 1600, 1919, 1920) if w in with_list]
    assert len(sample) >= 8
    lines = iter(ask(exe, [f"bands {w}" for w in sample]))
    for w in sample:
        for (xs, T, *_), _ in with_list[w]:
            band = np.array([int(x, 16) for x in next(lines).split()], np.uint32).reshape(3, 64, 4)
            assert (band[0] == band_rule(w, xs, 0, True)).all(), w
            assert (band[1] == band_rule(w, xs, 0, False)).all(), w
            assert (band[2] == band_rule(w, xs, T - 1, False)).all(), w
            for tile in range(1, T - 1):
                assert (band_rule(w, xs, tile, False) == band[0]).all(), (w, tile)


def test_column_strips_rebase_the_x_table(exe, orc):
    """make_strip_geom: the strips' cells partition the table; entries are the table's, rebased to the strip"""
    for w in (2049, 3000, 4097, 5000, 8191):
        si, di, al, first = orc_tab(orc, w)
        for ncol in (2, 4, 8):
            cpw = 32 // ncol
            for s, ln in enumerate(ask(exe, [f"cols {w} 0 {ncol} {s}" for s in range(ncol)])):
                head, body, xfirst = ln.split("|")
                x0, ws, n = (int(x) for x in head.split())
                gsi, gdi, gal = parse_tab(body.split())
                e0, e1 = first[s * cpw], first[(s + 1) * cpw]
                assert n == e1 - e0 and x0 == si[e0] and ws == si[e1 - 1] + 1 - x0
                assert (gsi == si[e0:e1] - x0).all() and (gdi == di[e0:e1] - s * cpw).all()
                assert (gal.view(np.uint32) == al[e0:e1].view(np.uint32)).all()
                assert gsi.min() == 0 and gsi.max() == ws - 1 and x0 + ws <= w
                xf = [int(x) for x in xfirst.split()]
                assert xf == [int(first[min(s * cpw + c, (s + 1) * cpw)] - e0) for c in range(33)]
    # integer ratios: whole pixel runs, no tables
    assert ask(exe, ["cols 4096 1 2 1", "cols 8192 1 4 3"]) == ["2048 2048 0 | |", "6144 2048 0 | |"]


def test_steps_per_strip_cover_the_image(exe):
    cases = [(h, ks, t, halo) for h in (40, 97, 300, 960, 1080, 8192) for ks, halo in ((14, 6), (21, 6), (15, 4), (15, 2))
             for t in range(1, 9)]
    got = [int(x) for x in ask(exe, [f"steps {h} {ks} {t} {halo} 1" for h, ks, t, halo in cases])]
    for (h, ks, t, halo), st in zip(cases, got):
        span = (h + halo + ks - 1) // ks  # one strip spanning the image
        out = st * ks - halo
        assert 1 <= st <= span and out >= 1, (h, ks, t)
        strips = (h + out - 1) // out
        assert strips * out >= h > (strips - 1) * out  # strips x output rows cover h, none is empty
        if t >= span:
            assert st == span
        else:
            assert max(2, t - 1) <= st <= t + 3
    # a forced "hash_stream" value: that many steps, clamped to one strip spanning the image
    forced = [(h, ks, v) for h in (40, 97, 300, 8192) for ks in (14, 21) for v in (2, 3, 4, 9, 50, 1000)]
    got = [int(x) for x in ask(exe, [f"steps {h} {ks} {v} 6 {v}" for h, ks, v in forced])]
    assert got == [max(1, min(v, (h + 6 + ks - 1) // ks)) for h, ks, v in forced]


def test_rows_per_step_fit_the_lds(exe):
    cases = [(K, T, ncell, per_row, fixed) for K in (3, 5, 7) for T in (64, 128, 192, 256) for ncell in (4, 8, 16, 32)
             for per_row in (64, 520, 1024, 2048, 2176, 3000, 3100, 3200, 4096)
             for fixed in (16, 2064, 4112, 9000)]
    got = [int(x) for x in ask(exe, ["rows %d %d %d %d %d" % c for c in cases])]
    for (K, T, ncell, per_row, fixed), ks in zip(cases, got):
        if K != 7:
            assert ks == 15
            continue
        assert ks in (14, 21)
        if ks == 21:  # 21 rows per step only when they fit 64 KB
            assert fixed + 21 * per_row <= 64 * 1024
            cap = 2 * T // ncell  # ... and fill the area phase's turns better than 14 do
            use = {k: k / (-(-k // cap) * cap) for k in (14, 21)}
            assert use[21] > use[14] + 0.05
    by_fit = {c: ks for c, ks in zip(cases, got) if c[0] == 7 and c[1:3] == (192, 32)}  # 12 slots per turn: 21 fills them
    assert by_fit[(7, 192, 32, 3000, 16)] == 21 and by_fit[(7, 192, 32, 3200, 16)] == 14  # 63016 / 67216 bytes
    assert by_fit[(7, 192, 32, 3100, 16)] == 21 and by_fit[(7, 192, 32, 3100, 2064)] == 14  # 65116 / 67164 bytes
