"""Same-box A/B of Index::slice() between two BUILDS of the library, in ONE process: the parent commit's library (built from
`git stash` / an earlier checkout and kept as a file) and the current one are loaded side by side (RTLD_LOCAL: each keeps
its own arena and knobs; they share the HIP runtime), every case is built in both, the two slices are first held equal,
then the two are timed alternately, five times each, on the host clock around calls that end in a synchronise.

Cases (a random half of the ids is kept):
  idx64_1e6       cbh_idx64_slice, 10^6 slots, one per id                                      (as long as both builds
  idx64_4e7       cbh_idx64_slice, 4 * 10^7 slots, 400 per id (a DctFeaturesIndex of 10^5 images)  take the host route these
                  two time one route against itself: its cost, and the noise of the method)
  idx256_1e5x100  10^5 media x 100 rows; parent side: rows_of + download_rows + add per kept media, what the adapters ran
  color_1e6       10^6 entries; parent side: download + host filter + add, what the adapters ran

Per case one JSON line: the medians, the parent's max - min spread, the bytes the slice has to move (computed from the
shapes: every id read once, every kept entry read and written once) over the new median.  Exit code 1 if in some case
the new median exceeds the parent's by more than the parent's own spread.

What the figures include: the host clock runs around a Python lambda and its ctypes calls on both sides; destroy is outside
the timed region on both.  The parent side of idx256_1e5x100 is the adapters' composition run through ctypes, a Python loop
of 5 * 10^4 iterations with three foreign calls each, not the C++ loop the adapter ran: the interpreter's share flatters that
ratio (and, through np.isin, colour's a little).
    python tools/ab/slice_ab.py PARENT_LIB [out=profiles/r09_slice_ab.jsonl] [cases=idx64_1e6,idx64_4e7,idx256_1e5x100,color_1e6]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from cbird_amd import _lib  # noqa: E402
from cbird_amd.colordesc import COLOR_DTYPE  # noqa: E402

ROUNDS = 5


def load(path):
    import torch  # noqa: F401  (the HIP runtime both libraries then share)

    L = C.CDLL(os.path.abspath(path), mode=C.RTLD_LOCAL)
    for name, (res, args) in _lib._SIGS.items():
        if hasattr(L, name):  # (the parent build lacks the new entry points)
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
    return L


def ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {rc}")


def timed(call, destroy):
    t0 = time.perf_counter()
    h = call()
    ms = (time.perf_counter() - t0) * 1e3
    assert h
    destroy(h)
    return ms


def alternate(case, parent, new, nbytes, extra):
    p, n = [], []
    for _ in range(ROUNDS):
        p.append(timed(*parent))
        n.append(timed(*new))
    pm, nm = statistics.median(p), statistics.median(n)
    spread = max(p) - min(p)
    return dict(case=case, **extra, parent_ms=[round(x, 3) for x in p], new_ms=[round(x, 3) for x in n],
                parent_median_ms=round(pm, 3), new_median_ms=round(nm, 3), parent_spread_ms=round(spread, 3),
                speedup=round(pm / nm, 2), bytes_moved=int(nbytes), new_tb_per_s=round(nbytes / (nm * 1e-3) / 1e12, 4),
                within_condition=bool(nm <= pm + spread))


def case_idx64(P, N, name, n, per_id):
    rng = np.random.default_rng(1)
    ids = (np.arange(n, dtype=np.uint32) // per_id + 1).astype(np.uint32)
    h = rng.integers(1, 1 << 63, n, dtype=np.uint64)
    want = np.ascontiguousarray(rng.permutation(np.unique(ids))[: (n // per_id) // 2], np.uint32)
    hp, hn = P.cbh_idx64_create(0), N.cbh_idx64_create(0)
    ok(P.cbh_idx64_load(hp, h.ctypes.data, ids.ctypes.data, n), "load")
    ok(N.cbh_idx64_load(hn, h.ctypes.data, ids.ctypes.data, n), "load")

    def down(L, s):
        m = L.cbh_idx64_count(s)
        a, b = np.zeros(m, np.uint64), np.zeros(m, np.uint32)
        ok(L.cbh_idx64_download(s, a.ctypes.data, b.ctypes.data, m), "download")
        return a, b

    sp, sn = P.cbh_idx64_slice(hp, want.ctypes.data, len(want)), N.cbh_idx64_slice(hn, want.ctypes.data, len(want))
    (ah, ai), (bh, bi) = down(P, sp), down(N, sn)
    assert len(ai) == len(bi) > 0 and (ah == bh).all() and (ai == bi).all(), "the two slices differ"
    m = len(ai)
    P.cbh_idx64_destroy(sp), N.cbh_idx64_destroy(sn)
    r = alternate(name, (lambda: P.cbh_idx64_slice(hp, want.ctypes.data, len(want)), P.cbh_idx64_destroy),
                  (lambda: N.cbh_idx64_slice(hn, want.ctypes.data, len(want)), N.cbh_idx64_destroy),
                  4 * n + 2 * 12 * m, dict(slots=n, kept=m, wanted_ids=len(want)))
    P.cbh_idx64_destroy(hp), N.cbh_idx64_destroy(hn)
    return r


def case_idx256(P, N, name, media, per):
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 256, (media * per, 32), dtype=np.uint8)
    hp, hn = P.cbh_idx256_create(0), N.cbh_idx256_create(0)
    for L, hnd in ((P, hp), (N, hn)):
        for i in range(media):
            ok(L.cbh_idx256_add(hnd, i + 1, rows[i * per:(i + 1) * per].ctypes.data, per), "add")
    want = np.ascontiguousarray(np.sort(rng.permutation(media)[: media // 2] + 1), np.uint32)
    buf = np.zeros((per, 32), np.uint8)

    def compose():  # what GpuCvFeaturesIndex::slice ran: one rows_of, one blocking download, one add per media
        s = P.cbh_idx256_create(0)
        f, c = C.c_size_t(0), C.c_size_t(0)
        for mid in want:
            ok(P.cbh_idx256_rows_of(hp, int(mid), C.byref(f), C.byref(c)), "rows_of")
            if c.value:
                ok(P.cbh_idx256_download_rows(hp, f.value, c.value, buf.ctypes.data), "download_rows")
                ok(P.cbh_idx256_add(s, int(mid), buf.ctypes.data, c.value), "add")
        return s

    def down(L, s):
        m = L.cbh_idx256_count(s)
        a = np.zeros((m, 32), np.uint8)
        ok(L.cbh_idx256_download_rows(s, 0, m, a.ctypes.data), "download_rows")
        return a

    sp, sn = compose(), N.cbh_idx256_slice(hn, want.ctypes.data, len(want))
    a, b = down(P, sp), down(N, sn)
    assert a.shape == b.shape and len(a) > 0 and (a == b).all(), "the two slices differ"
    m = len(a)
    P.cbh_idx256_destroy(sp), N.cbh_idx256_destroy(sn)
    r = alternate(name, (compose, P.cbh_idx256_destroy),
                  (lambda: N.cbh_idx256_slice(hn, want.ctypes.data, len(want)), N.cbh_idx256_destroy),
                  2 * 32 * m, dict(rows=media * per, kept_rows=m, kept_media=len(want)))
    P.cbh_idx256_destroy(hp), N.cbh_idx256_destroy(hn)
    return r


def case_color(P, N, name, n):
    rng = np.random.default_rng(3)
    d = np.zeros(n, COLOR_DTYPE)
    d["colors"] = rng.integers(0, 65536, d["colors"].shape, dtype=np.uint16)
    d["numColors"] = rng.integers(0, 33, n)
    ids = np.arange(1, n + 1, dtype=np.uint32)
    hp, hn = P.cbh_color_create(0), N.cbh_color_create(0)
    ok(P.cbh_color_add(hp, ids.ctypes.data, d.ctypes.data, n), "add")
    ok(N.cbh_color_add(hn, ids.ctypes.data, d.ctypes.data, n), "add")
    want = np.ascontiguousarray(np.sort(rng.permutation(n)[: n // 2] + 1), np.uint32)

    def compose():  # what GpuColorDescIndex::slice ran: download, filter on the host, add
        gi, gd = np.zeros(n, np.uint32), np.zeros(n, COLOR_DTYPE)
        ok(P.cbh_color_download(hp, gi.ctypes.data, gd.ctypes.data, n), "download")
        keep = np.isin(gi, want)
        ki, kd = np.ascontiguousarray(gi[keep]), np.ascontiguousarray(gd[keep])
        s = P.cbh_color_create(0)
        ok(P.cbh_color_add(s, ki.ctypes.data, kd.ctypes.data, len(ki)), "add")
        return s

    needles = np.ascontiguousarray(d[:4])

    def look(L, s):
        m = L.cbh_color_count(s)
        gi, gd = np.zeros(m, np.uint32), np.zeros(m, COLOR_DTYPE)
        ok(L.cbh_color_download(s, gi.ctypes.data, gd.ctypes.data, m), "download")
        dist = np.zeros((4, m), np.float32)
        ok(L.cbh_color_distances(s, needles.ctypes.data, 4, dist.ctypes.data), "distances")
        return gi.tobytes(), gd.tobytes(), dist.tobytes(), m

    sp, sn = compose(), N.cbh_color_slice(hn, want.ctypes.data, len(want))
    a, b = look(P, sp), look(N, sn)
    assert a == b and a[3] > 0, "the two slices differ"
    m = a[3]
    P.cbh_color_destroy(sp), N.cbh_color_destroy(sn)
    r = alternate(name, (compose, P.cbh_color_destroy),
                  (lambda: N.cbh_color_slice(hn, want.ctypes.data, len(want)), N.cbh_color_destroy),
                  m * 4 + 2 * m * (96 * 4 + 4 + 1), dict(entries=n, kept=m))
    P.cbh_color_destroy(hp), N.cbh_color_destroy(hn)
    return r


CASES = {"idx64_1e6": lambda P, N: case_idx64(P, N, "idx64_1e6", 10 ** 6, 1),
         "idx64_4e7": lambda P, N: case_idx64(P, N, "idx64_4e7", 4 * 10 ** 7, 400),
         "idx256_1e5x100": lambda P, N: case_idx256(P, N, "idx256_1e5x100", 10 ** 5, 100),
         "color_1e6": lambda P, N: case_color(P, N, "color_1e6", 10 ** 6)}


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r09_slice_ab.jsonl")
    names = sys.argv[3].split(",") if len(sys.argv) > 3 else list(CASES)
    P, N = load(sys.argv[1]), load(os.path.join(ROOT, "cbird_amd", "libcbird_hip.so"))
    if N.cbh_device_count() <= 0:
        sys.exit("no usable gfx950 device: nothing is measured without one")
    bad = 0
    with open(out, "a") as f:
        for name in names:
            r = CASES[name](P, N)
            bad += not r["within_condition"]
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
