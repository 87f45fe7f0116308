"""Same-box A/B of the bucketed join ("scan_mfma" 4) between two BUILDS of the library in ONE process: the parent commit's
library (built from an earlier checkout and kept as a file) and the current one, loaded side by side as tools/ab/slice_ab.py
does.  Data: the bench's image-derived hashes (bench.gen_images + cbh_dcthash_batch_dev), `images` of them as slots and as
needles.  Per threshold 1..8 three contestants, alternated five times:
  parent     the parent build (slots' side prepared on every call)
  plain      this build, handle not opted in (likewise)
  resident   this build, cbh_idx64_join_prepare'd handle (slot tables built before the timed region)
Plain handles: cbh_idx64_time_scan_dev, i.e. HIP events around one joined launch.  (1, 5) sharded handles: that entry point
does not take them, so the host clock around cbh_idx64_find_batch_dev (which ends in a synchronise; k = 8) -- the whole
call, cut included, on all three.  One JSON line per (shape, threshold) with the five times of each, medians, the parent's
max - min spread and the two verdicts the change is held to: plain <= parent + spread, resident < parent - spread; and a
last line per shape with the 1..8 sweeps.  Nothing is tuned here: what a threshold does not gain is for NOTES.md to say.
    python tools/ab/join_resident_ab.py PARENT_LIB [out=profiles/join_resident_ab.jsonl] [images=1000000]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from cbird_amd import _lib  # noqa: E402
from slice_ab import load, ok  # noqa: E402

ROUNDS = 5
CAP = 1 << 24  # records a timed launch may write (more are counted, not stored)


def image_hashes(torch, L, n, seed=1234):
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    step = 16384
    for a in range(0, n, step):
        b = min(n, a + step)
        imgs = bench.gen_images(torch, "cuda", a, b, n, seed)
        ok(L.cbh_dcthash_batch_dev(imgs.data_ptr(), b - a, bench.W, bench.H, bench.W, bench.W * bench.H,
                                   out[a:b].data_ptr(), 0, None), "dcthash")
    torch.cuda.synchronize()
    return out


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "join_resident_ab.jsonl")
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
    import torch

    P, N = load(sys.argv[1]), load(os.path.join(ROOT, "cbird_amd", "libcbird_hip.so"))
    if N.cbh_device_count() <= 0:
        sys.exit("no usable gfx950 device: nothing is measured without one")
    dh = image_hashes(torch, N, n)
    di = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    rec = torch.empty(CAP + 1, dtype=torch.int64, device="cuda")
    tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    dout = torch.empty((n, 8, 2), dtype=torch.int32, device="cuda")
    dcnt = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for L in (P, N):
        ok(L.cbh_set_tuning(b"scan_mfma", 4), "scan_mfma")
    bad = 0
    with open(out, "a") as f:
        def emit(r):
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for shape in ("plain", "sharded_1x5"):
            def make(L):
                h = L.cbh_idx64_create(0) if shape == "plain" else L.cbh_idx64_create_sharded(1, 5)
                assert h
                ok(L.cbh_idx64_load_dev(h, dh.data_ptr(), di.data_ptr(), n, None), "load_dev")
                return h

            hp, hn, hr = make(P), make(N), make(N)
            who = {"parent": (P, hp), "plain": (N, hn), "resident": (N, hr)}
            sweep = {k: 0.0 for k in who}
            for t in range(1, 9):
                ok(N.cbh_idx64_join_prepare(hr, t), "join_prepare")

                def once(L, h):
                    if shape == "plain":
                        ms = C.c_float(0)
                        ok(L.cbh_idx64_time_scan_dev(h, dh.data_ptr(), n, t, rec.data_ptr(), CAP, tot.data_ptr(), 1,
                                                     C.byref(ms)), "time_scan_dev")
                        return float(ms.value), int(tot.item())
                    total = C.c_uint64(0)
                    t0 = time.perf_counter()
                    ok(L.cbh_idx64_find_batch_dev(h, dh.data_ptr(), n, t, 8, dout.data_ptr(), dcnt.data_ptr(),
                                                  C.byref(total), None), "find_batch_dev")
                    return (time.perf_counter() - t0) * 1e3, int(total.value)

                totals = {k: once(*v)[1] for k, v in who.items()}  # (warm: arenas, workspaces, record blocks)
                assert len(set(totals.values())) == 1, totals
                ms = {k: [] for k in who}
                for _ in range(ROUNDS):
                    for k, v in who.items():
                        ms[k].append(once(*v)[0])
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = max(ms["parent"]) - min(ms["parent"])
                for k in who:
                    sweep[k] += med[k]
                r = dict(shape=shape, slots=n, needles=n, thresh=t, records=totals["parent"],
                         **{k + "_ms": [round(x, 4) for x in v] for k, v in ms.items()},
                         **{k + "_median_ms": round(v, 4) for k, v in med.items()}, parent_spread_ms=round(spread, 4),
                         plain_no_slower=bool(med["plain"] <= med["parent"] + spread),
                         resident_faster=bool(med["resident"] < med["parent"] - spread))
                bad += not (r["plain_no_slower"] and r["resident_faster"])
                emit(r)
            st = _lib.cbh_join_stats()
            ok(N.cbh_idx64_join_stats(hr, C.byref(st)), "join_stats")
            emit(dict(shape=shape, sweep_1_8_ms={k: round(v, 3) for k, v in sweep.items()}, resident_bytes=int(st.bytes),
                      builds=int(st.builds), hits=int(st.hits), resident_sweep_below_parent=bool(sweep["resident"] < sweep["parent"])))
            bad += not sweep["resident"] < sweep["parent"]
            for L, h in who.values():
                L.cbh_idx64_destroy(h)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
