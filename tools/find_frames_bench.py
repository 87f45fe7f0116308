"""Image needles against the video index: cbh_vidx_find_frames_batch (one scan, one reduction on the device, frames.hip)
against a loop over cbh_vidx_find_frame (one scan, sort, copy and host reduction per needle), in the same process on the
same resident index, alternating; both sides must return equal results.  Then the cost of long runs: one static video of
S identical frames searched by N needles that all hit it, N * S held constant -- time per record must stay flat.

    python tools/find_frames_bench.py [needles=4096] [clips=10000] [frames=300] [dht=5] [reps=5]

Host clock around calls that end in a stream synchronise; warm-up first; medians of `reps`.  One JSON line per result."""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from cbird_amd import _lib, require_device, synth_video  # noqa: E402

H = 0x0F0F0F0F0F0F0F0E


def build(L, clips, first_id=1):
    v = L.cbh_vidx_create(0)
    assert v
    for i, (f, h) in enumerate(clips):
        f = np.ascontiguousarray(f, np.int32)
        h = np.ascontiguousarray(h, np.uint64)
        _lib.check(L.cbh_vidx_add_video(v, first_id + i, f.ctypes.data, h.ctypes.data, len(f)), "add_video")
    return v


def batch(L, v, q, dht, buf):
    offs = np.zeros(len(q) + 1, np.uint64)
    t0 = time.perf_counter()
    rc = L.cbh_vidx_find_frames_batch(v, q.ctypes.data, None, len(q), dht, 0, buf, len(buf), offs.ctypes.data)
    dt = time.perf_counter() - t0
    return rc, offs, dt


def loop(L, v, q, dht, buf):
    n = C.c_size_t(0)
    rows, counts = [], []
    t0 = time.perf_counter()
    for x in q.tolist():
        _lib.check(L.cbh_vidx_find_frame(v, x, dht, 0, -1, buf, len(buf), C.byref(n)), "find_frame")
        counts.append(n.value)
        rows.append(C.string_at(C.addressof(buf), n.value * C.sizeof(_lib.cbh_vmatch)))
    dt = time.perf_counter() - t0
    return rows, counts, dt


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    nq, n_clips, n_frames = int(kv.get("needles", 4096)), int(kv.get("clips", 10000)), int(kv.get("frames", 300))
    dht, reps = int(kv.get("dht", 5)), int(kv.get("reps", 5))
    require_device()
    L = _lib.lib()
    clips = synth_video.make_clips_fast(n_clips, n_frames, seed=1234, subclip_frac=0.01, max_gap=8)
    v = build(L, clips)
    entries = int(L.cbh_vidx_entries(v, 0))
    rng = np.random.default_rng(99)
    q = np.ascontiguousarray([clips[int(c)][1][int(rng.integers(0, len(clips[int(c)][1])))]
                              for c in rng.integers(0, n_clips, nq)], np.uint64)
    one = (_lib.cbh_vmatch * max(1, n_clips))()
    rc, offs, _ = batch(L, v, q, dht, (_lib.cbh_vmatch * 1)())  # warm-up, and the room the result needs
    assert rc in (0, _lib.CBH_E_OVERFLOW)
    buf = (_lib.cbh_vmatch * max(1, int(offs[-1])))()
    loop(L, v, q[:64], dht, one)
    tb, tl = [], []
    for _ in range(reps):  # alternating
        rc, offs, dt = batch(L, v, q, dht, buf)
        assert rc == 0
        tb.append(dt)
        rows, counts, dt = loop(L, v, q, dht, one)
        tl.append(dt)
    sz = C.sizeof(_lib.cbh_vmatch)
    raw = C.string_at(C.addressof(buf), len(buf) * sz)
    for i in range(nq):  # equal results, needle by needle
        assert int(offs[i + 1] - offs[i]) == counts[i], i
        assert raw[int(offs[i]) * sz:int(offs[i + 1]) * sz] == rows[i], i
    b, l = statistics.median(tb), statistics.median(tl)
    print(json.dumps({"bench": "find_frames", "needles": nq, "entries": entries, "dht": dht, "rows": int(offs[-1]),
                      "batch_ms": round(b * 1e3, 3), "loop_ms": round(l * 1e3, 3),
                      "batch_us_per_needle": round(b / nq * 1e6, 3), "loop_us_per_needle": round(l / nq * 1e6, 3),
                      "loop_over_batch": round(l / b, 2), "batch_ms_all": [round(x * 1e3, 3) for x in tb],
                      "loop_ms_all": [round(x * 1e3, 3) for x in tl]}))
    L.cbh_vidx_destroy(v)
    # long runs: every needle hits every frame of one static video
    records = 1 << 22
    for s in (1 << 10, 1 << 12, 1 << 14, 1 << 16):
        v = build(L, [(np.arange(s, dtype=np.int32), np.full(s, H, np.uint64))])
        assert int(L.cbh_vidx_entries(v, 0)) == s
        qs = np.full(records // s, H, np.uint64)
        buf = (_lib.cbh_vmatch * len(qs))()
        ts = []
        for _ in range(reps + 1):
            rc, offs, dt = batch(L, v, qs, 3, buf)
            assert rc == 0 and int(offs[-1]) == len(qs) and (buf[0].score, buf[0].dst_in) == (0, 0)
            ts.append(dt)
        t = statistics.median(ts[1:])
        print(json.dumps({"bench": "find_frames_static", "records_per_needle": s, "needles": len(qs), "records": records,
                          "ms": round(t * 1e3, 3), "ns_per_record": round(t / records * 1e9, 3)}))
        L.cbh_vidx_destroy(v)


if __name__ == "__main__":
    main()
