"""-merge A B: the DCT stage for all needles in one launch plus the placement behind the C ABI (database.merge,
cbh_merge_find + cbh_merge_place, merge.hip) against the reference's shape written with what exists (batched=False: per
needle one index.slice() of A + b_0 .. b_k and one query, the placement in Python), in the same process on the same
resident index.

    python tools/merge_bench.py [shapes=10000x100,10000x1000,16384x16384] [dht=5] [reps=5] [loop_max=1000] [sample=100]

Inputs are one random walk -- each item flips 0-3 bits of the previous one -- shuffled and cut into A and B, so most
needles find a neighbour and a few do not.  Equal results (merged ids and the per-needle report) are asserted before
anything is reported: up to `loop_max` needles against the whole loop.  Above `loop_max` the loop is not run to its end;
its cost is then an ESTIMATE, marked as such: the mean time of multi_search (slice + query) for `sample` needles spread
evenly over B -- the slice grows with k -- times |B|, each sampled answer held against the device route's report.  Host
clock around calls that end in a stream synchronise; warm-up first; medians of `reps`.  One JSON line per result
(profiles/merge.jsonl keeps them)."""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from cbird_amd import DctHashIndex, Media, SearchParams, _lib, require_device  # noqa: E402
from cbird_amd.database import merge, multi_search  # noqa: E402


def walk(n, rng):
    h = np.zeros(n, np.uint64)
    cur = int(rng.integers(1, 1 << 63))
    for k in range(n):
        for b in rng.choice(64, int(rng.integers(0, 4)), replace=False):
            cur ^= 1 << int(b)
        h[k] = cur or 1
    rng.shuffle(h)
    return [Media(id=1 + k, dctHash=int(x), path=f"/db/{1 + k}.jpg") for k, x in enumerate(h)]


def ids_of(result):
    return [m.id for m in result[0]], result[1]


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return out, statistics.median(ts), ts


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    shapes = [tuple(int(v) for v in s.split("x")) for s in kv.get("shapes", "10000x100,10000x1000,16384x16384").split(",")]
    dht, reps = int(kv.get("dht", 5)), int(kv.get("reps", 5))
    loop_max, sample = int(kv.get("loop_max", 1000)), int(kv.get("sample", 100))
    require_device()
    rng = np.random.default_rng(2024)
    p = SearchParams(dctThresh=dht)
    L = _lib.lib()
    for n_a, n_b in shapes:
        media = walk(n_a + n_b, rng)
        a, b = media[:n_a], media[n_a:]
        idx = DctHashIndex()
        idx.load([m.dctHash for m in media], [m.id for m in media])
        dev, t_dev, all_dev = timed(lambda: merge(idx, a, b, p), reps)
        status = [r[0] for r in dev[1]]
        row = {"bench": "merge", "n_a": n_a, "n_b": n_b, "dht": dht, "placed": status.count(0), "no_match": status.count(1),
               "match_unplaced": status.count(2), "device_ms": round(t_dev * 1e3, 3),
               "device_ms_all": [round(x * 1e3, 3) for x in all_dev]}
        # the C-ABI calls alone (arrays ready, host memory): what the Python entry adds is list handling and the
        # download of the index's ids
        hashes = np.array([m.dctHash for m in media], np.uint64)
        ids = np.array([m.id for m in media], np.uint32)
        match, score = np.zeros(n_b, np.uint32), np.zeros(n_b, np.int32)
        order, st, n_out = np.zeros(n_a + n_b, np.uint32), np.zeros(n_b, np.uint8), C.c_size_t(0)
        mp = _lib.cbh_merge_params(dht, 0, p.minMatches, 2, 0, 0)
        rc, t_find, _ = timed(lambda: L.cbh_merge_find(hashes.ctypes.data, ids.ctypes.data, None, None, None, n_a, n_b,
                                                       C.byref(mp), match.ctypes.data, score.ctypes.data, 0), reps)
        assert rc == 0
        rc, t_place, _ = timed(lambda: L.cbh_merge_place(hashes.ctypes.data, n_a, n_b, match.ctypes.data, order.ctypes.data,
                                                         st.ctypes.data, C.byref(n_out)), reps)
        assert rc == 0 and ids[order[:n_out.value]].tolist() == [m.id for m in dev[0]] and st.tolist() == status
        row.update(find_ms=round(t_find * 1e3, 3), find_us_per_needle=round(t_find / n_b * 1e6, 3),
                   place_ms=round(t_place * 1e3, 3))
        if n_b <= loop_max:
            t0 = time.perf_counter()
            ref = merge(idx, a, b, p, batched=False)
            t_loop = time.perf_counter() - t0
            assert ids_of(ref) == ids_of(dev), "the device route and the loop differ"
            row.update(loop_ms=round(t_loop * 1e3, 1), loop_estimated=False)
        else:
            id_map = {m.id: m for m in media}
            all_ids = [m.id for m in media]
            ts = []
            for k in np.linspace(0, n_b - 1, sample).astype(int).tolist():
                t0 = time.perf_counter()
                got, algo = multi_search(idx, b[k], p, id_map, all_ids[:n_a + k + 1])
                ts.append(time.perf_counter() - t0)
                want = dev[1][k]
                assert (algo, got[0].score if got else -1, got[0].id if got else 0) == want[1:], "the routes differ"
            t_loop = statistics.mean(ts) * n_b
            row.update(loop_ms=round(t_loop * 1e3, 1), loop_estimated=True, loop_needle_us=round(statistics.mean(ts) * 1e6, 1))
        row["loop_over_device"] = round(t_loop / t_dev, 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
