"""-sort-similar: the whole chain in one kernel launch (database.sort_similar, cbh_sort_similar, sortsimilar.hip) against
the reference's shape written with what exists (batched=False: one index.slice(), one query and one insert per pass), in
the same process on the same resident index.

    python tools/sort_similar_bench.py [n=1000,16384] [sets=256] [set_n=1000] [dht=7] [reps=5] [loop_max=2000] [sample=200]

Inputs are random walks -- each item flips 0-3 bits of the previous one -- shuffled.  Single sets of every size in `n`,
then `sets` selections of `set_n` items as one batch.  Equal results are asserted before anything is timed: a single set
of at most `loop_max` items against the whole loop, the batch against the single-set calls and its first two sets against
the loop.  Above `loop_max` the loop is not run to its end (it takes 5 (n - 1) slices of a shrinking set); its cost is then
an ESTIMATE, marked as such: the median time of `sample` of its passes (slice of the whole unsorted set + query) times the
number of passes.  Host clock around calls that end in a stream synchronise; warm-up first; medians of `reps`.  One JSON
line per result."""
import ctypes as C
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from cbird_amd import DctHashIndex, Media, SearchParams, _lib, require_device  # noqa: E402
from cbird_amd.database import query, sort_similar, sort_similar_batch  # noqa: E402


def walk(n, rng, first_id):
    h = np.zeros(n, np.uint64)
    cur = int(rng.integers(1, 1 << 63))
    for k in range(n):
        for b in rng.choice(64, int(rng.integers(0, 4)), replace=False):
            cur ^= 1 << int(b)
        h[k] = cur or 1
    rng.shuffle(h)
    return [Media(id=first_id + k, dctHash=int(x), path=f"/db/{first_id + k}.jpg") for k, x in enumerate(h)]


def ids_of(result):
    return [m.id for m in result[0]], result[1], result[2]


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
    sizes = [int(x) for x in kv.get("n", "1000,16384").split(",")]
    n_sets, set_n = int(kv.get("sets", 256)), int(kv.get("set_n", 1000))
    dht, reps = int(kv.get("dht", 7)), int(kv.get("reps", 5))
    loop_max, sample = int(kv.get("loop_max", 2000)), int(kv.get("sample", 200))
    require_device()
    rng = np.random.default_rng(2024)
    p = SearchParams(dctThresh=dht)
    for n in sizes:
        sel = walk(n, rng, 1)
        idx = DctHashIndex()
        idx.load([m.dctHash for m in sel], [m.id for m in sel])
        dev, t_dev, all_dev = timed(lambda: sort_similar(idx, sel, p), reps)
        row = {"bench": "sort_similar", "n": n, "dht": dht, "sorted": len(dev[0]), "queries": dev[1], "not_found": dev[2],
               "device_ms": round(t_dev * 1e3, 3), "device_ms_all": [round(x * 1e3, 3) for x in all_dev]}
        # the C-ABI call alone (arrays ready, host memory): what the Python entry adds is list handling
        hashes = np.array([m.dctHash for m in sel], np.uint64)
        ids = np.array([m.id for m in sel], np.uint32)
        first = np.array([0, n], np.uint64)
        out_ids, res1 = np.zeros(n, np.uint32), _lib.cbh_sort_similar_result()
        sp = _lib.cbh_sort_similar_params(dht, 0, p.minMatches, p.maxMatches, 0, 0, 5)
        rc, t_c, _ = timed(lambda: _lib.lib().cbh_sort_similar(hashes.ctypes.data, ids.ctypes.data, None, None, None,
                                                               first.ctypes.data, 1, C.byref(sp), out_ids.ctypes.data,
                                                               C.byref(res1), 0), reps)
        assert rc == 0 and out_ids[:res1.sorted].tolist() == [m.id for m in dev[0]]
        row.update(cabi_ms=round(t_c * 1e3, 3), cabi_us_per_query=round(t_c / max(1, res1.queries) * 1e6, 3))
        if n <= loop_max:
            t0 = time.perf_counter()
            ref = sort_similar(idx, sel, p, batched=False)
            t_loop = time.perf_counter() - t0
            assert ids_of(ref) == ids_of(dev), "the device route and the loop differ"
            row.update(loop_ms=round(t_loop * 1e3, 1), loop_estimated=False)
        else:
            id_map = {m.id: m for m in sel}
            ts = []
            for k in range(sample):
                needle = sel[int(rng.integers(0, n))]
                t0 = time.perf_counter()
                query(idx.slice(list(id_map)), needle, p, id_map)
                ts.append(time.perf_counter() - t0)
            t_loop = statistics.median(ts) * dev[1]
            row.update(loop_ms=round(t_loop * 1e3, 1), loop_estimated=True, loop_pass_us=round(statistics.median(ts) * 1e6, 1))
        row["loop_over_device"] = round(t_loop / t_dev, 1)
        print(json.dumps(row), flush=True)
    sets = [walk(set_n, rng, 1 + s * set_n) for s in range(n_sets)]
    flat = [m for s in sets for m in s]
    idx = DctHashIndex()
    idx.load([m.dctHash for m in flat], [m.id for m in flat])
    res, t_batch, all_batch = timed(lambda: sort_similar_batch(idx, sets, p), reps)
    hashes = np.array([m.dctHash for m in flat], np.uint64)
    ids = np.array([m.id for m in flat], np.uint32)
    first = np.arange(n_sets + 1, dtype=np.uint64) * np.uint64(set_n)
    out_ids, resn = np.zeros(len(flat), np.uint32), (_lib.cbh_sort_similar_result * n_sets)()
    sp = _lib.cbh_sort_similar_params(dht, 0, p.minMatches, p.maxMatches, 0, 0, 5)
    rc, t_c, all_c = timed(lambda: _lib.lib().cbh_sort_similar(hashes.ctypes.data, ids.ctypes.data, None, None, None,
                                                               first.ctypes.data, n_sets, C.byref(sp), out_ids.ctypes.data,
                                                               resn, 0), reps)
    assert rc == 0
    for s in range(n_sets):
        assert out_ids[s * set_n:s * set_n + resn[s].sorted].tolist() == [m.id for m in res[s][0]], s
    t0 = time.perf_counter()
    singles = [sort_similar(idx, s, p) for s in sets]
    t_singles = time.perf_counter() - t0
    assert [ids_of(r) for r in res] == [ids_of(r) for r in singles], "the batch and the single-set calls differ"
    t0 = time.perf_counter()
    for s in range(min(2, n_sets)):
        assert ids_of(sort_similar(idx, sets[s], p, batched=False)) == ids_of(res[s]), "the batch and the loop differ"
    t_loop = (time.perf_counter() - t0) / max(1, min(2, n_sets)) * n_sets
    print(json.dumps({"bench": "sort_similar_batch", "sets": n_sets, "set_n": set_n, "dht": dht,
                      "queries": sum(r[1] for r in res), "batch_ms": round(t_batch * 1e3, 3),
                      "batch_ms_all": [round(x * 1e3, 3) for x in all_batch], "cabi_ms": round(t_c * 1e3, 3),
                      "cabi_ms_all": [round(x * 1e3, 3) for x in all_c], "single_calls_ms": round(t_singles * 1e3, 1),
                      "loop_ms": round(t_loop * 1e3, 1), "loop_estimated": True,
                      "loop_over_batch": round(t_loop / t_batch, 1)}), flush=True)


if __name__ == "__main__":
    main()
