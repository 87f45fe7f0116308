"""-sort-similar with -p.alg color: the score tables filled and walked on the device (ColorDescIndex.sort_similar,
cbh_color_sort_similar; color.hip + sortsimilar_table.hip) against the reference's shape written with what exists
(database.sort_similar with batched=False: one index.slice(), one query and one insert per pass), in the same process on
the same resident index.

    python tools/sort_similar_color_bench.py [n=1000,4096,16384] [sets=64] [set_n=1000] [reps=5] [loop_max=1000] [sample=200]
                                             [out=profiles/sort_similar_color.jsonl]

Descriptors come from synth_descriptors (tests/color_search_cases.py: random palettes with near-duplicates, 5 % without
colours) with the colour counts redrawn to 20..22, so that most pairs have a finite distance and the chain runs on.
Single selections of every size in `n`, then `sets` selections of `set_n` items in one call.  Host clock around whole
host-entry calls (they end in a stream synchronise), a warm-up first, the median of `reps`; one more call with
"color_sort_timing" 1 gives the table fill and the chain apart, from events inside the call.  The loop runs to its end up
to `loop_max` items (and its result is asserted equal); above that its cost is an ESTIMATE, marked as such: the median of
`sample` of its passes (slice of the whole unsorted set + query) times the device route's number of queries.  One JSON
line per result, printed and appended to `out`."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from color_search_cases import COLOR_DTYPE, synth_descriptors  # noqa: E402

from cbird_amd import Media, SearchParams, _lib, require_device  # noqa: E402
from cbird_amd.colordesc import ColorDescIndex  # noqa: E402
from cbird_amd.database import query, sort_similar, sort_similar_batch  # noqa: E402


def descriptors(n, seed):
    d, _ = synth_descriptors(n, seed)
    rng = np.random.default_rng([seed, n])
    fresh = rng.integers(0, 65536, (n, 32, 4)).astype(np.uint16)
    beyond = np.arange(32)[None, :] >= d["numColors"][:, None]
    d["colors"][beyond] = fresh[beyond]
    d["numColors"] = np.where(d["numColors"] == 0, 0, rng.integers(20, 23, n))
    return d


def media_of(descs, first_id):
    out = []
    for k, d in enumerate(descs):
        m = Media(id=first_id + k, path=f"/db/{first_id + k}.jpg")
        m.colorDescriptor = d
        out.append(m)
    return out


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


def tuning(key):
    v = C.c_longlong(0)
    assert _lib.lib().cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


def stages(call):
    L = _lib.lib()
    L.cbh_set_tuning(b"color_sort_timing", 1)
    try:
        call()
        return {"fill_ms": round(tuning(b"color_sort_fill_us") / 1e3, 3), "chain_ms": round(tuning(b"color_sort_chain_us") / 1e3, 3)}
    finally:
        L.cbh_set_tuning(b"color_sort_timing", 0)


def loop_pass_seconds(idx, sel, p, rng, sample):
    id_map = {m.id: m for m in sel}
    ts = []
    for _ in range(sample):
        needle = sel[int(rng.integers(0, len(sel)))]
        t0 = time.perf_counter()
        query(idx.slice(list(id_map)), needle, p, id_map)
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    sizes = [int(x) for x in kv.get("n", "1000,4096,16384").split(",")]
    n_sets, set_n, reps = int(kv.get("sets", 64)), int(kv.get("set_n", 1000)), int(kv.get("reps", 5))
    loop_max, sample = int(kv.get("loop_max", 1000)), int(kv.get("sample", 200))
    out_path = kv.get("out", os.path.join(ROOT, "profiles", "sort_similar_color.jsonl"))
    require_device()
    rng = np.random.default_rng(2024)
    p = SearchParams(algo=SearchParams.AlgoColor)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for n in sizes:
        descs = descriptors(n, 11)
        sel = media_of(descs, 1)
        ids = np.array([m.id for m in sel], np.uint32)
        idx = ColorDescIndex()
        idx.add(sel)
        dev, t_dev, all_dev = timed(lambda: idx.sort_similar(ids, descs, p)[0], reps)
        row = {"bench": "sort_similar_color", "n": n, "sorted": len(dev[0]), "queries": dev[1], "not_found": dev[2],
               "behind": dev[3], "device_ms": round(t_dev * 1e3, 3), "device_ms_all": [round(x * 1e3, 3) for x in all_dev],
               "us_per_query": round(t_dev / max(1, dev[1]) * 1e6, 3)}
        row.update(stages(lambda: idx.sort_similar(ids, descs, p)))
        py, t_py, _ = timed(lambda: sort_similar(idx, sel, p), reps)  # the Python entry: Media lists in and out
        assert ids_of(py) == (dev[0], dev[1], dev[2])
        row["python_entry_ms"] = round(t_py * 1e3, 3)
        if n <= loop_max:
            t0 = time.perf_counter()
            ref = sort_similar(idx, media_of(descs, 1), p, batched=False)
            t_loop = time.perf_counter() - t0
            assert ids_of(ref) == ids_of(py), "the device route and the loop differ"
            row.update(loop_ms=round(t_loop * 1e3, 1), loop_estimated=False)
        else:
            t_pass = loop_pass_seconds(idx, sel, p, rng, sample)
            t_loop = t_pass * dev[1]
            row.update(loop_ms=round(t_loop * 1e3, 1), loop_estimated=True, loop_pass_us=round(t_pass * 1e6, 1))
        row["loop_over_device"] = round(t_loop / t_py, 1)
        emit(row)

    descs = descriptors(n_sets * set_n, 12)
    flat = media_of(descs, 1)
    sets = [flat[s * set_n:(s + 1) * set_n] for s in range(n_sets)]
    ids = np.array([m.id for m in flat], np.uint32)
    first = np.arange(n_sets + 1, dtype=np.uint64) * np.uint64(set_n)
    idx = ColorDescIndex()
    idx.add(flat)
    res, t_batch, all_batch = timed(lambda: idx.sort_similar(ids, descs, p, set_first=first), reps)
    row = {"bench": "sort_similar_color_batch", "sets": n_sets, "set_n": set_n, "queries": sum(r[1] for r in res),
           "batch_ms": round(t_batch * 1e3, 3), "batch_ms_all": [round(x * 1e3, 3) for x in all_batch]}
    row.update(stages(lambda: idx.sort_similar(ids, descs, p, set_first=first)))
    py, t_py, _ = timed(lambda: sort_similar_batch(idx, sets, p), reps)
    assert [ids_of(r) for r in py] == [(r[0], r[1], r[2]) for r in res], "the Python entry and the C-ABI differ"
    t0 = time.perf_counter()
    assert ids_of(sort_similar(idx, media_of(descs[:set_n], 1), p, batched=False)) == ids_of(py[0]), "the batch and the loop differ"
    t_loop = (time.perf_counter() - t0) * n_sets
    row.update(python_entry_ms=round(t_py * 1e3, 3), loop_ms=round(t_loop * 1e3, 1), loop_estimated=True,
               loop_over_batch=round(t_loop / t_py, 1))
    emit(row)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
