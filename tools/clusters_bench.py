"""Clusters of a DctHashIndex on the device (cbh_idx64_clusters / cbh_idx64_cluster_labels, clusters.hip) against the
host route that exists without them: every entry through cbh_idx64_find_batch, the pairs into
scipy.sparse.csgraph.connected_components (the union-find of tests/clusters_rules.py if scipy does not import).

    python tools/clusters_bench.py [n=10000,100000,1000000] [dht=5,8] [data=synth,walk] [reps=5] [out=profiles/clusters.jsonl]

Data: cbird_amd.synth.make_hashes as bench.py makes them (uniform hashes, 5 % planted neighbours), and a shuffled random
walk of 0-3 flipped bits per step (tools/sort_similar_bench.py's set; one long chain of near-duplicates).
Per (data, n, dht): labels and nearest of the device must EQUAL the host route's -- asserted before anything is timed;
then the median of `reps` whole cbh_idx64_clusters calls (host clock, after a warm-up), the scans' share of one call from
cbh_idx64_get_stats, the node table / hook + flatten / output shares from events ("cluster_timing", a run of its own: it
waits after every stage), the host route's time, and at n <= 10000 similar(mergeGroups=1): its time and how many of its
groups share a member with another group (its groups differ from clusters by design).  One JSON line per result, appended
to `out`."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from cbird_amd import DctHashIndex, Media, SearchParams, _lib, require_device, synth  # noqa: E402
from cbird_amd.database import similar  # noqa: E402


def walk(n, seed):
    """each hash is the one before with 0-3 random bits flipped (positions may coincide), shuffled; ids 1..n"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 64, (n, 3)).astype(np.uint64)
    k = rng.integers(0, 4, n)
    step = np.zeros(n, np.uint64)
    for j in range(3):
        step ^= np.where(k > j, np.uint64(1) << bits[:, j], np.uint64(0))
    step[0] = np.uint64(rng.integers(1, 1 << 63))
    h = np.bitwise_xor.accumulate(step)
    h[h == 0] = np.uint64(1)
    rng.shuffle(h)
    return h, np.arange(1, n + 1, dtype=np.uint32)


def host_route(idx, h, ids, dht):
    """(label, nearest) per entry in id order (ids are 1..n in slot order here) from find_batch + connected components"""
    n = len(h)
    k = 16
    mi, ms, mc = idx.find_batch(h, dht, k)
    rows = [np.repeat(np.arange(n), np.minimum(mc, k))]
    sel = np.arange(k)[None, :] < np.minimum(mc, k)[:, None]
    cols, scores = [mi[sel].astype(np.int64) - 1], [ms[sel]]
    more = np.nonzero(mc > k)[0]
    if len(more):  # the few with more matches than that: all of theirs
        kk = int(mc[more].max())
        mi2, ms2, mc2 = idx.find_batch(h[more], dht, kk)
        sel2 = np.arange(kk)[None, :] < mc2[:, None]
        keep = ~np.isin(rows[0], more)
        rows, cols, scores = [rows[0][keep]], [cols[0][keep]], [scores[0][keep]]
        rows.append(np.repeat(more, mc2))
        cols.append(mi2[sel2].astype(np.int64) - 1)
        scores.append(ms2[sel2])
    r, c, s = np.concatenate(rows), np.concatenate(cols), np.concatenate(scores)
    other = r != c
    r, c, s = r[other], c[other], s[other]
    nearest = np.full(n, 0xFF, np.int64)
    np.minimum.at(nearest, r, s)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components

        _, comp = connected_components(coo_matrix((np.ones(len(r), np.int8), (r, c)), shape=(n, n)), directed=False)
        how = "scipy"
    except ImportError:
        from clusters_rules import _find

        parent = list(range(n))
        for a, b in zip(r.tolist(), c.tolist()):
            ra, rb = _find(parent, a), _find(parent, b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        comp, how = np.array([_find(parent, x) for x in range(n)]), "union-find"
    first = np.full(comp.max() + 1, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return ids[first[comp]], nearest.astype(np.uint8), len(r) // 2, how


def tuning(L, key):
    v = C.c_longlong(0)
    assert L.cbh_get_tuning(key, C.byref(v)) == 0
    return v.value


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    sizes = [int(x) for x in kv.get("n", "10000,100000,1000000").split(",")]
    dhts = [int(x) for x in kv.get("dht", "5,8").split(",")]
    kinds = kv.get("data", "synth,walk").split(",")
    reps, out_path = int(kv.get("reps", 5)), kv.get("out", "profiles/clusters.jsonl")
    require_device()
    L = _lib.lib()
    for kind in kinds:
        for n in sizes:
            h, ids = synth.make_hashes(n, seed=1234) if kind == "synth" else walk(n, 2024)
            idx = DctHashIndex()
            idx.load(h, ids)
            for dht in dhts:
                t0 = time.perf_counter()
                want_label, want_near, edges, how = host_route(idx, h, ids, dht)
                t_host = time.perf_counter() - t0
                got_ids, got_label, got_near = idx.cluster_labels(dht)
                equal = bool(np.array_equal(got_ids, ids) and np.array_equal(got_label, want_label)
                             and np.array_equal(got_near, want_near))
                assert equal, f"{kind} n={n} dht={dht}: the device's labels differ from the host route's"
                # the clusters call with room for its result, whole host-entry calls
                st = _lib.cbh_cluster_stats()
                nc, nm = C.c_size_t(0), C.c_size_t(0)
                first, members = np.zeros(1, np.uint64), np.zeros((1, 2), np.uint32)

                def call():
                    return L.cbh_idx64_clusters(idx.handle, dht, 2, first.ctypes.data, len(first) - 1, members.ctypes.data,
                                                len(members) if nm.value else 0, C.byref(nc), C.byref(nm), C.byref(st))

                assert call() in (0, _lib.CBH_E_OVERFLOW)
                first, members = np.zeros(nc.value + 1, np.uint64), np.zeros((max(nm.value, 1), 2), np.uint32)
                assert call() == 0  # warm-up, with room
                sizes_got = np.diff(first.astype(np.int64))
                _, cnt = np.unique(want_label, return_counts=True)
                assert sorted(sizes_got.tolist()) == sorted(cnt[cnt >= 2].tolist())
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    assert call() == 0
                    ts.append(time.perf_counter() - t0)
                L.cbh_idx64_reset_stats(idx.handle)
                assert call() == 0
                scan = _lib.cbh_stats()
                L.cbh_idx64_get_stats(idx.handle, C.byref(scan))
                L.cbh_set_tuning(b"cluster_timing", 1)
                try:
                    assert call() == 0
                    stage_us = [tuning(L, k) for k in (b"cluster_table_us", b"cluster_hook_us", b"cluster_emit_us")]
                finally:
                    L.cbh_set_tuning(b"cluster_timing", 0)
                t_dev = statistics.median(ts)
                row = {"bench": "clusters", "data": kind, "n": n, "dht": dht, "equal": equal, "host_components_by": how,
                       "edges": edges, "records": int(st.records), "chunks": int(st.chunks), "rescans": int(st.rescans),
                       "clusters": int(st.clusters), "members": int(st.members), "largest": int(sizes_got.max(initial=0)),
                       "device_ms": round(t_dev * 1e3, 3), "device_ms_all": [round(x * 1e3, 3) for x in ts],
                       "scan_ms": round(scan.scan_ms, 3), "scan_launches": int(scan.scan_launches),
                       "table_ms": round(stage_us[0] / 1e3, 3), "hook_flatten_ms": round(stage_us[1] / 1e3, 3),
                       "emit_ms": round(stage_us[2] / 1e3, 3), "host_route_ms": round(t_host * 1e3, 1),
                       "host_over_device": round(t_host / t_dev, 1)}
                if n <= 10000:
                    media = [Media(id=int(i), dctHash=int(x), path=f"/db/{int(i):08d}.jpg") for i, x in zip(ids, h)]
                    t0 = time.perf_counter()
                    groups = similar(idx, media, SearchParams(dctThresh=dht, mergeGroups=1))
                    t_merge = time.perf_counter() - t0
                    seen = {}
                    for g, grp in enumerate(groups):
                        for m in grp:
                            seen.setdefault(m.id, []).append(g)
                    overlapping = {g for gs in seen.values() if len(gs) > 1 for g in gs}
                    row.update(merge_route_ms=round(t_merge * 1e3, 1), merge_groups=len(groups),
                               merge_groups_overlapping=len(overlapping))
                print(json.dumps(row), flush=True)
                with open(out_path, "a") as f:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
