"""Same calls, same work: a fixed list of CvFeaturesIndex calls (knn, radius_match, find_batch, and a radius search whose
records outgrow the first block) on a plain handle and on one over mask 1 x 3 shards, under each of the three 256-bit scan
paths ("scan256_mfma" 2 + "scan256_small" 1, 2 + 0, 0), for comparing two BUILDS of the library.  Each build runs in a fresh
process under the tracer; the driver puts a hipDriverGetVersion call (which the library never makes) in front of every call,
so the report can cut the traces per call.

    rocprofv3 --kernel-trace --hip-trace --stats --output-format csv -d out/sc_new -- python3 tools/ab/scan256_same_calls.py run out/sc_new/calls.jsonl
    CBH_LIB_PATH=... rocprofv3 ... -d out/sc_parent -- python3 tools/ab/scan256_same_calls.py run out/sc_parent/calls.jsonl
    python3 tools/ab/scan256_same_calls.py report out/sc_parent out/sc_new

Per call the report prints: return code, total, a hash of every result array, the cbh_idx256_get_stats and
cbh_idx256_shard_stats deltas; the kernels (name grid/workgroup) counted, with a hash of their sequence in launch order; the
HIP API calls by name (push / pop = __hipPush/PopCallConfiguration; hipStreamQuery and hipEventQuery left out: polled).  A
line is printed once where the two builds agree; where they differ the first build's line is followed by a "second:" line.
"""
import collections, csv, glob, hashlib, json, os, re, sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
PATHS = {"mfma": (2, 1), "mfma_rows": (2, 0), "valu": (0, 1)}


def run(out_path):
    import ctypes as C
    import numpy as np
    import scan256_layout as S
    from cbird_amd import _lib
    from cbird_amd._lib import cbh_match

    L = _lib.lib()
    hip = L  # (dlsym on the library's handle also finds the HIP runtime it is linked against: the same one the tracer sees)
    ver = C.c_int(0)
    rng = np.random.default_rng(77)
    rows = rng.integers(0, 256, (120 * 300, 32), dtype=np.uint8)  # three runs of 16384 rows: every shard holds rows
    dense = S.build("dense", 40)
    q300 = rows[5:305].copy()
    q300[::2, 3] ^= 0x21
    q2000 = rows[::17][:2000].copy()
    q2000[::3, 9] ^= 0x11
    offs = np.arange(0, 8 * 60 + 1, 60, dtype=np.uint64)

    def handle(shards, data, per):
        h = L.cbh_idx256_create_sharded(*shards) if shards else L.cbh_idx256_create(0)
        assert h
        for i in range(0, len(data), per):
            _lib.check(L.cbh_idx256_add(h, i // per + 1, data[i:i + per].ctypes.data, min(per, len(data) - i)), "add")
        return h

    def stats(h):
        a, b = _lib.cbh_stats(), _lib.cbh_shard_stats()
        L.cbh_idx256_get_stats(h, C.byref(a))
        L.cbh_idx256_shard_stats(h, C.byref(b))
        return dict(launches=a.scan_launches, pairs=a.scan_pairs, scans=b.scans, rescans=b.rescans, collectives=b.collectives,
                    peer_copies=b.peer_copies, local_copies=b.local_copies)

    def knn(h, q, k, thresh):
        r, d, c = np.zeros((len(q), k), np.uint32), np.zeros((len(q), k), np.uint16), np.zeros(len(q), np.uint32)
        rc = L.cbh_idx256_knn(h, q.ctypes.data, len(q), k, thresh, r.ctypes.data, d.ctypes.data, c.ctypes.data)
        return rc, int(c.sum()), (r, d, c)

    def radius(h, q, max_dist, cap):
        out, first = np.zeros((cap, 3), np.int32), np.zeros(len(q) + 1, np.uint64)
        rc = L.cbh_idx256_radius_match(h, q.ctypes.data, len(q), max_dist, out.ctypes.data, cap, first.ctypes.data)
        return rc, int(first[-1]), (out[:min(cap, int(first[-1]))], first)

    def find_batch(h, q, thresh, k):
        cap = len(q) * k + 1
        buf, oo = (cbh_match * cap)(), np.zeros(len(offs), np.uint64)
        rc = L.cbh_idx256_find_batch(h, q.ctypes.data, offs.ctypes.data, len(offs) - 1, thresh, k, buf, cap, oo.ctypes.data)
        return rc, int(oo[-1]), (np.frombuffer(buf, np.uint8, int(oo[-1]) * C.sizeof(cbh_match)), oo)

    with open(out_path, "w") as f:
        for path, (mfma, small) in PATHS.items():
            assert L.cbh_set_tuning(b"scan256_mfma", mfma) == 0 and L.cbh_set_tuning(b"scan256_small", small) == 0
            for kind, shards in (("plain", None), ("sharded3", (1, 3))):
                h, hd = handle(shards, rows, 300), handle(shards, dense.rows, 256)
                calls = (("knn300", h, lambda: knn(h, q300, 6, 30)), ("knn2000", h, lambda: knn(h, q2000, 10, 25)),
                         ("knn2000_t41", h, lambda: knn(h, q2000, 10, 41)), ("radius300", h, lambda: radius(h, q300, 29, 1 << 16)),
                         ("find_batch8x60", h, lambda: find_batch(h, q300[:480].copy(), 25, 10)),
                         ("radius_regrow", hd, lambda: radius(hd, dense.needles, 39, len(dense.rows) * len(dense.needles))),
                         ("knn_after_regrow", hd, lambda: knn(hd, dense.needles[:64].copy(), 10, 40)))
                for name, hh, call in calls:
                    s0 = stats(hh)
                    hip.hipDriverGetVersion(C.byref(ver))  # the marker in front of the call
                    rc, total, arrays = call()
                    s1 = stats(hh)
                    sha = hashlib.sha1()
                    for a in arrays:
                        sha.update(np.ascontiguousarray(a).tobytes())
                    f.write(json.dumps(dict(call=f"{path} {kind} {name}", rc=rc, total=total, hash=sha.hexdigest()[:16],
                                            stats={k: int(s1[k] - s0[k]) for k in s0})) + "\n")
                hip.hipDriverGetVersion(C.byref(ver))  # ... and behind the last one, in front of the destroys
                L.cbh_idx256_destroy(h)
                L.cbh_idx256_destroy(hd)
        L.cbh_set_tuning(b"scan256_mfma", 1)
        L.cbh_set_tuning(b"scan256_small", 1)


def _rows(d, pattern):
    out = []
    for p in glob.glob(os.path.join(d, "**", pattern), recursive=True):
        with open(p, newline="") as f:
            out += list(csv.DictReader(f))
    return out


def _short(name):
    name = re.sub(r"\(anonymous namespace\)::|cbh::|^void ", "", name.strip('"'))
    m = re.match(r"([\w:]+(?:<[^(]*?>)?)\s*\(", name)
    return m.group(1) if m else name.split("(")[0]


def _dims(r, key):
    v = [int(r[f"{key}_{a}"]) for a in "XYZ"]
    return "x".join(str(x) for x in (v if v[2] > 1 else v[:2] if v[1] > 1 else v[:1]))


def load(d):
    """-> list of (call record, kernels line, hip api line), one per driver call"""
    calls = [json.loads(l) for l in open(os.path.join(d, "calls.jsonl"))]
    api = sorted(_rows(d, "*hip_api_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    marks = [int(r["Start_Timestamp"]) for r in api if r["Function"] == "hipDriverGetVersion"]
    kernels = sorted(_rows(d, "*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    out, m = [], 0
    for c in calls:
        t0, t1 = marks[m], marks[m + 1]
        m += 1 if not c["call"].endswith("knn_after_regrow") else 2  # (the marker in front of the destroys)
        names = collections.Counter()
        for r in api:
            if t0 < int(r["Start_Timestamp"]) < t1 and r["Function"] not in ("hipStreamQuery", "hipEventQuery"):
                names[{"__hipPushCallConfiguration": "push", "__hipPopCallConfiguration": "pop"}.get(r["Function"], r["Function"])] += 1
        seq = [f"{_short(r['Kernel_Name'])} {_dims(r, 'Grid_Size')}/{_dims(r, 'Workgroup_Size')}" for r in kernels
               if t0 < int(r["Start_Timestamp"]) < t1]
        cnt = collections.Counter(seq)
        kline = (f"kernels {len(seq)}, sha1 of the sequence in launch order {hashlib.sha1(chr(10).join(seq).encode()).hexdigest()[:16]}: "
                 + ", ".join(f"{n} x {k}" for k, n in sorted(cnt.items())))
        out.append((c, kline, "hip api: " + ", ".join(f"{k} {n}" for k, n in sorted(names.items()))))
    return out


def report(da, db):
    a, b = load(da), load(db)
    assert [x[0]["call"] for x in a] == [x[0]["call"] for x in b]
    differing = 0
    for (ca, ka, ha), (cb, kb, hb) in zip(a, b):
        head = lambda c: (f"rc {c['rc']} total {c['total']} hash {c['hash']} stats "
                          + ", ".join(f"{k}: {v}" for k, v in c["stats"].items()))
        print(f"== {ca['call']}: {head(ca)}")
        if head(ca) != head(cb):
            print(f"   second: {head(cb)}")
        for x, y in ((ka, kb), (ha, hb)):
            print(f"   {x}")
            if x != y:
                print(f"   second: {y}")
        differing += (head(ca), ka, ha) != (head(cb), kb, hb)
    print(f"# {len(a)} calls, {differing} with a difference")


if __name__ == "__main__":
    run(sys.argv[2]) if sys.argv[1] == "run" else report(sys.argv[2], sys.argv[3])
