"""Same-box A/B of two BUILDS of the library (a kernel changed in source, not behind a knob): child processes alternate
between cbird_amd/libcbird_hip.so and another file (default cbird_amd/libcbird_hip.so.prev, built from an earlier
commit's source and linked with the current objects), each timing the 1M x 1M scan at the given thresholds on the bench's
image-derived hashes.  Box-to-box variance on this pool is +-4 %; only alternation on one box resolves a 2 % change.
Each child also reports which prefilter its launches took ("scan_pre_mask" | "scan_pre48_mask" | "scan_pre16_mask").
The first child that exits non-zero or prints no result line ends the run: nothing more is started on that card.
`needles` < 1M scans only the first so many hashes against the 1M slots (threshold 65 matches every pair: 10^12 at 1M x 1M).
    python tools/ab/lib_ab.py [rounds=3] [thresholds=2,5,6,7] [other=cbird_amd/libcbird_hip.so.prev] [needles=1000000]"""
import json, os, subprocess, sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, ".")
from cbird_amd import _lib
if sys.argv[1] != "-":
    _lib.LIB_PATH = sys.argv[1]
import torch, cbird_amd, bench
L = _lib.lib()
N = 1000000
T = [int(x) for x in sys.argv[2].split(",")]
NQ = int(sys.argv[3])
dev = torch.device("cuda", 0)
out = torch.empty(N, dtype=torch.int64, device=dev)
for c0 in range(0, N, 100000):
    c1 = min(N, c0 + 100000)
    imgs = bench.gen_images(torch, dev, c0, c1, N, 1234)
    _lib.check(L.cbh_dcthash_batch_dev(imgs.data_ptr(), c1 - c0, 256, 256, 256, 65536, out[c0:].data_ptr(), 0, None), "h")
    del imgs
idx = cbird_amd.DctHashIndex(); ids = torch.arange(1, N + 1, dtype=torch.int32, device=dev)
idx.load_device(out.data_ptr(), ids.data_ptr(), N)
cap = 1 << 25
drec = torch.empty(cap, dtype=torch.int64, device=dev); dtot = torch.zeros(1, dtype=torch.int64, device=dev)
ms = C.c_float(0)
res = {}
for rep in range(3):
    for t in T:
        _lib.check(L.cbh_idx64_time_scan_dev(idx.handle, out.data_ptr(), NQ, t, drec.data_ptr(), cap, dtot.data_ptr(), 4, C.byref(ms)), "t")
        res.setdefault(str(t), []).append(round(ms.value, 3))
v = C.c_longlong(0)
for key in ("scan_pre_mask", "scan_pre48_mask", "scan_pre16_mask"):
    _lib.check(L.cbh_get_tuning(key.encode(), C.byref(v)), key)
    res[key] = [v.value]
print(json.dumps({k: min(v) for k, v in res.items()}))
'''


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    thr = sys.argv[2] if len(sys.argv) > 2 else "2,5,6,7"
    other = os.path.abspath(sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "cbird_amd", "libcbird_hip.so.prev"))
    needles = sys.argv[4] if len(sys.argv) > 4 else "1000000"
    out = {"this": [], "other": []}
    for _ in range(rounds):
        for name, path in (("this", "-"), ("other", other)):
            r = subprocess.run([sys.executable, "-c", CHILD, path, thr, needles], cwd=ROOT, capture_output=True, text=True,
                               timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                sys.exit(f"lib_ab: the child on {name} exited {r.returncode} without a result; stopped.\n{r.stderr[-2000:]}")
            out[name].append(json.loads(line[-1]))
    best = {n: {t: min(x[t] for x in v if t in x) for t in thr.split(",")} for n, v in out.items()}
    print(json.dumps({"needles": int(needles), "min_ms": best, "ratio_this_over_other": {t: round(best["this"][t] / best["other"][t], 4) for t in thr.split(",")},
                      "runs": out}))


if __name__ == "__main__":
    main()
