"""The video coverage map (cbh_video_coverage, cbird_amd/csrc/vcoverage.hip): whole host-entry calls -- uploads, both
kernels, the download -- against a NumPy brute force of the same definitions (tests/video_coverage_rules.py) in the same
run.  The parent commit has no coverage call, so the brute force is what a user would have written.

    python tools/video_coverage_bench.py [shapes=long,square,ragged] [thresh=5] [reps=5] [sample=16] [verify=1]

  long     one pair of two videos of 50 000 stored frames: a GUESS at a feature film after the indexer's de-duplication
           (a 2 h film has some 170 000 frames; how many survive depends on the film), not a measured length
  square   1024 pairs of 2 000 x 2 000, every video named once
  ragged   4096 pairs over 512 shared videos of 30 - 3 000 frames

Videos are random walks (0-3 bit flips a frame, gaps 1-9); a destination is a noisy cut of its source or an unrelated
walk.  Equal results are asserted before anything is reported: every summary field and every map entry, for `long` the
whole pair, for `square` and `ragged` the first `sample` pairs and `sample` more spread evenly over the batch (the
brute force would take minutes on all of them; the row says how many were compared).  Host clock around calls that end
in a stream synchronise; warm-up first; medians of `reps`.  A comparison is one (considered source frame, destination
entry) pair.  SCAN_RATE is the project's own full 64-bit threshold scan on the matrix cores, for scale: it answers
another question (all pairs under a threshold, not the nearest), so the two rates are not a ranking.  One JSON line per
shape (profiles/video_coverage.jsonl keeps them)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_coverage_rules as VR  # noqa: E402
from cbird_amd import _lib, require_device  # noqa: E402
from cbird_amd.video import VCOVER_DTYPE, VCOVER_FRAME_DTYPE  # noqa: E402

SCAN_RATE = 6.2e13  # FULL3, 16.1 ms per 10^12 pairs: profiles/r06_bench_under_kernel_trace.json


def walk(n, rng):
    nflip = rng.integers(0, 4, n)
    step = np.zeros(n, np.uint64)
    for k in range(3):
        step ^= np.where(nflip > k, np.uint64(1) << rng.integers(1, 64, n).astype(np.uint64), np.uint64(0))
    step[0] = rng.integers(0, 2**63, dtype=np.uint64)
    gaps = rng.integers(1, 10, n)
    gaps[0] = 0
    return np.cumsum(gaps).astype(np.int32), np.bitwise_xor.accumulate(step)


def noisy_cut(video, rng):
    f, h = video
    n = len(f)
    a = int(rng.integers(0, max(1, n // 3)))
    b = int(rng.integers(min(n, a + n // 2), n + 1))
    hh = h[a:b] ^ np.where(rng.random(b - a) < 0.3, np.uint64(1) << rng.integers(1, 64, b - a).astype(np.uint64), np.uint64(0))
    return (f[a:b] - f[a]).astype(np.int32), hh


def shape_of(name, rng):
    if name == "long":
        a = walk(50000, rng)
        b = walk(50000, rng)
        cut = noisy_cut(a, rng)
        m = len(cut[0]) // 2  # half of a's cut spliced into the middle of an unrelated film
        b = (b[0], np.concatenate([b[1][:20000], cut[1][:m], b[1][20000 + m:]])[:50000])
        return [a, b], [(0, 1)]
    if name == "square":
        videos = []
        for _ in range(1024):  # half of the destinations are noisy copies, half unrelated
            a = walk(2000, rng)
            noisy = (a[0], a[1] ^ np.where(rng.random(2000) < 0.3, np.uint64(2), np.uint64(0)))
            videos += [a, noisy if rng.random() < 0.5 else walk(2000, rng)]
        return videos, [(2 * k, 2 * k + 1) for k in range(1024)]
    videos = [walk(int(rng.integers(30, 3001)), rng) for _ in range(384)]
    videos += [noisy_cut(videos[int(rng.integers(0, 384))], rng) for _ in range(128)]
    return videos, [(int(a), int(b)) for a, b in rng.integers(0, 512, (4096, 2))]


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
    shapes = kv.get("shapes", "long,square,ragged").split(",")
    thresh, reps, sample = int(kv.get("thresh", 5)), int(kv.get("reps", 5)), int(kv.get("sample", 16))
    verify = int(kv.get("verify", 1))
    require_device()
    L = _lib.lib()
    rng = np.random.default_rng(2025)
    for name in shapes:
        videos, pairs = shape_of(name, rng)
        f = np.concatenate([v[0] for v in videos])
        h = np.concatenate([v[1] for v in videos])
        o = np.zeros(len(videos) + 1, np.uint64)
        np.cumsum([len(v[0]) for v in videos], out=o[1:])
        p = np.ascontiguousarray(np.asarray(pairs, np.uint32))
        sums = np.zeros(len(p), VCOVER_DTYPE)
        offs = np.zeros(len(p) + 1, np.uint64)
        one = np.zeros(1, VCOVER_FRAME_DTYPE)

        def call(m, cap):
            return L.cbh_video_coverage(0, f.ctypes.data, h.ctypes.data, o.ctypes.data, len(videos), p.ctypes.data, len(p),
                                        thresh, 0, sums.ctypes.data, None if m is None else m.ctypes.data, cap,
                                        offs.ctypes.data)

        assert call(one, 0) == _lib.CBH_E_OVERFLOW
        fmap = np.zeros(int(offs[-1]), VCOVER_FRAME_DTYPE)
        rc, t_map, all_map = timed(lambda: call(fmap, len(fmap)), reps)
        assert rc == 0
        with_map = sums.copy()
        rc, t_sum, all_sum = timed(lambda: call(None, 0), reps)
        assert rc == 0 and sums.tobytes() == with_map.tobytes()
        comparisons = int(sum(int(s["n_src"]) * int(s["n_dst"]) for s in sums))

        # the brute force, on the pairs it can take in reasonable time, each held against the device's answer
        if not verify:  # (a run under the profiler: the kernels' own times are wanted, nothing is reported)
            print(json.dumps({"bench": "video_coverage", "shape": name, "comparisons": comparisons, "verified": False,
                              "call_ms": round(t_map * 1e3, 3)}), flush=True)
            continue
        check = list(range(len(pairs))) if len(pairs) <= 2 * sample else sorted(
            set(range(sample)) | set(np.linspace(0, len(pairs) - 1, sample).astype(int).tolist()))
        t_host, host_cmp = 0.0, 0
        for k in check:
            a, b = pairs[k]
            t0 = time.perf_counter()
            s, frames, dframes, dist = VR.coverage(videos[a], videos[b], thresh, 0)
            t_host += time.perf_counter() - t0
            host_cmp += s["n_src"] * s["n_dst"]
            assert {n: int(sums[k][n]) for n in VR.FIELDS} == s, f"pair {k}: the summaries differ"
            m = fmap[int(offs[k]):int(offs[k + 1])]
            assert (m["src_frame"].tolist(), m["dst_frame"].tolist(), m["distance"].tolist()) == \
                (frames.tolist(), dframes.tolist(), dist.tolist()), f"pair {k}: the maps differ"
        row = {"bench": "video_coverage", "shape": name, "pairs": len(pairs), "videos": len(videos), "frames": int(len(f)),
               "thresh": thresh, "comparisons": comparisons, "map_entries": int(offs[-1]),
               "covered_frames": int(sums["n_covered"].sum()), "call_ms": round(t_map * 1e3, 3),
               "call_ms_all": [round(x * 1e3, 3) for x in all_map], "summaries_only_ms": round(t_sum * 1e3, 3),
               "summaries_only_ms_all": [round(x * 1e3, 3) for x in all_sum],
               "comparisons_per_s": round(comparisons / t_map, 0), "summaries_only_comparisons_per_s": round(comparisons / t_sum, 0),
               "pairs_compared_with_numpy": len(check), "numpy_ms_for_those": round(t_host * 1e3, 1),
               "numpy_comparisons_per_s": round(host_cmp / t_host, 0),
               "numpy_ms_whole_shape_estimated": round(t_host * comparisons / max(1, host_cmp) * 1e3, 1),
               "equal": True, "scan_full64_comparisons_per_s": SCAN_RATE}
        row["numpy_over_call"] = round(row["numpy_ms_whole_shape_estimated"] / row["call_ms"], 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
