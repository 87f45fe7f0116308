"""The video segments (cbh_video_segments, cbird_amd/csrc/vsegments.hip): whole host-entry calls at max_segments 1 and 4
beside cbh_video_coverage on the SAME pairs in the same process -- the yardstick: a segments call with one segment makes
coverage's comparisons twice, once for the supports and once for the members -- and against the NumPy model
(tests/video_segments_rules.py).

    python tools/video_segments_bench.py [shapes=long,square,ragged] [thresh=5] [tol=15] [min_frames=3] [reps=5]
                                         [sample=16] [verify=1]

The shapes are tools/video_coverage_bench.py's: one pair of 50 000 x 50 000 stored frames, 1024 pairs of 2 000 x 2 000,
4096 ragged pairs over 512 shared videos.  Equal results are asserted before anything is reported: every summary field,
segment record and map entry at both max_segments, for `long` the whole pair, for the batches the first `sample` pairs
and `sample` more spread evenly (the row says how many).  Host clock around calls that end in a stream synchronise;
warm-up first; medians of `reps`.  verify=0 is for a run under `rocprofv3 --kernel-trace --stats`, a run of its own: the
kernels' times come from its trace.  One JSON line per shape (profiles/video_segments.jsonl keeps them)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import video_segments_rules as SR  # noqa: E402
from video_coverage_bench import shape_of, timed  # noqa: E402
from cbird_amd import _lib, require_device  # noqa: E402
from cbird_amd.video import (VCOVER_DTYPE, VCOVER_FRAME_DTYPE, VSEGMENT_DTYPE, VSEGMENT_FRAME_DTYPE,  # noqa: E402
                             VSEGMENTS_DTYPE)


def main():
    kv = dict(a.split("=") for a in sys.argv[1:])
    shapes = kv.get("shapes", "long,square,ragged").split(",")
    thresh, tol, least = int(kv.get("thresh", 5)), int(kv.get("tol", 15)), int(kv.get("min_frames", 3))
    reps, sample, verify = int(kv.get("reps", 5)), int(kv.get("sample", 16)), int(kv.get("verify", 1))
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
        offs = np.zeros(len(p) + 1, np.uint64)

        # the yardstick: the coverage map of the same pairs
        csums = np.zeros(len(p), VCOVER_DTYPE)
        one = np.zeros(1, VCOVER_FRAME_DTYPE)

        def cover(m, cap):
            return L.cbh_video_coverage(0, f.ctypes.data, h.ctypes.data, o.ctypes.data, len(videos), p.ctypes.data, len(p),
                                        thresh, 0, csums.ctypes.data, None if m is None else m.ctypes.data, cap,
                                        offs.ctypes.data)

        assert cover(one, 0) == _lib.CBH_E_OVERFLOW
        cmap = np.zeros(int(offs[-1]), VCOVER_FRAME_DTYPE)
        rc, t_cover, all_cover = timed(lambda: cover(cmap, len(cmap)), reps)
        assert rc == 0
        comparisons = int(sum(int(s["n_src"]) * int(s["n_dst"]) for s in csums))

        fmap = np.zeros(int(offs[-1]), VSEGMENT_FRAME_DTYPE)
        row = {"bench": "video_segments", "shape": name, "pairs": len(pairs), "videos": len(videos), "frames": int(len(f)),
               "thresh": thresh, "tol": tol, "min_frames": least, "comparisons": comparisons, "map_entries": int(offs[-1]),
               "coverage_call_ms": round(t_cover * 1e3, 3), "coverage_call_ms_all": [round(x * 1e3, 3) for x in all_cover]}
        check = list(range(len(pairs))) if len(pairs) <= 2 * sample else sorted(
            set(range(sample)) | set(np.linspace(0, len(pairs) - 1, sample).astype(int).tolist()))
        for most in (1, 4):
            sums = np.zeros(len(p), VSEGMENTS_DTYPE)
            segs = np.zeros(len(p) * most, VSEGMENT_DTYPE)

            def call(m):
                return L.cbh_video_segments(0, f.ctypes.data, h.ctypes.data, o.ctypes.data, len(videos), p.ctypes.data,
                                            len(p), thresh, 0, tol, least, most, sums.ctypes.data, segs.ctypes.data,
                                            None if m is None else m.ctypes.data, len(fmap), offs.ctypes.data)

            rc, t_map, all_map = timed(lambda: call(fmap), reps)
            assert rc == 0
            with_map = (sums.copy(), segs.copy())
            rc, t_bare, _ = timed(lambda: call(None), reps)
            assert rc == 0 and (sums.tobytes(), segs.tobytes()) == (with_map[0].tobytes(), with_map[1].tobytes())
            key = f"max_segments_{most}"
            row[key] = {"call_ms": round(t_map * 1e3, 3), "call_ms_all": [round(x * 1e3, 3) for x in all_map],
                        "no_map_ms": round(t_bare * 1e3, 3), "call_over_coverage_call": round(t_map / t_cover, 2),
                        "segments": int(sums["n_segments"].sum()), "aligned_frames": int(sums["n_aligned"].sum()),
                        "pairs_with_a_segment": int((sums["n_segments"] > 0).sum())}
            if not verify:
                continue
            t_host = 0.0
            for k in check:
                a, b = pairs[k]
                t0 = time.perf_counter()
                s, found, frames, dframes, dist, seg = SR.segments(videos[a], videos[b], thresh, 0, tol, least, most)
                t_host += time.perf_counter() - t0
                assert {n: int(sums[k][n]) for n in SR.SUMMARY_FIELDS} == s, f"pair {k}: the summaries differ"
                got = [{n: int(g[n]) for n in SR.SEGMENT_FIELDS} for g in segs[k * most:(k + 1) * most]]
                assert got == found + [dict.fromkeys(SR.SEGMENT_FIELDS, 0)] * (most - len(found)), f"pair {k}: the segments differ"
                m = fmap[int(offs[k]):int(offs[k + 1])]
                assert (m["src_frame"].tolist(), m["dst_frame"].tolist(), m["distance"].tolist(), m["segment"].tolist()) == \
                    (frames.tolist(), dframes.tolist(), dist.tolist(), seg.tolist()), f"pair {k}: the maps differ"
            row[key].update(pairs_compared_with_numpy=len(check), numpy_ms_for_those=round(t_host * 1e3, 1), equal=True)
        row["verified"] = bool(verify)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
