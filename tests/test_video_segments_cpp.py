"""The segments drop-in (GpuDctVideoIndex::gpuSegments, cbird_amd/cpp/gpu_indexes.h): tests/cpp/test_video_segments.cpp
compiles against the mock cbird headers (CPU) and, on the MI355X, reproduces the model on the 12-clip set -- the videos
written as .vdx files and loaded the way cbird loads them, with maps and without."""
import os
import subprocess

import numpy as np
import pytest

import video_coverage_rules as VR
import video_segments_rules as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_video_segments")


def _build_cpp():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_video_segments.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"),
                           "-lcbird_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_dropin_compiles():
    _build_cpp()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_indexes.h")).read()
    assert "bool gpuSegments(const std::vector<std::pair<uint32_t, uint32_t>>& pairs, const SearchParams& p," in src


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [0, 20])
def test_dropin_runs_on_gpu(gpu, tmp_path, skip):
    clips = VR.clips()
    pairs = [(a, b) for a in range(1, 13) for b in range(1, 13)]
    tol, min_frames, max_segments = 15, 3, 4
    path = tmp_path / "clips.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(clips), 5, skip, len(pairs), tol, min_frames, max_segments], np.int32).tobytes())
        for frames, hashes in clips:
            f.write(np.int32(len(frames)).tobytes() + np.asarray(frames, np.int32).tobytes()
                    + np.asarray(hashes, np.uint64).tobytes())
        f.write(np.array(pairs, np.int32).tobytes())
    _build_cpp()
    out = subprocess.run([EXE, str(path), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 4 * len(pairs) + 1 and lines[-1] == "done"
    with_segments = 0
    for k, (a, b) in enumerate(pairs):
        s, segs, frames, dframes, dist, seg = SR.segments(clips[a - 1], clips[b - 1], 5, skip, tol, min_frames, max_segments)
        summary = [str(s[name]) for name in SR.SUMMARY_FIELDS]
        assert lines[3 * k].split() == ["pair", str(k), str(s["src_in"]), str(s["dst_in"]), str(s["len"])] + summary, (a, b)
        assert lines[3 * k + 1].split() == [":".join(str(g[n]) for n in SR.SEGMENT_FIELDS) for g in segs], (a, b)
        assert lines[3 * k + 2].split() == [f"{w}:{x}:{y}:{z}" for w, x, y, z in zip(frames, dframes, dist, seg)], (a, b)
        assert lines[3 * len(pairs) + k].split() == ["bare", str(k)] + summary, (a, b)
        with_segments += bool(segs) and a != b
    assert with_segments >= 8  # the four sub-clips and their sources, both ways
