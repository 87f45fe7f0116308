"""The clusters drop-in (GpuDctHashIndex::gpuClusters, cbird_amd/cpp/gpu_dcthashindex.h): tests/cpp/test_clusters.cpp
compiles against the mock cbird headers (CPU) and, on the MI355X, returns the model's clusters -- the capacity round
trip of cbh_idx64_clusters included, which the adapter starts with no room at all."""
import os
import subprocess

import numpy as np
import pytest

import clusters_rules as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_clusters")


def _build_cpp():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_clusters.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"),
                           "-lcbird_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_dropin_compiles():
    _build_cpp()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_dcthashindex.h")).read()
    assert "QVector<QVector<Index::Match>> gpuClusters(const SearchParams& p) const {" in src


@pytest.mark.gpu
def test_dropin_runs_on_gpu(gpu, tmp_path):
    a = 0x0123456789ABCDEF
    c = CR.flip(a, [0, 1, 2])
    b = CR.flip(c, [10, 11, 12])
    walk = CR.random_walks(257, 1)
    cases = [((np.array([a, b, c], np.uint64), np.array([1, 2, 3], np.uint32)), 5, 1),  # the issue's chain
             (walk, 5, 1), (walk, 5, 2), (walk, 3, 0), ((walk[0][:1], walk[1][:1]), 5, 1)]
    path = tmp_path / "sets.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for (h, ids), thresh, min_matches in cases:
            f.write(np.array([len(ids), thresh, min_matches], np.int32).tobytes())
            for x, i in zip(h, ids):
                f.write(np.uint32(i).tobytes() + np.uint64(x).tobytes())
    _build_cpp()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    at = 0
    for k, ((h, ids), thresh, min_matches) in enumerate(cases):
        want = CR.clusters(h, ids, thresh, max(2, min_matches + 1))
        assert lines[at] == f"case {k} {len(want)}"
        for g, line in zip(want, lines[at + 1: at + 1 + len(want)]):
            assert line.split() == [f"{i}:{s}" for i, s in g]
        at += 1 + len(want)
    assert at == len(lines) and lines[1].split() == ["1:3", "2:3", "3:3"]
