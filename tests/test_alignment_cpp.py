"""The alignment drop-ins of cbird_amd/cpp/gpu_cvutil.h (gpuAlignSpatial, its one-pair overload, gpuAlignTemporal)
compiled against the mock cv::Mat: on the CPU they must compile; on the GPU box tests/cpp/test_alignment.cpp runs them on
three pairs and one clip this test writes and must print the records of the numpy model (tests/alignment_rules.py)."""
import os
import subprocess

import numpy as np
import pytest

import alignment_rules as A
import difference_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_alignment")
SFIELDS = ["min_x", "min_y", "min_sad", "sad_at_zero"]
TFIELDS = ["placement", "offset", "min_mean", "start_mean"]


def _build():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_alignment.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"), "-lcbird_hip",
                           "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"), "-Wl,-rpath,/opt/rocm/lib"])


def test_alignment_dropins_compile():
    _build()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_cvutil.h")).read()
    assert ("void gpuAlignSpatial(const cv::Mat& left, const std::vector<cv::Mat>& rights, "
            "std::vector<cbh_align_spatial_result>& out)") in src
    assert "gpuAlignSpatial(const cv::Mat& left, const cv::Mat& right, float* alignX, float* alignY)" in src
    assert "gpuAlignTemporal(const std::vector<cv::Mat>& left, const std::vector<cv::Mat>& right" in src
    assert "int start = -1)" in src


def _write(f, im):
    ch = 1 if im.ndim == 2 else im.shape[2]
    f.write(np.array([im.shape[1], im.shape[0], ch], np.int32).tobytes())
    f.write(np.ascontiguousarray(im).tobytes())


@pytest.mark.gpu
def test_alignment_dropins_run_on_gpu(gpu, tmp_path):
    """a planted shift, and two textures of other sizes in the other channel counts (one library call per count); a clip
    of 12 frames whose window of 3 is cut at placement 7, searched from 2 and from the default start"""
    left, planted = A.planted(3, -5, seed=21)
    rights = [planted, R.textured(41, 30, 22, 1), R.textured(19, 57, 23, 4)]
    lf = [R.textured(9, 7, 30 + k) for k in range(12)]
    rf = lf[7:10]
    path = tmp_path / "align.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(rights)).tobytes())
        for im in [left] + rights:
            _write(f, im)
        f.write(np.array([len(lf), len(rf), 2], np.int32).tobytes())
        for im in lf + rf:
            _write(f, im)
    _build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    want = [A.align_spatial(left, r)[1] for r in rights]
    assert (want[0]["min_x"], want[0]["min_y"], want[0]["min_sad"]) == (3, -5, 0)
    for what in ("group", "single"):
        got = [ln for ln in lines if ln[0] == what]
        assert len(got) == len(want)
        for i, rec in enumerate(want):
            assert [int(v) for v in got[i][1:6]] == [i] + [rec[k] for k in SFIELDS], (what, i)
            if what == "single":
                assert [float(v) for v in got[i][6:]] == [float(rec["min_x"]), float(rec["min_y"])]
    for what, start in (("clip", 2), ("clip_default", A.default_start(10))):
        rec = A.align_temporal(lf, rf, start)[2]
        assert rec["placement"] == 7 and rec["min_mean"] == 0
        got = next(ln for ln in lines if ln[0] == what)
        assert [int(v) for v in got[1:]] == [rec[k] for k in TFIELDS], what
