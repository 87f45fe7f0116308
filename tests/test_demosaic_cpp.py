"""The demosaicHough drop-ins of cbird_amd/cpp/gpu_cvutil.h (gpuDemosaicHough for a batch and for one sheet) compiled
against the mock cv::Mat: on the CPU they must compile; on the GPU box tests/cpp/test_demosaic.cpp runs them on sheets this
test writes and must print the rectangles of the numpy model (tests/demosaic_rules.py)."""
import os
import subprocess

import numpy as np
import pytest

import demosaic_rules as M
import difference_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_demosaic")


def _build():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_demosaic.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"), "-lcbird_hip",
                           "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"), "-Wl,-rpath,/opt/rocm/lib"])


def test_demosaic_dropins_compile():
    _build()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_cvutil.h")).read()
    assert "void gpuDemosaicHough(const cv::Mat& cvImg, Rects& rects, const Params& params)" in src
    assert ("void gpuDemosaicHough(const std::vector<cv::Mat>& sheets, std::vector<Rects>& rects, "
            "const Params& params)") in src


@pytest.mark.gpu
def test_demosaic_dropins_run_on_gpu(gpu, tmp_path):
    """a staggered sheet (subdivided), a plain grid in four channels, a strip in one channel and a texture that is no
    sheet: one library call per channel count in the batch form, then each as a view through the one-sheet form"""
    sheets = [M.sheet(*M.LAYOUTS[0], seed=1)[0], R.as_channels(M.sheet(*M.LAYOUTS[1], seed=1)[0], 4, 1),
              R.as_channels(M.sheet(*M.LAYOUTS[3], seed=1)[0], 1, 2), R.textured(60, 45, 9)]
    path = tmp_path / "sheets.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(sheets)).tobytes())
        for im in sheets:
            ch = 1 if im.ndim == 2 else im.shape[2]
            f.write(np.array([im.shape[1], im.shape[0], ch], np.int32).tobytes())
            f.write(np.ascontiguousarray(im).tobytes())
    _build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    want = [M.demosaic(im) for im in sheets]
    assert [len(w) for w in want] == [7, 6, 4, 1]
    for what in ("batch", "single"):
        for i, w in enumerate(want):
            got = [tuple(int(v) for v in ln[2:]) for ln in lines if ln[0] == what and int(ln[1]) == i]
            assert got == [tuple(r) for r in w], (what, i)
    tight = [tuple(int(v) for v in ln[2:]) for ln in lines if ln[0] == "tight"]
    assert tight == [tuple(r) for r in M.demosaic(sheets[0], M.params(hough_thresh_factor=0.99))]
