"""The qualityScore drop-ins of cbird_amd/cpp/gpu_cvutil.h (gpuQualityScore, gpuQualityScores) compiled against the mock
cv::Mat: on the CPU they must compile; on the GPU box tests/cpp/test_quality.cpp runs them on images this test writes
and must print the scores of the numpy restatement (tests/test_quality_rules.py)."""
import os
import subprocess

import numpy as np
import pytest

import test_quality_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_quality")


def _build():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_quality.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"), "-lcbird_hip",
                           "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"), "-Wl,-rpath,/opt/rocm/lib"])


def test_quality_dropins_compile():
    _build()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_cvutil.h")).read()
    assert "int gpuQualityScore(const cv::Mat& img)" in src
    assert "void gpuQualityScores(const std::vector<cv::Mat>& images, std::vector<int>& scores)" in src


@pytest.mark.gpu
def test_quality_dropins_run_on_gpu(gpu, tmp_path):
    """one image at a time, views into larger images (rows read where they lie), and a mixed-size, mixed-channel group
    in one call"""
    cases = R.cases()
    prefixes = ["side_2x2_", "side_9x19_", "qw_64_", "blocky3_c1", "blocky4_c3", "blocky3_c4", "constant_c3",
                "red_constant_c4", "side1_1x40_c3", "run_of_2_ends_at_3_y_c3", "tall_7x300_c1", "strips_c1"]
    names = [next(n for n in cases if n.startswith(p)) for p in prefixes]
    imgs = [cases[n] for n in names]
    views = []
    for im in imgs:
        h, w = im.shape[:2]
        vx, vy = w // 5, h // 4
        views.append((vx, vy, max(w // 2, 1), max(h // 2, 1)))
    path = tmp_path / "images.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(imgs)).tobytes())
        for im, v in zip(imgs, views):
            ch = 1 if im.ndim == 2 else im.shape[2]
            f.write(np.array([im.shape[1], im.shape[0], ch, *v], np.int32).tobytes())
            f.write(np.ascontiguousarray(im).tobytes())
    _build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.stdout.strip().splitlines()}
    want = [int(R.yardstick()[n]["score"]) for n in names]
    want_views = [int(R.quality_stencil(im[vy: vy + vh, vx: vx + vw])["score"])
                  for im, (vx, vy, vw, vh) in zip(imgs, views)]
    assert got["one"] == want and got["group"] == want
    assert got["view"] == want_views and got["views"] == want_views
    assert sum(s != R.NO_SCORE for s in want) >= 8 and sum(s != R.NO_SCORE for s in want_views) >= 6
