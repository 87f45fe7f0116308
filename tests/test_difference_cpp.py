"""The difference-image drop-ins of cbird_amd/cpp/gpu_cvutil.h (gpuBrightnessAndContrastAuto, gpuDifferenceImage,
gpuDifferenceImages) compiled against the mock cv::Mat: on the CPU they must compile; on the GPU box
tests/cpp/test_difference.cpp runs them on three pairs this test writes and must print the records and picture hashes of
the numpy model (tests/difference_rules.py)."""
import os
import subprocess

import numpy as np
import pytest

import difference_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_difference")
FIELDS = ["w", "h", "warped", "sum_total", "sum_max", "n_ge32", "n_ge1024", "left_min", "left_max", "right_min", "right_max"]


def _build():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_difference.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"), "-lcbird_hip",
                           "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"), "-Wl,-rpath,/opt/rocm/lib"])


def fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_difference_dropins_compile():
    _build()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_cvutil.h")).read()
    assert "void gpuBrightnessAndContrastAuto(const cv::Mat& src, cv::Mat& dst, float clipHistPercent = 0" in src
    assert "cv::Mat gpuDifferenceImage(const cv::Mat& left, const cv::Mat& right, const double* tx = nullptr" in src
    assert "void gpuDifferenceImages(const cv::Mat& left, const std::vector<cv::Mat>& rights" in src


@pytest.mark.gpu
def test_difference_dropins_run_on_gpu(gpu, tmp_path):
    """of the dyadic group: the identity with its flag set (no warp: the left side is scaled), an integer translation and
    a quarter turn, the right images in three channel counts (one library call per count)"""
    grp = next(g for g in R.pair_groups() if g["name"] == "dyadic")
    pick = [0, 1, 3]
    left = R.as_channels(grp["left"], 4, 1)
    rights = [R.as_channels(grp["rights"][i], ch, i) for i, ch in zip(pick, (3, 1, 4))]
    txs = [grp["tx"][i] for i in pick]
    path = tmp_path / "pairs.bin"
    with open(path, "wb") as f:
        f.write(np.int32(len(rights)).tobytes())
        for im, tx in [(left, np.zeros(6))] + list(zip(rights, txs)):
            ch = 1 if im.ndim == 2 else im.shape[2]
            f.write(np.array([im.shape[1], im.shape[0], ch, 1], np.int32).tobytes())
            f.write(np.asarray(tx, np.float64).tobytes())
            f.write(np.ascontiguousarray(im).tobytes())
    _build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    want = [R.difference_image(left, r, tx, True, 5) for r, tx in zip(rights, txs)]
    assert [w[1]["warped"] for w in want] == [0, 1, 1]
    for what in ("group", "single"):
        got = [ln for ln in lines if ln[0] == what]
        assert len(got) == len(want)
        for i, (pic, rec) in enumerate(want):
            assert [int(v) for v in got[i][1:]] == [i] + [rec[k] for k in FIELDS] + [fnv(pic)], (what, i)
    stretched, (lo, hi), _ = R.auto_contrast(left, 5)
    assert [int(v) for v in lines[-1][1:]] == [lo, hi, fnv(stretched)] and lines[-1][0] == "contrast"
