"""The drop-in gpuTemplateMatchPairs of cbird_amd/cpp/gpu_cvutil.h compiled against the mock cv::Mat: on the CPU it must
compile; on the GPU box tests/cpp/test_template_pairs.cpp runs it on the 3-channel fixture of
tests/template_pairs_rules.py and must print the rows of the model."""
import os
import subprocess

import numpy as np
import pytest

import template_pairs_rules as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_template_pairs")
INT_MAX = (1 << 31) - 1


def _build():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_template_pairs.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"),
                           "-lcbird_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_template_pairs_dropin_compiles():
    _build()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_cvutil.h")).read()
    assert ("inline void gpuTemplateMatchPairs(const std::vector<cv::Mat>& images, "
            "const std::vector<std::pair<int, int>>& pairs,") in src


@pytest.mark.gpu
def test_template_pairs_dropin_runs_on_gpu(gpu, tmp_path):
    from cbird_amd.orb import synthetic_pattern

    images, pt, pc, model = P.pairs_fixture(3)
    assert P.pairs_conditions(images, pt, pc, model) == []
    path = tmp_path / "pairs.bin"
    with open(path, "wb") as f:
        f.write(synthetic_pattern().astype(np.int8).tobytes())
        f.write(np.array([3, len(images)], np.int32).tobytes())
        for im in images:
            f.write(np.array([im.shape[1], im.shape[0]], np.int32).tobytes() + np.ascontiguousarray(im).tobytes())
        f.write(np.int32(len(pt)).tobytes())
        f.write(np.stack([pt, pc], 1).astype(np.int32).tobytes())
    _build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [[int(x) for x in ln.split()] for ln in out.stdout.strip().splitlines()]
    want = []
    for m in model:
        if m["r"] is None:  # the chain never got that far: the blank record
            want.append([m["status"], m["w"], m["h"], 0, 0, 0, INT_MAX, 0, 0] + [0] * 8)
        else:
            want.append([m["status"], m["w"], m["h"], m["n_keypoints"], m["n_matches"], int(m["r"]["found"]), m["r"]["score"],
                         m["r"]["cand_hash"], m["r"]["tmpl_hash"], *[int(v) for v in m["r"]["roi"]]])
    assert got == want
