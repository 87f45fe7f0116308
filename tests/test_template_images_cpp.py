"""The drop-in gpuTemplateMatchImages of cbird_amd/cpp/gpu_cvutil.h compiled against the mock cv::Mat: on the CPU it must
compile; on the GPU box tests/cpp/test_template_images.cpp runs it on the chain's group of tests/template_images_rules.py
and must print the results of the model."""
import os
import subprocess

import numpy as np
import pytest

import template_images_rules as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_template_images")


def _build():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_template_images.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"),
                           "-lcbird_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_template_images_dropin_compiles():
    _build()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_cvutil.h")).read()
    assert "inline void gpuTemplateMatchImages(const cv::Mat& tmplImg, const std::vector<cv::Mat>& candImgs," in src


@pytest.mark.gpu
def test_template_images_dropin_runs_on_gpu(gpu, tmp_path):
    from cbird_amd.orb import synthetic_pattern

    tmpl, cands, model = M.chain_fixture(3)
    assert M.chain_conditions(model) == []
    path = tmp_path / "group.bin"
    with open(path, "wb") as f:
        f.write(synthetic_pattern().astype(np.int8).tobytes())
        f.write(np.array([tmpl.shape[1], tmpl.shape[0], tmpl.shape[2]], np.int32).tobytes())
        f.write(tmpl.tobytes())
        f.write(np.int32(len(cands)).tobytes())
        for c in cands:
            f.write(np.array([c.shape[1], c.shape[0]], np.int32).tobytes() + np.ascontiguousarray(c).tobytes())
    _build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [[int(x) for x in ln.split()] for ln in out.stdout.strip().splitlines()]
    want = [[m["status"], m["w"], m["h"], m["n_keypoints"], m["n_matches"], int(m["r"]["found"]), m["r"]["score"],
             m["r"]["cand_hash"], m["r"]["tmpl_hash"], *[int(v) for v in m["r"]["roi"]]] for m in model]
    assert got == want
