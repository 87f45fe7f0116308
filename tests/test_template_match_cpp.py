"""The drop-in gpuTemplateMatch of cbird_amd/cpp/gpu_cvutil.h compiled against the mock cv::Mat: on the CPU it must
compile; on the GPU box tests/cpp/test_template_match.cpp runs it on the chain's group of tests/template_match_rules.py
and must print the results of the numpy model."""
import os
import subprocess

import numpy as np
import pytest

import template_match_rules as R
import test_template_match_rules as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "test_template_match")


def _build():
    """the rules of tests/cpp/Makefile for one more program"""
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cbird_amd", "cpp"), "-I" + os.path.join(CPP, "mock"), "-o", EXE,
                           os.path.join(CPP, "test_template_match.cpp"), "-L" + os.path.join(ROOT, "cbird_amd"),
                           "-lcbird_hip", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "cbird_amd"),
                           "-Wl,-rpath,/opt/rocm/lib"])


def test_template_match_dropin_compiles():
    _build()
    src = open(os.path.join(ROOT, "cbird_amd", "cpp", "gpu_cvutil.h")).read()
    assert "inline void gpuTemplateMatch(const cv::Mat& tmplImg, const std::vector<cv::Mat>& candImgs," in src


@pytest.mark.gpu
def test_template_match_dropin_runs_on_gpu(gpu, tmp_path):
    tmpl, cands, al, bl, scales = R.chain_fixture()
    yard = T.chain_yardstick()
    path = tmp_path / "group.bin"
    with open(path, "wb") as f:
        f.write(np.array([tmpl.shape[1], tmpl.shape[0], tmpl.shape[2]], np.int32).tobytes())
        f.write(tmpl.tobytes())
        f.write(np.int32(len(cands)).tobytes())
        for c, a, b, s in zip(cands, al, bl, scales):
            f.write(np.array([c.shape[1], c.shape[0], c.shape[2], len(a)], np.int32).tobytes())
            f.write(np.float32(s).tobytes() + np.ascontiguousarray(c).tobytes())
            f.write(np.ascontiguousarray(a, np.float32).tobytes() + np.ascontiguousarray(b, np.float32).tobytes())
    _build()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [[int(x) for x in ln.split()] for ln in out.stdout.strip().splitlines()]
    want = [[int(r["found"]), r["score"], int(r["tx_found"]), r["iterations"], r["good_count"], r["cand_hash"],
             r["tmpl_hash"], *[int(v) for v in r["roi"]]] for r in yard]
    assert got == want
    assert sum(r["found"] for r in yard) == 4
