"""CPU: the host-only part of cbh_video_segments -- the views and the range, budget and grouping arithmetic of
cbird_amd/csrc/cbh_vviews.h -- in a stand-alone program (tests/cpp/vviews_host_check.cpp) built with the address and
undefined-behaviour sanitizers and run: hand-made videos, the edges of the budget and of 32-bit frame numbers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_views_ranges_and_groups_under_host_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if not shutil.which(cxx):
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "vviews_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "cbird_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "vviews_host_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]
