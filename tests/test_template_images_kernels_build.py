"""CPU: every kernel of cbird_amd/csrc/tmimages.hip compiles for gfx950 without scratch memory and without spills -- the
compiler's own resource remarks through tools/kernel_resources.py (cross-compiles, no GPU), as
tests/test_template_match_kernels_build.py does for tmatch.hip.  k_resize_ragged keeps eight weights, eight offsets and
CH accumulators per pixel and packs four pixels into CH dwords: an index the compiler cannot resolve would move them to
scratch memory, pass every result check and only run slower."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNELS = ["k_resize_ragged<1>", "k_resize_ragged<3>", "k_resize_ragged<4>", "k_gray_ragged<3>", "k_gray_ragged<4>",
           "k_tm_match<false>", "k_tm_match<true>", "k_tm_scan_queries", "k_tm_scan_first", "k_tm_gather"]


def test_template_images_kernels_neither_spill_nor_use_scratch():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "tmimages.hip"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]  # (non-zero: a kernel spills or uses scratch)
    lines = [l for l in r.stdout.splitlines() if l.startswith("tmimages.hip")]
    assert len(lines) == len(KERNELS), r.stdout
    for k in KERNELS:
        mine = [l for l in lines if f" {k} " in l]
        assert len(mine) == 1 and " scratch   0 " in mine[0], r.stdout
