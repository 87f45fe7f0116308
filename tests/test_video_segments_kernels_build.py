"""CPU: every kernel of cbird_amd/csrc/vsegments.hip compiles for gfx950 without scratch memory and without spills -- the
compiler's own resource remarks through tools/kernel_resources.py (cross-compiles, no GPU), as
tests/test_video_coverage_kernels_build.py does."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SOURCE = "vsegments.hip"
KERNELS = ["k_vs_init", "k_vs_support", "k_vs_pick", "k_vs_members", "k_vs_finish"]


def test_segments_kernels_neither_spill_nor_use_scratch():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SOURCE],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]  # (non-zero: a kernel spills or uses scratch)
    lines = [l for l in r.stdout.splitlines() if l.startswith(SOURCE)]
    assert len(lines) == len(KERNELS), r.stdout
    for k in KERNELS:
        mine = [l for l in lines if f" {k} " in l]
        assert len(mine) == 1 and " scratch   0 " in mine[0], r.stdout
