"""CPU: every kernel of cbird_amd/csrc/diffimage.hip compiles for gfx950 without scratch memory and without spills -- the
compiler's own resource remarks through tools/kernel_resources.py (cross-compiles, no GPU), as
tests/test_quality_kernels_build.py does for the quality kernels.  The colour pass holds two view descriptors with a 2 x 3
f64 matrix each and the four pixels of both sides; a pixel array indexed by a loop the compiler did not unroll would land
in scratch memory, pass every result check and only run slower."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNELS = (["k_diff_hist<%d>" % c for c in (1, 3, 4)] + ["k_diff_tables", "k_diff_stretch", "k_diff_detail"] +
           ["k_diff_color<%d, %d>" % (a, b) for a in (1, 3, 4) for b in (1, 3, 4)])


def test_difference_kernels_neither_spill_nor_use_scratch():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "diffimage.hip"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]  # (non-zero: a kernel spills or uses scratch)
    lines = [l for l in r.stdout.splitlines() if l.startswith("diffimage.hip")]
    assert len(lines) == len(KERNELS), r.stdout
    for k in KERNELS:
        mine = [l for l in lines if f" {k} " in l]
        assert len(mine) == 1 and " scratch   0 " in mine[0], r.stdout
