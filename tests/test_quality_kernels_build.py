"""CPU: every kernel of cbird_amd/csrc/quality.hip compiles for gfx950 without scratch memory and without spills -- the
compiler's own resource remarks through tools/kernel_resources.py (cross-compiles, no GPU), as
tests/test_slice_kernels_build.py does for the slice kernels.  The walkers keep five rows of a strip in registers; an
array of theirs that lands in scratch memory, or lane masks that no longer fit the scalar registers, would pass every
result check and only run slower."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNELS = ["k_quality_pack<1>", "k_quality_pack<3>", "k_quality_pack<4>", "k_quality_edges<true>", "k_quality_edges<false>",
           "k_quality_score"]


def test_quality_kernels_neither_spill_nor_use_scratch():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "quality.hip"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]  # (non-zero: a kernel spills or uses scratch)
    lines = [l for l in r.stdout.splitlines() if l.startswith("quality.hip")]
    assert len(lines) == len(KERNELS), r.stdout
    for k in KERNELS:
        mine = [l for l in lines if f" {k} " in l]
        assert len(mine) == 1 and " scratch   0 " in mine[0], r.stdout
