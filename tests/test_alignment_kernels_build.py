"""CPU: every kernel of cbird_amd/csrc/align.hip compiles for gfx950 without scratch memory and without spills -- the
compiler's own resource remarks through tools/kernel_resources.py (cross-compiles, no GPU), as
tests/test_difference_kernels_build.py does for the difference image.  k_align_sad keeps 17 accumulators and 16 staged
left dwords per lane in arrays that only fully unrolled loops index; one loop left rolled would put them in scratch
memory, pass every result check and only run slower."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNELS = (["k_align_scale<%d, %d>" % (c, s) for c in (1, 3, 4) for s in (256, 128)] +
           ["k_align_sad", "k_align_pick", "k_align_cell", "k_align_means", "k_align_tpick"])


def test_alignment_kernels_neither_spill_nor_use_scratch():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "align.hip"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]  # (non-zero: a kernel spills or uses scratch)
    lines = [l for l in r.stdout.splitlines() if l.startswith("align.hip")]
    assert len(lines) == len(KERNELS), r.stdout
    for k in KERNELS:
        mine = [l for l in lines if f" {k} " in l]
        assert len(mine) == 1 and " scratch   0 " in mine[0], r.stdout
