"""CPU: every instantiation of k_turn_views (cbird_amd/csrc/turns.hip) compiles for gfx950 without scratch memory and
without spills -- the compiler's own resource remarks through tools/kernel_resources.py (cross-compiles, no GPU), as
tests/test_demosaic_kernels_build.py does for the contact-sheet kernels.  The kernel keeps a chunk's 16 * CH source
bytes and its assembled stores in registers that only fully unrolled loops index."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNELS = ["k_turn_views<%d, %s>" % (c, b) for c in (1, 3, 4) for b in ("false", "true")]


def test_turn_kernels_neither_spill_nor_use_scratch():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "turns.hip"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]  # (non-zero: a kernel spills or uses scratch)
    lines = [l for l in r.stdout.splitlines() if l.startswith("turns.hip")]
    assert len(lines) == len(KERNELS), r.stdout
    for k in KERNELS:
        mine = [l for l in lines if f" {k} " in l]
        assert len(mine) == 1 and " scratch   0 " in mine[0], r.stdout
