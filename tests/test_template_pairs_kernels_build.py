"""CPU: every kernel of cbird_amd/csrc/tmpairs.hip compiles for gfx950 without scratch memory and without spills -- the
compiler's own resource remarks through tools/kernel_resources.py (cross-compiles, no GPU), as
tests/test_template_images_kernels_build.py does for tmimages.hip.  k_warp_ragged packs four pixels into CH dwords as k_warp
does: an index the compiler cannot resolve would move them to scratch memory, pass every result check and only run slower."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNELS = ["k_tm_match_pairs<false>", "k_tm_match_pairs<true>", "k_warp_ragged<1>", "k_warp_ragged<3>", "k_warp_ragged<4>",
           "k_tm_mask_ragged"]


def test_template_pairs_kernels_neither_spill_nor_use_scratch():
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "tmpairs.hip"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]  # (non-zero: a kernel spills or uses scratch)
    lines = [l for l in r.stdout.splitlines() if l.startswith("tmpairs.hip")]
    assert len(lines) == len(KERNELS), r.stdout
    for k in KERNELS:
        mine = [l for l in lines if f" {k} " in l]
        assert len(mine) == 1 and " scratch   0 " in mine[0], r.stdout
