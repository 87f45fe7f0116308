"""CPU: the kernels of the -sort-similar chain over a table (cbird_amd/csrc/sortsimilar_table.hip) and the two kernels
cbh_color_sort_similar adds to color.hip compile for gfx950 without scratch memory and without spills -- the compiler's
own resource remarks through tools/kernel_resources.py (cross-compiles, no GPU), as tests/test_turn_kernels_build.py does.
k_sort_similar_table keeps its loop's uniform state in scalar registers, which is where it ran out first."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KERNELS = {"sortsimilar_table.hip": ["k_ss_keys", "k_st_gather", "k_st_permute", "k_sort_similar_table"],
           "color.hip": ["k_color_table", "k_color_absent"]}


@pytest.mark.parametrize("source", list(KERNELS))
def test_table_kernels_neither_spill_nor_use_scratch(source):
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), source],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]  # (non-zero: a kernel spills or uses scratch)
    lines = [l for l in r.stdout.splitlines() if l.startswith(source)]
    if source == "sortsimilar_table.hip":
        assert len(lines) == len(KERNELS[source]), r.stdout
    for k in KERNELS[source]:
        mine = [l for l in lines if f" {k} " in l]
        assert len(mine) == 1 and " scratch   0 " in mine[0], r.stdout
