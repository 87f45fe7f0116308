"""tests/test_slice_device.py again, in a child process under the virtual-device shim (tests/shim/vdev.c, see
tests/test_virtual_devices.py): with CBH_VDEV set that file takes the shapes mask 0b1101 x 1 shard and 2 ordinals x 2
shards, so the copies between ordinals of the 256-bit slice (rows that change ordinal travel as a staged block) execute,
and the shim's device discipline checks see every launch and event of them."""
import os
import re
import subprocess
import sys

import pytest

from test_virtual_devices import HERE, ROOT, build_shim, shim_env


@pytest.mark.gpu
def test_slices_over_virtual_ordinals(gpu):
    build_shim()
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(HERE, "test_slice_device.py"), "-x", "-q", "-m", "gpu",
                          "-p", "no:cacheprovider"], env=shim_env(4), capture_output=True, text=True, timeout=900, cwd=ROOT)
    tail = (out.stdout + out.stderr)[-3000:]
    assert out.returncode == 0, tail
    # with two shapes: 12 sizes x 2 of the 64-bit index, 2 of the 256-bit one, 4 + 2 of colour, 2 x 2 radixes of video,
    # 3 walks over refused allocations, 1 video slice that allocates nothing -- all of them run, none left out
    expected = 12 * 2 + 2 + (4 + 2) + 2 * 2 + 3 + 1
    summary = out.stdout.strip().splitlines()[-1]
    m = re.fullmatch(r"=* ?(\d+) passed(, \d+ warnings?)? in [\d.]+s( \([\d:]+\))? ?=*", summary)
    assert m and int(m.group(1)) == expected, (summary, tail)
