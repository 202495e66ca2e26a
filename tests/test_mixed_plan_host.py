"""The host plan of ntscsim_mixed_fields_device (csrc/mixed_plan.hpp: groups per set in order of first use, a piece of one
common scanline space per group at a multiple of 64 rows, the block -> (group, block in group) tables of the encoder and
of the three decoder classes, every descriptor's rand() start position) has no HIP in it, so it is swept on the host:
tests/mixed_plan_check.cpp, a stand-alone program with its own main, is compiled with plain g++, and again with the address
and undefined-behaviour sanitizers, and both are run as the programs they are."""
import os
import re
import shutil
import subprocess

import pytest

import _libs as L

_FLAGS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(_FLAGS))
def test_plan_groups_rows_blocks_and_positions(tmp_path, build):
    """Hand-made calls and 160 pseudo-random ones (up to 5,000 descriptors, 1..64 sets, Lslot in 1, 8, 62, 63, 64, 65, 243):
    first-use order and stability, bases, no overlap, every row of every group in exactly one encoder and one decoder
    block, rand() positions against a serial walk, and the size limits for the padded space."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/mixed_plan_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / ("mixed_plan_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "mixed_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"mixed_plan: (\d+) checks, (\d+) bad", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) > 100000 and int(m.group(2)) == 0, r.stdout[-4000:]
