"""What the host plan (csrc/mixed_plan.hpp) gained for ntscsim_mixed_fields422_device: fields that draw nothing
(NTSCSIM_422_NOCOMP) and a composite-plane limit that can be switched off (the YUV422P tool has no composite plane).
tests/mixed_plan422_check.cpp, a stand-alone program with its own main, is compiled with plain g++, and again with the
address and undefined-behaviour sanitizers, and both are run as the programs they are."""
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
def test_plan_fields_that_draw_nothing_and_the_plane_limit(tmp_path, build):
    """200 pseudo-random calls (up to 3,000 descriptors, 1..40 sets, a third of the fields drawing nothing, AUTO and
    explicit positions, also backwards) against a naive restatement of the position rule; the same calls with no such
    field and the limit on against the plan as it was called before; 65535 / 65536 fields of Lslot 243 at W 720."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/mixed_plan422_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / ("mixed_plan422_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "mixed_plan422_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"mixed_plan422: (\d+) checks, (\d+) bad", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) > 100000 and int(m.group(2)) == 0, r.stdout[-4000:]
