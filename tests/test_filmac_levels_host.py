"""The arithmetic of the filmac stage (csrc/filmac_levels.hpp: block grid, block mean, frame levels, recurrence, byte
table) is plain integer code that the kernels and the host share, so it is swept on the host: tests/filmac_levels_check.cpp
is compiled with plain g++, and again with the address and undefined-behaviour sanitizers as the stand-alone program it
is, and both are run."""
import os
import shutil
import subprocess

import pytest

import _libs as L

_FLAGS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}


@pytest.mark.parametrize("build", sorted(_FLAGS))
def test_levels_header_equals_the_tools_loops(tmp_path, build):
    """The block grid of every width 16 .. 1100, frame levels of random frames through block records, 2000 runs of the
    recurrence, and the table of 10^4 random (final_minv, final_maxv) pairs -- a denominator of 1 and minima above every
    pixel among them -- plus the denominators only ntscsim_filmac_set_state() can produce."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/filmac_levels_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / ("filmac_levels_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "filmac_levels_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 bad" in r.stdout, r.stdout
