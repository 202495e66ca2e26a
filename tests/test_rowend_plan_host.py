"""The decoder's row schedule (csrc/ntsc_rowend_plan.hpp: fill groups, steady loop, drain groups, the stages and loads
live at each stream position, where bursts complete) is plain integer code, so it is swept on the host:
tests/rowend_plan_check.cpp is compiled with plain g++, and again with the address and undefined-behaviour sanitizers as
the stand-alone program it is, and both are run."""
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
def test_row_schedule_equals_the_one_position_predicates(tmp_path, build):
    """Every W in 1 ... 800, 1920 and 3840; chroma delay 9, 12, 14; the non-VHS, S-Video and full-output-filter forms:
    every position covered exactly once, the steady range today's, every output pixel stored exactly once."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/rowend_plan_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / ("rowend_plan_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "rowend_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 bad" in r.stdout, r.stdout
