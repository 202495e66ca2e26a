"""The vhsled run detector and smoothing step (csrc/led_run.hpp) are plain integer code, so they are swept on the host:
tests/led_run_check.cpp is compiled with plain g++, and again with the address and undefined-behaviour sanitizers as
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
def test_run_detector_equals_the_bit_by_bit_loop(tmp_path, build):
    """Every 16-bit pattern at bit offsets 0, 47 and 48 with every carry, 10^5 random masks, runs that start at bits
    55 .. 63 of the first of two chunks, and the smoothing step at every residue modulo 9 up to the widest frame."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/led_run_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / ("led_run_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "led_run_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 bad" in r.stdout, r.stdout
