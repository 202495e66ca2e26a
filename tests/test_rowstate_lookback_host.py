"""The noise accumulators at a row's first draw (csrc/ntsc_rowstate_lookback.hpp: the look-back over the row's rand()
window and its backward extension) are plain integer code, so they are swept on the host:
tests/rowstate_lookback_check.cpp is compiled with plain g++, and again with the address and undefined-behaviour
sanitizers as the stand-alone program it is, together with csrc/glibc_rand.cpp, and both are run."""
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
def test_lookback_equals_the_serial_replay(tmp_path, build):
    """K in {1, 4, 16, 100}, row strides 8 ... 720, rows 0 ... 3 of the stream, luma and chroma, the window path and the
    ring path at three look-back lengths: every result equals the serial replay from the stream's first draw, and the
    test hook's lengths drive most rows through the extension."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/rowstate_lookback_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(L.PKG, "csrc")
    exe = tmp_path / ("rowstate_lookback_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", csrc, "-I", os.path.join(L.ROOT, "include"), os.path.join(here, "rowstate_lookback_check.cpp"),
                           os.path.join(csrc, "glibc_rand.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 bad" in r.stdout, r.stdout
