"""The host logic every device stage shares (csrc/ntsc_frames.hpp: spans, the plane check, the in-order launch planner,
the writes of a call, the copy between row pitches) has no HIP in it, so it is driven here without a GPU:
tests/frames_host_check.cpp is compiled with plain g++, and again with the address and undefined-behaviour sanitizers
as the stand-alone program it is, and both are run."""
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
def test_frames_host_logic(tmp_path, build):
    """The planner beside the quadratic restatement of its rule on 4000 random calls (6 frame slots, spans of two
    heights, 0 to 3 read spans, n in 0 .. 40, caps 1, 2, 12 and 65535), its edge cases (touching, the last 4 bytes, a
    failing launch), the writes of a call (overlap by the last dword, touching, a source over the first, last and a
    middle output, the empty set), the plane check with alignment on and off, and copy_rows between pitches 40 and 48."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/frames_host_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / ("frames_host_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", os.path.join(L.ROOT, "include"), "-I", os.path.join(L.PKG, "csrc"),
                           os.path.join(here, "frames_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "frames_host_check: 0 failed" in r.stdout, r.stdout
