"""The decoder's pixel pack (csrc/ntsc_pack.hpp) is plain integer code, so its identity -- clamp to 0xFFFF and pick byte 1
== shift by 8 and clamp to 255 -- is swept on the host: tests/pack_check.cpp is compiled with plain g++ and run."""
import os
import shutil
import subprocess

import _libs as L


def test_pixel_pack_equals_the_per_channel_clamp(tmp_path):
    """Every channel value 0 ... 0x1FFFF plus 2^31 and 2^32 - 1, in each of the three channel positions, against
    clamp(x >> 8, 0, 255) of the value the reference's own conversion yields."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/pack_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "pack_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(L.PKG, "csrc"),
                           os.path.join(here, "pack_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
