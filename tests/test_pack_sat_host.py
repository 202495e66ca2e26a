"""The saturating pixel pack (csrc/ntsc_pack.hpp: pack_bgra_sat, what pack_bgra calls) is plain integer code around a model
of v_cvt_pk_u16_u32, so its identity with the per-channel shift / clamp / or is swept on the host:
tests/pack_sat_check.cpp is compiled with plain g++ and run, as it is and as a stand-alone program under the address
and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

import _libs as L


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_saturating_pack_equals_the_shift_pack(tmp_path, sanitize):
    """Every channel value 0 ... 0x1FFFF and every power of two with its neighbours up to 2^32 - 1, in each of the three
    channel positions."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/pack_sat_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "pack_sat_check"
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra +
                          ["-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "pack_sat_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
