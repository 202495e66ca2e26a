"""The parser of the posterize and colormap stages (csrc/pixmap_params.cpp) owns a heap block per parameter struct and
walks an argv that ends in a NULL, so it is driven on the host as the stand-alone program tests/pixmap_params_check.cpp:
compiled with plain g++, and again with the address and undefined-behaviour sanitizers, and both are run."""
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
def test_parser_and_free_over_the_argument_vectors(tmp_path, build):
    assert shutil.which("g++") is not None, "g++ is needed to build tests/pixmap_params_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / ("pixmap_params_check_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + _FLAGS[build] +
                          ["-I", os.path.join(L.ROOT, "include"), os.path.join(here, "pixmap_params_check.cpp"),
                           os.path.join(L.PKG, "csrc", "pixmap_params.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert " 0 bad" in r.stdout, r.stdout
