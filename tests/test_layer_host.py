"""The host logic the colorkey and average_delay stages share (csrc/ntsc_layer.hpp: spans, the launch-cut planner, the clip
disjointness validation, the host-frame dedupe and aliasing rule) has no HIP in it, so it is driven here without a GPU:
tests/layer_host_check.cpp is compiled with plain g++ and run."""
import os
import shutil
import subprocess

import _libs as L


def test_layer_host_logic(tmp_path):
    """In-order descriptors (a destination a later descriptor reads, a destination written twice, the per-launch cap of 1,
    n = 0), clip calls (ring / outputs / sources overlapping by their last dword or only touching, every error code, a
    linesize of a layer that is never present) and host frames (one frame under two roles, two frames sharing one byte
    without being the same (pointer, linesize)), for ntscsim_key_desc and ntscsim_avg_desc alike."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/layer_host_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "layer_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(L.ROOT, "include"),
                           "-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "layer_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
