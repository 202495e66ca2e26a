"""What the two host-frame engines decide without the GPU (csrc/engine_host.hpp: the copy threads that deliver staged
results, the row maps of a field with and without line doubling, the copy lists of both engines, the clash rule for fields
that share a frame, the ranges of pinned memory, the writer table that chains the tight rows of the 4:2:2 engine) has no HIP in
it, so it is driven here without a GPU:
tests/engine_host_check.cpp is compiled with plain g++ and run."""
import os
import shutil
import subprocess

import _libs as L


def test_engine_host_logic(tmp_path):
    """Delivery with 1, 4 and 16 copy threads (post order, a failed launch, cancel, restart, drain, the padding of every
    destination row), the BGRA engine's rows against a model of the reference's line doubling for heights 2..5, both copy
    lists' bounds and disjointness, sub_dst_conflict, find / overlaps / release / page_span of the pin ranges, and H422Writers
    on a seeded random walk (batched writes, one-at-a-time iterations, DIRTY, re-makes of the rings to more and to fewer slots
    than a live device frame's, more caller frames than the table holds) against a brute-force model of the chain rule."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/engine_host_check.cpp"
    here = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / "engine_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", os.path.join(L.ROOT, "include"),
                           "-I", os.path.join(L.PKG, "csrc"), os.path.join(here, "engine_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
