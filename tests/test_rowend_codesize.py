"""A guard against the grouped row ends (csrc/ntsc_decode_fast.hip: grouped_row) quietly falling out of the build.

The kernel names are the same with and without them, and a row that does not take them still decodes correctly through
the one-position path in the same kernel, so no parity test can tell whether they are there.  What can: the code object.
A decoder that takes the groups holds, beside the one-position path, the fill + steady loop + drain once per chroma
delay class (d mod 4 = 0, 1, 2), i.e. three more copies of the steady loop alone; if decode_fast_body's GROUPS, or
rowend::grouped(), ever became constant false the compiler would drop all of it and the kernel would be back at the
size of its one-position sibling.  So: each grouped kernel must be larger than the largest -vhs decoder of the same
precision that keeps the one-position row ends (S-Video, any-phase, full-output-filter forms) by at least twice that
sibling's own steady loop -- taken, conservatively, as one eighth of the sibling (the loop is 5.5 KB of the 31 KB
one-position k_decode_fast<true,double>: profiles/r08_rowends_census.txt section 3).  Needs no GPU."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = "/opt/rocm/lib/llvm/bin"

GROUPED = ["k_decode_fast<true, double, false>", "k_decode_fast<true, double, true>", "k_decode_fast_bk<true, double>"]
ONE_POSITION = ["k_decode_fast_sv<double>", "k_decode_fast_xi<double>", "k_decode_fast_fo<double>"]


def _kernel_sizes(obj):
    """{demangled kernel name: bytes of code} of the gfx950 code object in a host object."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat"), os.path.join(d, "co")
        subprocess.run([BIN + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([BIN + "/clang-offload-bundler", "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co], check=True)
        syms = subprocess.run([BIN + "/llvm-readelf", "-s", "--demangle", "-W", co], check=True,
                              stdout=subprocess.PIPE, text=True).stdout
    sizes = {}
    for line in syms.splitlines():
        m = re.match(r"\s*\d+:\s+[0-9a-f]+\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+void ntscsim::(k_\w+<[^(]*>)\(", line)
        if m:
            sizes[m.group(2)] = int(m.group(1))
    return sizes


def test_grouped_decoders_hold_the_grouped_code():
    obj = os.path.join(ROOT, "composite-video-simulator_amd", "csrc", "ntscsim_hip.o")
    if not os.path.exists(obj) or not os.path.exists(BIN + "/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("device objects or llvm tools not present")
    sizes = _kernel_sizes(obj)
    missing = [k for k in GROUPED + ONE_POSITION if k not in sizes]
    assert not missing, (missing, sorted(sizes)[:60])
    sibling = max(sizes[k] for k in ONE_POSITION)
    need = sibling + 2 * (sibling // 8)
    small = {k: sizes[k] for k in GROUPED if sizes[k] <= need}
    assert not small, "no grouped row ends in %s (a one-position sibling is %d bytes, a grouped kernel needs more than %d)" % (
        small, sibling, need)
