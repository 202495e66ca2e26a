"""filmac_cli, the tool's command line on raw BGRA files: a small clip in, the stretched clip out -- the output byte
stream is the checker's, with and without -gamma."""
import os
import subprocess

import numpy as np
import pytest

import _filmac_ref as R
import _libs as L

CLI = os.path.join(L.PKG, "filmac_cli")


def test_cli_refuses_like_the_tool(tmp_path):
    """Switch errors end the program with 1 before any device is touched; so does a missing size, which the tool would
    take from its input."""
    io = ["-i", "a", "-o", str(tmp_path / "o")]
    for args in (["-width", "31"] + io, ["-height", "31", "-width", "64"] + io, ["-o", str(tmp_path / "o")], ["-i", "a"], ["-gamma"],
                 ["-bogus"] + io, ["-fa", "2"] + io, ["stray"] + io, ["-h"], io, ["-width", "64"] + io):
        r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1, args
    assert not os.path.exists(str(tmp_path / "o"))


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [None, "ntsc"])
def test_cli_equals_checker(tmp_path, gamma):
    w, h = 96, 32
    clip = np.stack(R.branch_clip(w, h, 96)[:5])
    fin, fout = str(tmp_path / "in.bgra"), str(tmp_path / "out.bgra")
    with open(fin, "wb") as f:
        f.write(clip.tobytes() + b"tail")                                          # a partial frame at the end is dropped
    args = [CLI, "-width", str(w), "--height", "0x20", "-underscan", "5", "-422", "-i", fin, "-o", fout]
    if gamma:
        args += ["-gamma", gamma]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    want = np.stack(R.run(clip, 2.2 if gamma else -1.0)[0])
    got = np.fromfile(fout, dtype=np.uint8)
    assert got.size == want.size, "frames written: %r" % (got.size / (w * h * 4),)
    assert int((got.reshape(want.shape) != want).sum()) == 0
    assert int((want != clip).sum()) > 0                                           # the compare means something
    if gamma:
        assert int((want != np.stack(R.run(clip)[0])).sum()) > 0                   # and -gamma changes bytes
