"""vhsled_cli, the tool's command line on raw BGRA files: a small clip in, the aligned clip out -- the output byte
stream is the checker's."""
import os
import subprocess

import numpy as np
import pytest

import _led_ref as R
import _libs as L

CLI = os.path.join(L.PKG, "vhsled_cli")


def test_cli_refuses_like_the_tool(tmp_path):
    """Switch errors end the program with 1 before any device is touched; so does a missing size, which the tool would
    take from its input."""
    io = ["-i", "a", "-o", str(tmp_path / "o")]
    for args in (["-width", "31"] + io, ["-height", "31", "-width", "64"] + io, ["-o", str(tmp_path / "o")], ["-i", "a"], ["-or"],
                 ["-bogus"] + io, ["-fa", "2"] + io, ["stray"] + io, ["-h"], io, ["-width", "64"] + io):
        r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1, args
    assert not os.path.exists(str(tmp_path / "o"))


@pytest.mark.gpu
def test_cli_equals_checker(tmp_path):
    w, h, n = 72, 40, 19                                                           # more than one batch of 16 frames
    rng = np.random.RandomState(77)
    clip = np.stack([R.capture_frame(rng, w, h) for _ in range(n)])
    fin, fout = str(tmp_path / "in.bgra"), str(tmp_path / "out.bgra")
    with open(fin, "wb") as f:
        f.write(clip.tobytes() + b"tail")                                          # a partial frame at the end is dropped
    args = [CLI, "-width", str(w), "--height", "0x28", "-gamma", "vga", "-underscan", "5", "-422", "-i", fin, "-o", fout]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    want = np.stack([R.align_frame(f)[0] for f in clip])
    got = np.fromfile(fout, dtype=np.uint8)
    assert got.size == want.size, "frames written: %r" % (got.size / (w * h * 4),)
    assert int((got.reshape(want.shape) != want).sum()) == 0
    assert int((want != clip).sum()) > 0                                           # the compare means something: rows moved
