"""average_delay_cli, the tool's command line on raw BGRA files: two layers of different length, a ring of two frames,
an in-range and a wrapping level -- the output byte stream is the checker's loop."""
import os
import subprocess

import numpy as np
import pytest

import _avg_ref as R
import _libs as L

CLI = os.path.join(L.PKG, "average_delay_cli")


def test_cli_refuses_like_the_tool(tmp_path):
    """Switch errors end the program with 1 before any device is touched."""
    for args in (["-d", "0"], ["-o", str(tmp_path / "o")], ["-n", "8", "-i", "a", "-o", "b"], ["-bogus"], ["-h"]):
        r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1, args


@pytest.mark.gpu
def test_cli_equals_checker_loop(tmp_path):
    w, h = 100, 35
    n = (9, 5)                                                                     # the second layer ends first and keeps its last frame
    clips = [np.stack([R.make_frame(w, h, 300 + 20 * l + t) for t in range(n[l])]) for l in range(2)]
    paths = [str(tmp_path / ("in%d.bgra" % l)) for l in range(2)]
    for c, p in zip(clips, paths):
        c.tofile(p)
    fout = str(tmp_path / "out.bgra")
    args = [CLI, "-width", str(w), "-height", str(h), "-d", "2", "-i", paths[0], "-n", "96", "-i", paths[1], "-n", "300", "-o", fout]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    T = max(n)
    frames = [[clips[l][min(t, n[l] - 1)] for l in range(2)] for t in range(T)]
    ring = [np.zeros((h, w, 4), np.uint8) for _ in range(2)]
    want, _, _ = R.avg_clip(ring, frames, [96, 300])
    got = np.fromfile(fout, dtype=np.uint8)
    assert got.size == want.size, "frames written: %r" % (got.size / (w * h * 4),)
    assert int((got.reshape(want.shape) != want).sum()) == 0
