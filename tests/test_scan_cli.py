"""scanimate_cli, the tool's command line on raw BGRA files: three -inntsc source frames in, three fields out -- the
output byte stream is the checker's, with row 0 of the field == 1 outputs zero as the tool's memset leaves it."""
import os
import subprocess

import numpy as np
import pytest

import _libs as L
import _scan_ref as R

CLI = os.path.join(L.PKG, "scanimate_cli")


def test_cli_refuses_like_the_tool(tmp_path):
    """Switch errors end the program with 1 before any device is touched."""
    for args in (["-width", "31", "-i", "a", "-o", "b"], ["-o", str(tmp_path / "o")], ["-i", "a"], ["-tvstd"], ["-bogus"], ["-h"]):
        r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1, args


@pytest.mark.gpu
def test_cli_equals_checker(tmp_path):
    w, h, sw, sh = 240, 160, 480, 480                                              # -inntsc: the source size the tool derives
    clip = np.stack([R.make_source(sw, sh, 900 + t) for t in range(3)])
    fin, fout = str(tmp_path / "in.bgra"), str(tmp_path / "out.bgra")
    clip.tofile(fin)
    args = [CLI, "-inntsc", "-width", str(w), "-height", str(h), "-i", str(tmp_path / "unread.bgra"), "-i", fin, "-o", fout]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    want = np.stack([R.scan_field(clip[t], w, h, 1, t)[1] for t in range(3)])
    got = np.fromfile(fout, dtype=np.uint8)
    assert got.size == want.size, "fields written: %r" % (got.size / (w * h * 4),)
    assert int((got.reshape(want.shape) != want).sum()) == 0
    assert int(want[0][0].max()) == 0 and int(want[1][0, :, 3].min()) == 255       # field numbers 0 / 1: field 1 / 0
    lit, sat = int((want[..., 0] > 0).sum()), int((want[..., 0] == 255).sum())
    assert lit > 50000 and sat < 0.05 * lit                                       # the compare means something: lit, hardly saturated
