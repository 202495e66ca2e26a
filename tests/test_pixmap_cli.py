"""posterize_cli and colormap_cli, the two tools' command lines on raw BGRA files, against the checker's statement of
the tools' loops: one frame of every input per output frame until every input has ended, an ended input keeping its
last frame, an input that never delivered one being the all-zero frame the tools allocate."""
import os
import subprocess

import numpy as np
import pytest

import _libs as L
import _pixmap_ref as R

POST = os.path.join(L.PKG, "posterize_cli")
CMAP = os.path.join(L.PKG, "colormap_cli")
W, H = 40, 6


def clip(seed, n):
    return np.random.RandomState(seed).randint(0, 256, size=(n, H, W, 4)).astype(np.uint8)


def write(path, frames, tail=b""):
    with open(str(path), "wb") as f:
        f.write(frames.tobytes() + tail)
    return str(path)


def run(cli, args, out, want):
    r = subprocess.run([cli, "-width", str(W), "--height", str(H)] + args + ["-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    got = np.fromfile(out, dtype=np.uint8)
    assert got.size == want.size, "frames written: %r" % (got.size / (W * H * 4),)
    assert int((got.reshape(want.shape) != want).sum()) == 0


@pytest.mark.parametrize("cli", [POST, CMAP])
def test_cli_refuses_like_the_tool(tmp_path, cli):
    """Switch errors end the program with 1 before any device is touched."""
    io = ["-i", "a", "-o", str(tmp_path / "o")]
    cases = [["-width", "31"] + io, ["-o", str(tmp_path / "o")], ["-i", "a"], ["-bogus"] + io, ["stray"] + io, ["-h"],
             ["-tvstd", "secam"] + io, ["-threshhold", "4"] + io, ["-height", "0"] + io]
    if cli == CMAP:
        cases.append(io + ["-threshhold", "4"])                                   # posterize's switch
    for args in cases:
        r = subprocess.run([cli] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 1, args
    assert not os.path.exists(str(tmp_path / "o"))


@pytest.mark.gpu
def test_colormap_cli_second_input_shorter(tmp_path):
    a, b = clip(1, 4), clip(2, 2)
    s = R.ColorStream()
    want = np.stack([s.frame(a[t], b[min(t, 1)]) for t in range(4)])              # the map's last frame persists
    assert (want[3] == R.apply(a[3], R.take(b[1]))).all() and (want != np.repeat(a[:, :, :, 1:2], 4, axis=3)).any()
    run(CMAP, ["-i", write(tmp_path / "a", a), "-i", write(tmp_path / "b", b, b"tail")], str(tmp_path / "o"), want)


@pytest.mark.gpu
def test_colormap_cli_one_input_and_an_empty_second_input(tmp_path):
    a = clip(3, 3)
    fa = write(tmp_path / "a", a)
    run(CMAP, ["-i", fa], str(tmp_path / "o1"), np.repeat(a[:, :, :, 1:2], 4, axis=3))    # identity grey from green
    # a second input that never delivers a frame is an all-zero frame, not an absent one: the table is all zero
    run(CMAP, ["-i", fa, "-i", write(tmp_path / "e", a[:0])], str(tmp_path / "o2"), np.zeros_like(a))


@pytest.mark.gpu
def test_posterize_cli_two_inputs_with_their_own_threshholds(tmp_path):
    a, b = clip(4, 4), clip(5, 2)
    fa, fb = write(tmp_path / "a", a), write(tmp_path / "b", b)
    want = np.stack([R.posterize_loop([a[t], b[min(t, 1)]], [2, 5]) for t in range(4)])
    assert (want[2] == R.posterize(b[1], 5)).all()
    run(POST, ["-i", fa, "-threshhold", "2", "-i", fb, "-threshhold", "5"], str(tmp_path / "o1"), want)
    # the other way round the longer input is the last: its own frames, its own threshhold; -i inherits the value
    run(POST, ["-i", fb, "-threshhold", "5", "-i", fa], str(tmp_path / "o2"), np.stack([R.posterize(f, 5) for f in a]))
    run(POST, ["-i", fa], str(tmp_path / "o3"), np.stack([R.posterize(f, 3) for f in a]))
