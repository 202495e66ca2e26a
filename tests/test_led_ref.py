"""The vhsled checker (tests/_led_ref.py) against frames recorded from the reference's own lines: ffmpeg_vhsled.cpp
:682-692 and :866-931 compiled behind a stand-in AVFrame, run on the frames of tests/golden/led_ref.npz (io_WxH:
[frame, row, 0 = source / 1 = output, W, 4]).  No GPU.  The recording must keep a row of every kind, so that it cannot
quietly lose its coverage."""
import os

import numpy as np
import pytest

import _led_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "led_ref.npz")
GEOMS = [(16, 16), (64, 16), (65, 17), (96, 32), (130, 21), (200, 40)]


@pytest.fixture(scope="module")
def recorded():
    z = np.load(GOLDEN)
    out = []
    for (w, h) in GEOMS:
        io = z["io_%dx%d" % (w, h)]
        assert io.shape[1:] == (h, 2, w, 4) and io.shape[0] >= 2
        out += [(np.ascontiguousarray(f[:, 0]), np.ascontiguousarray(f[:, 1])) for f in io]
    return out


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 200 * 1024


def test_checker_reproduces_every_recorded_frame(recorded):
    for i, (src, want) in enumerate(recorded):
        got, _, _ = R.align_frame(src)
        assert int((got != want).sum()) == 0, "frame %d (%dx%d)" % (i, src.shape[1], src.shape[0])


def test_scalar_and_vectorised_forms_agree(recorded):
    for i, (src, want) in enumerate(recorded):
        a, ea, xa = R.align_frame(src)
        b, eb, xb = R.align_frame_scalar(src)
        assert int((b != want).sum()) == 0, "frame %d" % i
        assert (ea == eb).all() and (xa == xb).all() and (a == b).all(), "frame %d" % i


def test_recording_covers_every_kind_of_row(recorded):
    kinds = {"x0": 0, "shifted": 0, "unshifted": 0, "no_edge": 0, "blue0": 0, "blue255": 0, "dark_frame": 0, "short_run": 0}
    for src, want in recorded:
        h, w = src.shape[:2]
        _, e, x = R.align_frame(src)
        kinds["x0"] += int((x == 0).sum())
        kinds["shifted"] += int(((x > 0) & (x < w // 2)).sum())
        kinds["unshifted"] += int((x >= w // 2).sum())
        kinds["no_edge"] += int((e == w).sum())
        kinds["blue0"] += int(((src[:, 0, 0] == 0) & (src[:, 0, 1:3].max(axis=1) >= 100)).sum())
        kinds["blue255"] += int((src[:, 0, 0] == 255).sum())
        kinds["dark_frame"] += int((e == w).all())
        nb = R.not_blackish(src)
        for y in range(h):                                                        # a bright run of 1 .. 8 in front of the edge
            if 9 <= e[y] < w and nb[y, :e[y]].any():
                kinds["short_run"] += 1
        moved = (x > 0) & (x < w // 2)
        if moved.any():                                                           # a shifted row differs from its source
            assert (want[moved] != src[moved]).any()
    assert all(v > 0 for v in kinds.values()), kinds
