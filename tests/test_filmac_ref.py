"""The filmac checker (tests/_filmac_ref.py) against runs recorded from the reference's own lines: filmac.cpp:633-680 and
:857-1006 compiled behind a stand-in frame, run on the clips of tests/golden/filmac_ref.npz (io_<W>x<H>_<n|g>_<clip>:
[frame, 0 = source / 1 = output, H, W, 4]; lv_...: [frame, (minv, maxv, final_minv, final_maxv)]; n: no -gamma, g:
-gamma 2.2).  No GPU.  The recording must keep a frame of every kind, so that it cannot quietly lose its coverage."""
import os

import numpy as np
import pytest

import _filmac_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filmac_ref.npz")
GEOMS = [(32, 32), (160, 130), (345, 129)]
GAMMAS = {"n": -1.0, "g": 2.2}


@pytest.fixture(scope="module")
def recorded():
    """[(key, gamma, sources, outputs, levels)], one per recorded run"""
    z = np.load(GOLDEN)
    runs = []
    for key in sorted(k[3:] for k in z.files if k.startswith("io_")):
        io, lv = z["io_" + key], z["lv_" + key]
        size, tag, _ = key.split("_")
        w, h = (int(v) for v in size.split("x"))
        assert io.shape[1:] == (2, h, w, 4) and lv.shape == (io.shape[0], 4)
        runs.append((key, GAMMAS[tag], io[:, 0], io[:, 1], lv))
    assert {(r[2].shape[2], r[2].shape[1], r[1]) for r in runs} >= {(w, h, g) for (w, h) in GEOMS for g in GAMMAS.values()}
    return runs


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 200 * 1024


def test_checker_reproduces_every_recorded_run(recorded):
    for key, gamma, src, want, lv in recorded:
        outs, levels, _ = R.run(src, gamma)
        for i in range(len(src)):
            assert levels[i] == tuple(int(v) for v in lv[i]), "%s frame %d: levels" % (key, i)
            assert int((outs[i] != want[i]).sum()) == 0, "%s frame %d" % (key, i)


def test_scalar_and_vectorised_forms_agree(recorded):
    for key, gamma, src, want, lv in recorded:
        if src.shape[2] > 32:
            src, want, lv = src[:2], want[:2], lv[:2]                             # the scalar form is slow: whole runs at 32 x 32 only
        a, b = R.Stream(gamma), R.Stream(gamma)
        for i, f in enumerate(src):
            oa, la = a.frame(f)
            ob, lb = b.frame_scalar(f)
            assert la == lb == tuple(int(v) for v in lv[i]), "%s frame %d" % (key, i)
            assert (oa == ob).all() and (ob == want[i]).all(), "%s frame %d" % (key, i)


def test_recording_covers_every_kind_of_frame(recorded):
    kinds = {"first": 0, "max_up": 0, "max_down": 0, "min_down": 0, "min_up": 0, "minv_eq_maxv_black": 0,
             "brightest_left_of_blocks": 0, "brightest_right_of_90_percent": 0, "block_row_clipped_by_height": 0,
             "block_clipped_by_width": 0, "below_zero": 0, "clamp_high": 0, "clamp_low": 0, "alpha_replaced": 0}
    for key, gamma, src, want, lv in recorded:
        s = R.Stream(gamma)
        h, w = src.shape[1:3]
        xs, ys = R.block_origins(w, h)
        for i, f in enumerate(src):
            out, (minv, maxv, fmin, fmax) = s.frame(f)
            start_min, start_max = (s.scale * 6) // 10, (s.scale * 4) // 10
            if maxv == minv + 1 and gamma < 1 and (f[:, :, :3] == 128).all():
                assert (want[i][:, :, :3] == 0).all()
                kinds["minv_eq_maxv_black"] += 1
            top = f[:, :, :3].max(axis=2)
            cols = np.nonzero((top == top.max()).any(axis=0))[0]
            if cols.max() < xs[0] and int(s.lut[top.max()]) > maxv:                # brightest pixel not measured
                kinds["brightest_left_of_blocks"] += 1
            if cols.min() >= (w * 90) // 100 and int(s.lut[top.max()]) == maxv and maxv > start_max:
                kinds["brightest_right_of_90_percent"] += 1
            kinds["block_row_clipped_by_height"] += int(h % R.BLOCK != 0 and len(ys) > 1)
            kinds["block_clipped_by_width"] += int(xs[-1] + R.BLOCK > w)
            for k, v in s.kinds_of(f).items():
                kinds[k] += int(v)
            kinds["alpha_replaced"] += int((f[:, :, 3] != 0xFF).any() and (want[i][:, :, 3] == 0xFF).all())
        for k, v in s.branches.items():
            kinds[k] += v
    assert all(v > 0 for v in kinds.values()), kinds
