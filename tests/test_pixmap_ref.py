"""The posterize / colormap checker (tests/_pixmap_ref.py) against runs recorded from the reference's own lines:
ffmpeg_posterize.cpp:789-813 and ffmpeg_colormap.cpp:785-822 compiled behind a stand-in frame, run on the inputs of
tests/golden/pixmap_ref.npz:
  post_<W>x<H>_src [H, W, 4], post_<W>x<H>_t<threshhold> [H, W, 4]: a source and its outputs;
  cmap_<W>x<H>_io [frame, 0 = source / 1 = map / 2 = output, H, W, 4], cmap_<W>x<H>_absent [frame] (1: the second input
  has no frame object; its map plane is zeros and was never shown to the tool), cmap_<W>x<H>_table [frame, 256]: the
  tool's colormap[] behind each frame of a clip that starts from the identity grey.
No GPU.  The recording must keep a case of every kind, so that it cannot quietly lose its coverage."""
import os

import numpy as np
import pytest

import _pixmap_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pixmap_ref.npz")
GEOMS = [(1, 1), (37, 5), (64, 2), (256, 3), (260, 18)]


@pytest.fixture(scope="module")
def recorded():
    z = np.load(GOLDEN)
    post, cmap = [], []
    for w, h in GEOMS:
        key = "%dx%d" % (w, h)
        src = z["post_%s_src" % key]
        assert src.shape == (h, w, 4)
        for name in sorted(n for n in z.files if n.startswith("post_%s_t" % key)):
            post.append((name, src, int(name.rsplit("_t", 1)[1]), z[name]))
        io, absent, table = z["cmap_%s_io" % key], z["cmap_%s_absent" % key], z["cmap_%s_table" % key]
        assert io.shape[1:] == (3, h, w, 4) and absent.shape == (len(io),) and table.shape == (len(io), 256)
        cmap.append((key, io, absent, table))
    return post, cmap


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 200 * 1024


def test_checker_reproduces_every_recorded_run(recorded):
    post, cmap = recorded
    for name, src, t, want in post:
        assert int((R.posterize(src, t) != want).sum()) == 0, name
    for key, io, absent, table in cmap:
        s = R.ColorStream()
        for i in range(len(io)):
            got = s.frame(io[i, 0], None if absent[i] else io[i, 1])
            assert (s.table == table[i]).all(), "%s frame %d: table" % (key, i)
            assert int((got != io[i, 2]).sum()) == 0, "%s frame %d" % (key, i)


def test_recording_covers_every_kind_of_case(recorded):
    post, cmap = recorded
    kinds = {"t0_clears": 0, "t1": 0, "t3": 0, "t8_copies": 0, "alpha_bits_masked": 0,
             "width_below_256": 0, "width_256": 0, "width_above_256_not_a_multiple": 0,
             "odd_height": 0, "even_height": 0, "height_1": 0, "map_alpha_in_output": 0, "only_green_counts": 0,
             "absent_after_present_keeps_table": 0, "absent_first_identity_grey": 0, "rows_other_than_the_middle_ignored": 0}
    for name, src, t, want in post:
        kinds["t0_clears"] += int(t == 0 and not want.any() and src.any())
        kinds["t1"] += int(t == 1 and set(np.unique(want)) <= {0, 0x80})
        kinds["t3"] += int(t == 3)
        kinds["t8_copies"] += int(t == 8 and (want == src).all())
        kinds["alpha_bits_masked"] += int(0 < t < 8 and (src[:, :, 3] & ~want[:, :, 3]).any() and want[:, :, 3].any())
    for key, io, absent, table in cmap:
        h, w = io.shape[2:4]
        took = absent == 0
        kinds["width_below_256"] += int(w < 256 and took.any() and len(set((np.arange(256) * w) // 256)) < 256)
        kinds["width_256"] += int(w == 256 and took.any())
        kinds["width_above_256_not_a_multiple"] += int(w > 256 and w % 256 != 0 and took.any())
        kinds["odd_height"] += int(h % 2 == 1 and h > 1 and took.any())
        kinds["even_height"] += int(h % 2 == 0 and took.any())
        kinds["height_1"] += int(h == 1 and took.any())
        for i in range(len(io)):
            src, m, out = io[i]
            if took[i]:
                kinds["map_alpha_in_output"] += int(m[h // 2, :, 3].any() and out[:, :, 3].any()
                                                    and (out[:, :, 3] == (table[i] >> 24).astype(np.uint8)[src[:, :, 1]]).all())
                others = np.delete(m, h // 2, axis=0)
                kinds["rows_other_than_the_middle_ignored"] += int(others.size > 0 and (others != m[h // 2]).any())
            else:
                assert not m.any()
            if (src[:, :, 0] != src[:, :, 1]).any() and (src[:, :, 2] != src[:, :, 1]).any():
                grey = src.copy()
                grey[:, :, 0] = grey[:, :, 2] = grey[:, :, 3] = src[:, :, 1]
                kinds["only_green_counts"] += int((R.apply(grey, table[i]) == out).all())
            if not took[i] and i > 0 and took[:i].any():
                kinds["absent_after_present_keeps_table"] += int((table[i] == table[i - 1]).all() and (table[i] != R.identity_table()).any())
            if not took[i] and not took[:i].any():
                kinds["absent_first_identity_grey"] += int((table[i] == R.identity_table()).all() and (out == src[:, :, 1:2]).all())
    assert all(v > 0 for v in kinds.values()), kinds
