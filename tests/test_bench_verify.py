"""tools/bench_verify.py, the verification step of the stage benchmarks, without a GPU: its block-wise rand() stream is
the checker's, and its two compare loops pick the frames they say and stop the tool on the first wrong byte."""
import os
import sys

import numpy as np
import pytest

import _key_ref as RK
import _libs as L

sys.path.insert(0, os.path.join(L.ROOT, "tools"))
import bench_verify as V  # noqa: E402


def test_block_rand_is_the_checkers_stream():
    fast, slow = V.block_rand(RK.GlibcRand), RK.GlibcRand()
    for pos, n in ((0, 1), (0, 5000), (4999, 3), (123457, 300), (400000, 31)):      # inside, across and far behind a block
        assert fast.draws(pos, n).tolist() == slow.draws(pos, n).tolist()
        assert fast.draws(pos, n).dtype == slow.draws(pos, n).dtype
    for pos in (0, 1, 30, 31, 344, 250000):
        assert fast.window(pos) == slow.window(pos)
    assert fast.draws(7, 50).tolist() == slow.draws(7, 50).tolist()                  # going back after going far
    # blocks of 256 words and a stretch that is cut every 1000: words behind the request are dropped on the way
    small = V.block_rand(RK.GlibcRand, maxlog=8, slack=1000)
    for pos, n in ((0, 10), (5000, 700), (5100, 3), (40000, 2000), (300000, 31), (7, 50), (299990, 100)):
        assert small.draws(pos, n).tolist() == slow.draws(pos, n).tolist()
        assert small.window(pos) == slow.window(pos)
        assert len(small.a) < n + 2 * 1000 + 2 * (256 + 31) + 344 and (pos < 5000 or small.at > 0)


def test_sample_frames():
    assert V.sample_frames(600) == [0, 1, 300, 599]
    assert V.sample_frames(3) == [0, 1, 2] and V.sample_frames(1) == [0] and V.sample_frames(0) == []


def test_verify_frames_and_clip_stop_on_a_wrong_byte(monkeypatch):
    frames = [np.full((2, 3, 4), k, np.uint8) for k in range(9)]
    v = V.verify_frames(9, lambda k: frames[k], lambda k: frames[k].copy(), "case")
    assert v["frames_verified"] == [0, 1, 4, 8] and v["verify_s"] >= 0
    wrong = frames[4].copy()
    wrong[1, 2, 3] ^= 1
    with pytest.raises(SystemExit) as e:
        V.verify_frames(9, lambda k: frames[k], lambda k: wrong if k == 4 else frames[k], "case")
    assert e.value.code not in (0, None) and "frame 4" in str(e.value.code)

    # a clip whose frame t adds t + 1 to its ring frame: delay 2, T = 9
    def step(dst, t):
        dst += np.uint8(t + 1)

    ring = [np.zeros((2, 3, 4), np.uint8) for _ in range(2)]
    outs = []
    for t in range(9):
        step(ring[t % 2], t)
        outs.append(ring[t % 2].copy())
    v = V.verify_clip(9, 2, (2, 3, 4), step, lambda t: outs[t], lambda i: ring[i], "clip")
    assert v["frames_verified"] == list(range(9))                                    # fast enough for the whole clip
    with pytest.raises(SystemExit):
        V.verify_clip(9, 2, (2, 3, 4), step, lambda t: outs[t], lambda i: ring[1 - i], "clip")   # the ring behind it
    monkeypatch.setattr(V, "WHOLE_CLIP_S", -1.0)                                     # no time for more than the prefix
    v = V.verify_clip(9, 2, (2, 3, 4), step, lambda t: outs[t], lambda i: ring[1 - i], "clip")
    assert v["frames_verified"] == list(range(2 * 2 + 3))
    with pytest.raises(SystemExit):
        V.verify_clip(9, 2, (2, 3, 4), step, lambda t: outs[t if t != 6 else 5], lambda i: ring[i], "clip")
