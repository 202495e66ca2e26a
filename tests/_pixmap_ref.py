"""NumPy checker of the posterize and colormap stages: ffmpeg_posterize.cpp:789-813 and ffmpeg_colormap.cpp:785-822 of
the reference restated on uint8 [H, W, 4] BGRA frames (a pixel as uint32 is B | G<<8 | R<<16 | A<<24).  Pinned to runs
recorded from the reference's own lines by tests/test_pixmap_ref.py."""
import numpy as np


def _px(frame):
    """[H, W, 4] uint8 -> [H, W] uint32, a copy"""
    return np.ascontiguousarray(frame).view("<u4")[:, :, 0].copy()


def _bytes(px):
    """[H, W] uint32 -> [H, W, 4] uint8"""
    return np.ascontiguousarray(px.astype("<u4")).view(np.uint8).reshape(px.shape + (4,))


def mask_of(threshhold):
    """:796-797; the shift count is defined for 0 .. 8 only"""
    assert 0 <= threshhold <= 8
    return (((0xFF << (8 - threshhold)) & 0xFF) * 0x01010101) & 0xFFFFFFFF


def posterize(frame, threshhold):
    """composite_layer() :806-812: out = in & mask, alpha included"""
    return _bytes(_px(frame) & np.uint32(mask_of(threshhold)))


def identity_table():
    """ffmpeg_colormap.cpp:833"""
    return (np.arange(256, dtype=np.uint64) * 0x01010101).astype(np.uint32)


def take(map_frame):
    """take_colormap() :793-798: entry i is pixel (i * W) / 256 of row H / 2, a whole dword"""
    h, w = map_frame.shape[:2]
    return _px(map_frame)[h // 2, (np.arange(256) * w) // 256].astype(np.uint32)


def apply(frame, table):
    """composite_layer() :814-821: the green byte selects the output pixel"""
    return _bytes(np.asarray(table, dtype=np.uint32)[frame[:, :, 1]])


class ColorStream:
    """The tool's state over a clip: frame(src, map) is :1072-1075 for one output frame; map None: no second input."""

    def __init__(self, table=None):
        self.table = identity_table() if table is None else np.asarray(table, dtype=np.uint32).copy()

    def frame(self, src, map_frame=None):
        if map_frame is not None:
            self.table = take(map_frame)
        return apply(src, self.table)


def posterize_loop(inputs, threshholds):
    """ffmpeg_posterize.cpp:1035-1062 for one output frame: every input that has a frame (None: it has none) overwrites
    the whole output; None when no input has one (the tool's output frame then keeps what it held)."""
    out = None
    for f, t in zip(inputs, threshholds):
        if f is not None:
            out = posterize(f, t)
    return out
