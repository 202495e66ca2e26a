"""Checker of the average_delay stage: a NumPy restatement of ffmpeg_average_delay.cpp's composite_layer() (:801-837)
and of its frame loop over the ring of destination frames (:948-970, :1069-1122).  Test infrastructure only: the
product never sees it.

Frames are uint8 [H, W, 4] BGRA; a pixel as the tool reads it is the little-endian uint32 of its four bytes.  The
arithmetic is written as the tool writes it -- s * n + d * (256 - n) + dither per channel, in uint32 that wraps -- not
in the rearranged form the kernels use."""
import numpy as np

M = 0xFFFFFFFF


def layer_flags(newlevel, name="x"):
    """The switches that make a layer of this newlevel (behind its -i)."""
    return ["-i", name, "-n", str(newlevel)]


def u32(frame):
    a = np.ascontiguousarray(frame)
    return a.view("<u4").reshape(a.shape[0], a.shape[1]).copy()


def bgra(px):
    return np.ascontiguousarray(px.astype("<u4")).view(np.uint8).reshape(px.shape[0], px.shape[1], 4)


def dither(h, w, field, delay):
    """[H, W] uint32: ((((x ^ y) + efield) & 3) * 255) / 3 with efield = field / delay in 64 bits (:802, :821)"""
    efield = (int(field) & 0xFFFFFFFFFFFFFFFF) // int(delay)
    x = np.arange(w, dtype=np.uint64)[None, :]
    y = np.arange(h, dtype=np.uint64)[:, None]
    return ((((x ^ y) + np.uint64(efield & 0xFFFFFFFF)) & np.uint64(3)) * np.uint64(255) // np.uint64(3)).astype(np.uint32)


def avg_layer(dst, src, newlevel, field, delay):
    """composite_layer() :815-836 on uint32 [H, W] arrays; dst is changed in place."""
    h, w = dst.shape
    n = np.uint32(int(newlevel) & M)                       # int -> unsigned int by the multiplication :819
    m = np.uint32((256 - int(newlevel)) & M)               # (256 - newlevel) is an int, converted likewise :820
    dth = dither(h, w, field, delay)
    out = np.zeros_like(dst)
    with np.errstate(over="ignore"):
        for shift in (16, 8, 0):
            s = (src >> np.uint32(shift)) & np.uint32(255)
            d = (dst >> np.uint32(shift)) & np.uint32(255)
            c = (s * n + d * m + dth) >> np.uint32(8)      # uint32 throughout: wraps like unsigned int
            out = out + (c << np.uint32(shift))            # :834 adds, it does not OR
    dst[...] = out


def avg_layer_scalar(dst, src, newlevel, field, delay):
    """The same, pixel by pixel in Python integers (for small frames: cross-checks the vectorised form)."""
    h, w = dst.shape
    n = int(newlevel) & M
    m = (256 - int(newlevel)) & M
    efield = int(field) // int(delay)
    for y in range(h):
        for x in range(w):
            sp, dp = int(src[y, x]), int(dst[y, x])
            dth = ((((x ^ y) + efield) & 3) * 255) // 3
            px = 0
            for shift in (16, 8, 0):
                c = ((((sp >> shift) & 255) * n) + (((dp >> shift) & 255) * m) + dth) & M
                px = (px + ((c >> 8) << shift)) & M
            dst[y, x] = px


def avg_frame(dst, srcs, levels, field, delay, scalar=False):
    """All layers of one output frame on a uint8 [H, W, 4] destination, in place; srcs[l] None = absent (:808: the
    destination stays as it is, top byte included).  All layers see the same field (:1069-1122)."""
    d = u32(dst)
    fn = avg_layer_scalar if scalar else avg_layer
    for src, n in zip(srcs, levels):
        if src is not None:
            fn(d, u32(src), n, field, delay)
    dst[...] = bgra(d)


def avg_clip(ring, frames, levels, ring_index=0, field=0):
    """The frame loop: frames[t][l] is layer l of output frame t (None: absent); ring is the list of `delay` destination
    frames, changed in place.  Returns (outputs [T, H, W, 4], ring_index, field) behind the clip."""
    out = []
    delay = len(ring)
    for srcs in frames:
        avg_frame(ring[ring_index], srcs, levels, field, delay)
        out.append(ring[ring_index].copy())
        ring_index = (ring_index + 1) % delay                                 # :1117-1118
        field += 1
    return (np.stack(out) if out else np.zeros((0,) + ring[0].shape, np.uint8)), ring_index, field


def make_frame(w, h, seed):
    """A source frame for the tests: random bytes (the top byte too), with runs of 0xFFFFFFFF and 0 pixels."""
    rs = np.random.RandomState(seed)
    f = rs.randint(0, 256, size=(h, w, 4)).astype(np.uint8)
    f[rs.random_sample((h, w)) < 0.08] = 255
    f[rs.random_sample((h, w)) < 0.08] = 0
    f[0, 0] = 255
    f[h - 1, w - 1] = 0
    return f
