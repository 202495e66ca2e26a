"""Checker of the colorkey stage: a NumPy / Python restatement of ffmpeg_colorkey.cpp's composite_layer() (:844-885)
and of its frame loop over the ring of destination frames (:1013-1016, :1118-1171), with glibc's unseeded rand()
written out from the recurrence csrc/glibc_rand.hpp documents.  Test infrastructure only: the product never sees it.

Frames are uint8 [H, W, 4] BGRA; a pixel as the tool reads it is the little-endian uint32 of its four bytes."""
import numpy as np

LAYER_DEFAULTS = dict(color=0, threshhold=0, fade=0, xdivr=1, invert=0, noisekey=0)      # InputFile() :68


def layer(**kw):
    d = dict(LAYER_DEFAULTS)
    for k, v in kw.items():
        assert k in d, k
        d[k] = v
    return d


def layer_flags(lay, name="x"):
    """The switches that make this layer (behind its -i)."""
    return ["-i", name, "-color", "0x%X" % lay["color"], "-threshhold", str(lay["threshhold"]), "-f", str(lay["fade"]),
            "-xd", str(lay["xdivr"]), "-inv", str(lay["invert"]), "-noise", str(lay["noisekey"])]


# ---- rand(): glibc TYPE_3, seed 1.  s[i] = s[i-31] + s[i-3] (mod 2^32); the k-th rand() returns s[344+k] >> 1 ------
class GlibcRand:
    def __init__(self):
        s = [0] * 34
        word = 1
        s[0] = 1
        for i in range(1, 31):                      # the minimal-standard LCG in Schrage's form
            hi, lo = divmod(word, 127773)
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            s[i] = word
        for i in range(31, 34):
            s[i] = s[i - 31]
        self.s = s
        self._extend(344)

    def _extend(self, n):
        s = self.s
        i = len(s)
        if n <= i:
            return
        s.extend([0] * (n - i))
        while i < n:
            s[i] = (s[i - 31] + s[i - 3]) & 0xFFFFFFFF
            i += 1

    def draws(self, pos, n):
        """rand() number pos .. pos + n - 1 as uint32"""
        self._extend(344 + pos + n)
        return np.array(self.s[344 + pos:344 + pos + n], dtype=np.uint64).astype(np.uint32) >> np.uint32(1)

    def window(self, pos):
        """the 31 words the generator holds at position pos: w[j] = s[313 + pos + j] (csrc/glibc_rand.hpp RandState)"""
        self._extend(344 + pos)
        return list(self.s[313 + pos:344 + pos])


RAND = GlibcRand()          # one stream for the whole test session, extended on demand


def u32(frame):
    a = np.ascontiguousarray(frame)
    return a.view("<u4").reshape(a.shape[0], a.shape[1]).copy()


def bgra(px):
    return np.ascontiguousarray(px.astype("<u4")).view(np.uint8).reshape(px.shape[0], px.shape[1], 4)


def noise_hits(lay, h, w, pos):
    """[H, W] bool: the hit of :861-863 at every pixel, draws pos .. pos + 3*W*H - 1 in raster order"""
    r = RAND.draws(pos, 3 * w * h).reshape(h, w, 3)
    x = (r[:, :, 0] * r[:, :, 1] * r[:, :, 2]) % np.uint32(20001)            # uint32 products wrap like unsigned int
    return x < np.uint32(min(lay["noisekey"], 0xFFFFFFFF))


def key_layer(dst, src, lay, pos=0):
    """composite_layer() :844-885 on uint32 [H, W] arrays; dst is changed in place.  Returns the position behind."""
    h, w = dst.shape
    xd = max(1, lay["xdivr"] & 0xFFFFFFFF)
    xs = np.arange(w)
    start = xs - xs % xd                                                     # where xdivc was last 0 (:847, :853, :883)
    s = src.astype(np.int64)
    key = lay["color"]
    dist = (np.abs(((s >> 16) & 255) - ((key >> 16) & 255)) + np.abs(((s >> 8) & 255) - ((key >> 8) & 255)) +
            np.abs((s & 255) - (key & 255)))
    d = dist[:, start]
    if lay["noisekey"] > 0:
        hit = noise_hits(lay, h, w, pos)
        last = np.maximum.accumulate(np.where(hit, xs[None, :], -1), axis=1)  # x of the last hit at or left of x
        d = np.where(last >= start[None, :], 0xFFFF, d)                        # held until the next recomputation
        pos += 3 * w * h
    if lay["fade"] != 0:
        f = np.uint32((256 - lay["fade"]) & 0xFFFFFFFF)                        # unsigned int: fade > 256 wraps
        r = (((dst >> np.uint32(16)) & np.uint32(255)) * f) >> np.uint32(8)
        g = (((dst >> np.uint32(8)) & np.uint32(255)) * f) >> np.uint32(8)
        b = ((dst & np.uint32(255)) * f) >> np.uint32(8)
        dst[...] = (r << np.uint32(16)) + (g << np.uint32(8)) + b
    copy = (d < lay["threshhold"]) if lay["invert"] else (d >= lay["threshhold"])
    dst[copy] = src[copy]
    return pos


def key_layer_scalar(dst, src, lay, pos=0):
    """The same, pixel by pixel in the tool's own order (for small frames: cross-checks the vectorised form)."""
    h, w = dst.shape
    M = 0xFFFFFFFF
    nk, fade, thr, key, xdivr = lay["noisekey"], lay["fade"], lay["threshhold"], lay["color"], lay["xdivr"]
    rnd = RAND.draws(pos, 3 * w * h).tolist() if nk > 0 else None
    k = 0
    d = 0
    for y in range(h):
        xdivc = 0
        for x in range(w):
            sp = int(src[y, x])
            if xdivc == 0:
                d = (abs(((sp >> 16) & 255) - ((key >> 16) & 255)) + abs(((sp >> 8) & 255) - ((key >> 8) & 255)) +
                     abs((sp & 255) - (key & 255)))
            if nk > 0:
                v = (((rnd[k] * rnd[k + 1]) & M) * rnd[k + 2]) & M
                k += 3
                if v % 20001 < nk:
                    d = 0xFFFF
            if fade != 0:
                dp = int(dst[y, x])
                f = (256 - fade) & M
                r = ((((dp >> 16) & 255) * f) & M) >> 8
                g = ((((dp >> 8) & 255) * f) & M) >> 8
                b = (((dp & 255) * f) & M) >> 8
                dst[y, x] = (((r << 16) & M) + ((g << 8) & M) + b) & M
            if (d < thr) if lay["invert"] else (d >= thr):
                dst[y, x] = sp
            xdivc += 1
            if xdivc >= xdivr:
                xdivc = 0
    return pos + (3 * w * h if nk > 0 else 0)


def key_frame(dst, srcs, layers, pos=0, scalar=False):
    """All layers of one output frame (:1119-1146) on a uint8 [H, W, 4] destination, in place; srcs[l] None = absent
    (the early return :837-842: no draws).  Returns the position behind the frame."""
    d = u32(dst)
    fn = key_layer_scalar if scalar else key_layer
    for src, lay in zip(srcs, layers):
        if src is not None:
            pos = fn(d, u32(src), lay, pos)
    dst[...] = bgra(d)
    return pos


def rand_advance(layers, w, h, pos, present=None):
    for l, lay in enumerate(layers):
        if (present is None or present[l]) and lay["noisekey"] > 0:
            pos += 3 * w * h
    return pos


def key_clip(ring, frames, layers, ring_index=0, pos=0):
    """The frame loop :1118-1171: frames[t][l] is layer l of output frame t (None: absent); ring is the list of
    `delay` destination frames, changed in place.  Returns (outputs [T, H, W, 4], ring_index, pos) behind the clip."""
    out = []
    for srcs in frames:
        pos = key_frame(ring[ring_index], srcs, layers, pos)
        out.append(ring[ring_index].copy())
        ring_index = (ring_index + 1) % len(ring)                             # :1166-1167
    return (np.stack(out) if out else np.zeros((0,) + ring[0].shape, np.uint8)), ring_index, pos


def make_frame(w, h, seed, key=0x00FF00, near=0.5, spread=120):
    """A source frame for the tests: about `near` of its pixels lie within `spread` of the key colour (so that
    thresholds between 1 and 765 split them), the rest anywhere; the alpha byte is random too."""
    rs = np.random.RandomState(seed)
    f = rs.randint(0, 256, size=(h, w, 4)).astype(np.int64)
    kc = np.array([key & 255, (key >> 8) & 255, (key >> 16) & 255])
    nearpx = np.clip(kc[None, None, :] + rs.randint(-spread // 3, spread // 3 + 1, size=(h, w, 3)), 0, 255)
    exact = rs.random_sample((h, w)) < 0.15
    nearpx[exact] = kc
    m = rs.random_sample((h, w)) < near
    f[:, :, :3][m] = nearpx[m]
    return f.astype(np.uint8)
