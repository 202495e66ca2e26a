"""Checker of the vhsled stage: ffmpeg_vhsled.cpp:682-692 (blackish) and :866-931 (the frame body) restated in NumPy
and, a second time, as a scalar loop in plain Python integers.  tests/test_led_ref.py pins both to frames recorded from
the reference's own lines (tests/golden/led_ref.npz); the GPU tests compare the device with align_frame().

Frames are uint8 [H, W, 4] BGRA; a pixel as uint32 is B | G << 8 | R << 16 | A << 24 (little endian)."""
import numpy as np

RUN = 9


def px32(frame):
    return np.ascontiguousarray(frame).view(np.uint32)[:, :, 0]


def not_blackish(frame):
    """[H, W] bool: one of B, G, R exceeds the BLUE byte of the row's first pixel by 16 or more (:682-692; r is never
    shifted, so all three channels meet the same byte; a darker channel is blackish; the top byte plays no part)."""
    f = np.asarray(frame).astype(np.int32)
    ref = f[:, :1, 0:1]                                                           # blue of in[y][0]
    return ((f[:, :, :3] - ref) >= 16).any(axis=2)


def edges(frame):
    """e[y]: start of the first run of nine non-blackish pixels, W if there is none (:869-898)."""
    nb = not_blackish(frame)
    h, w = nb.shape
    if w < RUN:
        return np.full(h, w, np.int32)
    win = np.ones((h, w - RUN + 1), bool)
    for k in range(RUN):
        win &= nb[:, k:w - RUN + 1 + k]
    return np.where(win.any(axis=1), win.argmax(axis=1), w).astype(np.int32)


def smooth(e):
    """adj2 (:900-906) and x (:913) from e; int32 arithmetic (the sums stay inside it for W <= 3640)."""
    adj = e.astype(np.int64) << 16
    adj2 = adj.copy()
    h = len(e)
    if h > 8:
        s = np.zeros(h - 8, np.int64)
        for k in range(9):
            s += adj[k:h - 8 + k]
        assert int(s.max()) + 5 < (1 << 31)
        adj2[4:h - 4] = (s + 5) // 9                                              # non-negative: // truncates like the tool's /
    x = (adj2 + 0x8000) >> 16
    return adj2.astype(np.int32), x.astype(np.int32)


def align_frame(frame):
    """(out, e, x) of one frame."""
    src = px32(frame)
    h, w = src.shape
    e = edges(frame)
    _, x = smooth(e)
    out = src.copy()
    for y in range(h):
        xs = int(x[y])
        if xs < w // 2:                                                           # :921
            out[y, :w - xs] = src[y, xs:]
    return out.view(np.uint8).reshape(h, w, 4), e, x


def align_frame_scalar(frame):
    """The same, pixel by pixel in Python integers, in the shape of the tool's loops."""
    src = [[int(v) for v in row] for row in px32(frame)]
    h, w = len(src), len(src[0])

    def blackish(p, r):
        for _ in range(3):
            c = (p & 0xFF) - (r & 0xFF)
            if c >= 16:
                return False
            p >>= 8
        return True

    adj = []
    for y in range(h):
        count, x, bc = w, 0, 0
        while count > 0:
            if not blackish(src[y][x], src[y][0]):
                if bc >= 8:
                    x -= bc
                    break
                bc += 1
            else:
                bc = 0
            count -= 1
            x += 1
        adj.append(x << 16)
    adj2 = list(adj)
    for y in range(4, h - 4):
        adj2[y] = (sum(adj[y - 4:y + 5]) + 5) // 9
    out = np.empty((h, w), np.uint32)
    xs = []
    for y in range(h):
        x = (adj2[y] + 0x8000) >> 16
        xs.append(x)
        row = list(src[y])
        if x < w // 2:
            row[:w - x] = src[y][x:]
        out[y] = row
    return out.view(np.uint8).reshape(h, w, 4), np.array([a >> 16 for a in adj], np.int32), np.array(xs, np.int32)


# ---- test material ---------------------------------------------------------------------------------------------------

def dark_row(rng, w, blue=None):
    """A row that is blackish throughout: first pixel with blue `blue` (default 20 .. 60), every channel of every pixel
    below blue + 16; random top bytes."""
    b = int(rng.randint(20, 61)) if blue is None else blue
    row = np.zeros((w, 4), np.uint8)
    row[:, :3] = rng.randint(0, b + 16, size=(w, 3)).clip(0, 255)
    row[0, 0] = b
    row[0, 1:3] = rng.randint(0, b + 16, size=2).clip(0, 255)
    row[:, 3] = rng.randint(0, 256, size=w)
    return row


def bright(rng, n, blue):
    """n pixels that are not blackish against `blue` (< 240): one channel at least blue + 16."""
    p = np.zeros((n, 4), np.uint8)
    p[:, :3] = rng.randint(0, 256, size=(n, 3))
    ch = rng.randint(0, 3, size=n)
    p[np.arange(n), ch] = rng.randint(blue + 16, 256, size=n)
    p[:, 3] = rng.randint(0, 256, size=n)
    return p


def row_with_edge(rng, w, e, blue=None):
    """A dark row whose first run of nine non-blackish pixels starts at e (e + 9 <= w; e = w: none), bright to the end."""
    row = dark_row(rng, w, blue)
    b = int(row[0, 0])
    if e < w:
        assert e + RUN <= w
        row[e:] = bright(rng, w - e, b)
        if e == 0:
            row[0, 0] = b                                                         # pixel 0 keeps its blue: G or R carries it
            row[0, 1] = max(int(row[0, 1]), b + 16)
    return row


def frame_with_edges(rng, w, es, blue=None):
    return np.stack([row_with_edge(rng, w, int(e), blue) for e in es])


def capture_frame(rng, w, h, lo=None, hi=None):
    """Dark left borders of jittering length over random picture content, short bright runs (1 .. 8) inside the border."""
    lo = min(8, w // 8) if lo is None else lo
    hi = max(lo + 1, min(40, w // 3)) if hi is None else hi
    f = frame_with_edges(rng, w, rng.randint(lo, hi + 1, size=h))
    for y in range(h):
        e = int(edges(f[y:y + 1])[0])
        if e >= 12 and rng.randint(0, 2):
            n = int(rng.randint(1, 9))
            at = int(rng.randint(1, e - n - 1)) if e - n - 1 > 1 else 1
            if at + n < e:                                                        # a blackish pixel stays between the run and the edge
                f[y, at:at + n] = bright(rng, n, int(f[y, 0, 0]))
    return f
