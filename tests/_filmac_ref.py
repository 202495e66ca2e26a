"""Checker of the filmac stage: filmac.cpp:857-1006 (the frame body) with :633-680 (clamp255 and the gamma tables)
restated twice -- vectorised in NumPy with the stretch as a 256-entry table, and as a scalar loop in plain Python
integers in the shape of the tool's loops.  tests/test_filmac_ref.py pins both to frames recorded from the reference's
own lines (tests/golden/filmac_ref.npz); the GPU tests compare the device with Stream.

Frames are uint8 [H, W, 4] BGRA.  A Stream is one run of the tool: it carries (final_init, final_minv, final_maxv),
asserts final_maxv > final_minv for every frame and counts which branch of the recurrence each frame took."""
import math

import numpy as np

BLOCK = 128


def tdiv(a, b):
    """C's integer division: truncates toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def gamma_tables(gamma):
    """gamma16_do_init() :672-680 with the host's pow()"""
    dec = [int(math.pow(i / 255.0, gamma) * 8192) for i in range(256)]
    enc = [int(math.pow(i / 8192.0, 1.0 / gamma) * 255) for i in range(8193)]
    return dec, enc


def block_origins(w, h):
    """(xs, ys) of the 128 x 128 blocks :891-898, in unsigned arithmetic; blocks are clipped by the frame alone"""
    minx, maxx = (w * 15) // 100, (w * 90) // 100
    return list(range(minx, maxx, BLOCK)), list(range(0, h, BLOCK))


def last_measured_x(w):
    """the last column of the last block of a row: at or right of w*90/100 unless the blocks end exactly there"""
    return min(w, block_origins(w, 1)[0][-1] + BLOCK) - 1


class Stream:
    def __init__(self, gamma=-1.0, strict=True):
        """strict=False: a state that only ntscsim_filmac_set_state() can bring about is followed as the stage defines it
        (a denominator of 0 counts as 1, a negative one divides as C does) instead of failing the assertion"""
        self.strict = strict
        self.use_gamma = gamma > 1                                                # :859
        self.dec, self.enc = gamma_tables(gamma) if self.use_gamma else (list(range(256)), None)
        self.scale = 0x10000 * 8192 if self.use_gamma else 0x10000 * 256          # :886
        self.lut = np.array(self.dec, np.int64) << 16                            # L of a byte :866 / :879
        self.reset()

    def reset(self):
        self.init, self.fmin, self.fmax = False, -1, -1                           # :828-829
        self.branches = {"first": 0, "max_up": 0, "max_down": 0, "min_down": 0, "min_up": 0}

    # ---- the three parts -------------------------------------------------------------------------------------

    def frame_levels(self, frame):
        """(minv, maxv) :887-925"""
        h, w = frame.shape[:2]
        lo = self.lut[frame[:, :, :3].min(axis=2)]                                # the decode table does not decrease
        hi = self.lut[frame[:, :, :3].max(axis=2)]
        minv, maxv = (self.scale * 6) // 10, (self.scale * 4) // 10
        xs, ys = block_origins(w, h)
        for y in ys:
            for x in xs:
                blo, bhi = lo[y:y + BLOCK, x:x + BLOCK], hi[y:y + BLOCK, x:x + BLOCK]
                grd = blo.size
                maxv = max(maxv, int(bhi.max()))
                minv = min(minv, (int(blo.sum()) + grd // 2) // grd)
        if minv == maxv:
            maxv += 1
        return minv, maxv

    def step(self, minv, maxv):
        """:927-942"""
        if not self.init:
            self.init, self.fmin, self.fmax = True, minv, maxv
            self.branches["first"] += 1
        else:
            if self.fmax < maxv:
                self.fmax = tdiv(self.fmax + maxv, 2)
                self.branches["max_up"] += 1
            else:
                self.fmax = tdiv(self.fmax * 4 + maxv, 5)
                self.branches["max_down"] += 1
            if self.fmin > minv:
                self.fmin = tdiv(self.fmin + minv, 2)
                self.branches["min_down"] += 1
            else:
                self.fmin = tdiv(self.fmin * 4 + minv, 5)
                self.branches["min_up"] += 1
        assert self.fmax > self.fmin or not self.strict, (self.fmin, self.fmax)
        return self.fmin, self.fmax

    def stretched(self, byte):
        """v of one input byte before the clamp :949"""
        return tdiv((self.dec[byte] * 65536 - self.fmin) * self.scale, (self.fmax - self.fmin) or 1)

    def out_byte(self, byte):
        """:949-951 and :986 / :1000"""
        v = max(-0x7FFFFFFF, min(0x7FFFFFFF, self.stretched(byte)))
        t = max(0, v >> 16)
        if self.use_gamma:
            return min(255, self.enc[min(t, 8192)])
        return min(255, t)

    def table(self):
        return np.array([self.out_byte(b) for b in range(256)], np.uint8)

    # ---- a frame ---------------------------------------------------------------------------------------------

    def frame(self, frame):
        """(out, (minv, maxv, final_minv, final_maxv)) of the next frame of the run"""
        minv, maxv = self.frame_levels(frame)
        fmin, fmax = self.step(minv, maxv)
        out = np.empty_like(frame)
        out[:, :, :3] = self.table()[frame[:, :, :3]]
        out[:, :, 3] = 0xFF
        return out, (minv, maxv, fmin, fmax)

    def frame_scalar(self, frame):
        """The same, pixel by pixel in Python integers, in the shape of the tool's loops."""
        h, w = frame.shape[:2]
        px = frame.tolist()
        L = [[[self.dec[px[y][x][c]] << 16 for c in range(3)] for x in range(w)] for y in range(h)]
        minv, maxv = (self.scale * 6) // 10, (self.scale * 4) // 10
        minx, maxx = (w * 15) // 100, (w * 90) // 100
        y = 0
        while y < h:
            x = minx
            while x < maxx:
                grmin = grd = 0
                for sy in range(BLOCK):
                    for sx in range(BLOCK):
                        if x + sx >= w or y + sy >= h:
                            continue
                        grd += 1
                        grmin += min(L[y + sy][x + sx])
                        maxv = max(maxv, max(L[y + sy][x + sx]))
                grmin = tdiv(grmin + grd // 2, grd)
                if minv > grmin:
                    minv = grmin
                x += BLOCK
            y += BLOCK
        if minv == maxv:
            maxv += 1
        fmin, fmax = self.step(minv, maxv)
        out = np.empty_like(frame)
        for y in range(h):
            for x in range(w):
                for c in range(3):
                    v = tdiv((L[y][x][c] - fmin) * self.scale, fmax - fmin)
                    v = max(-0x7FFFFFFF, min(0x7FFFFFFF, v))
                    t = max(0, v >> 16)
                    out[y, x, c] = min(255, self.enc[min(t, 8192)]) if self.use_gamma else min(255, t)
                out[y, x, 3] = 0xFF
        return out, (minv, maxv, fmin, fmax)

    def kinds_of(self, frame):
        """What the frame just processed exercised: a stretch result below 0, below and above the clamp."""
        vs = [self.stretched(int(b)) for b in np.unique(frame[:, :, :3])]
        return {"below_zero": any(v < 0 for v in vs), "clamp_low": any(v < -0x7FFFFFFF for v in vs),
                "clamp_high": any(v > 0x7FFFFFFF for v in vs)}


def run(frames, gamma=-1.0, stream=None):
    """([out], [(minv, maxv, final_minv, final_maxv)], stream) of a run of frames"""
    s = stream if stream is not None else Stream(gamma)
    res = [s.frame(f) for f in frames]
    return [r[0] for r in res], [r[1] for r in res], s


# ---- test material ---------------------------------------------------------------------------------------------------

def flat_frame(w, h, lo, hi, rng, tiles=8, alpha=None):
    """Flat tiles of a few grey-ish values between lo and hi (inclusive): compressible, and every block has a mean of
    its own.  Alpha is random per tile unless given: the stage must not pass it on."""
    f = np.empty((h, w, 4), np.uint8)
    ty, tx = max(1, h // tiles), max(1, w // tiles)
    for y in range(0, h, ty):
        for x in range(0, w, tx):
            v = int(rng.randint(lo, hi + 1))
            f[y:y + ty, x:x + tx, 0] = v
            f[y:y + ty, x:x + tx, 1] = min(255, v + int(rng.randint(0, 3)))
            f[y:y + ty, x:x + tx, 2] = max(0, v - int(rng.randint(0, 3)))
            f[y:y + ty, x:x + tx, 3] = int(rng.randint(0, 256)) if alpha is None else alpha
    return f


def branch_clip(w, h, seed):
    """Nine frames whose run takes each of the four branches of the recurrence at least once (the range opens, closes,
    opens again), with a frame whose brightest pixel lies left of w*15/100 (it must not count) and one whose brightest
    lies right of w*90/100 inside the last block (it must count)."""
    rng = np.random.RandomState(seed)
    spans = [(70, 170), (30, 230), (90, 150), (100, 140), (20, 250), (60, 200), (110, 130), (40, 220), (80, 160)]
    frames = [flat_frame(w, h, lo, hi, rng) for lo, hi in spans]
    for f, (lo, hi) in zip(frames, spans):                                        # the span is reached inside the blocks
        x = (w * 15) // 100 + 1
        f[1, x, :3] = hi
        f[2:4, x:x + 2, :3] = lo
    frames[2][h // 2, 0, :3] = 255                                                # left of the blocks: not measured
    frames[3][h // 2, last_measured_x(w), :3] = 254                               # right of w*90/100: measured
    return frames


def grey_clip(w, h):
    """Flat grey 128; the same with a brighter and a darker pixel left of the blocks; flat again.  Without gamma minv
    equals maxv in all three, the denominator is 1, the flat frames come out black and the two pixels of the middle
    frame run into the clamp on either side."""
    flat = np.full((h, w, 4), 128, np.uint8)
    flat[:, :, 3] = 7
    mid = flat.copy()
    mid[h // 2, 0, :3] = 129
    mid[h // 2, 1, :3] = 127
    return [flat, mid, flat.copy()]
