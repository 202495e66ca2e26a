"""The verification step the stage benchmarks share (tools/bench_key.py, bench_avg.py, bench_blend.py, bench_scan.py,
bench_led.py): the bytes a benchmark has timed are compared with the stage's checker (tests/_*_ref.py) before that
case's numbers are printed.  It runs once per case, outside the timed region, on what the timed calls themselves left
in the output buffers; it is on by default and is switched off with --no-verify.

Non-recurrent stages (blend, scan, led): output frames 0, 1, the middle one and the last.  Clip stages (key, avg): a
run starts from the ring the run before it left, so the tool zeroes the ring in front of its last timed run, outside that
run's events, and that run's output is compared: the first 2 * delay + 3 output frames, and what does not depend on the
ring: the ring index and the position or field number behind the clip.  Where the checker's pace over that prefix puts
the whole clip under about 20 s the whole clip is compared, and the ring behind it.  A case's entry gains
`frames_verified` and `verify_s`; a mismatch ends the tool with a non-zero status."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))          # the checkers

WHOLE_CLIP_S = 20.0
M32 = 0xFFFFFFFF


def add_argument(ap):
    ap.add_argument("--no-verify", action="store_true", help="do not compare the timed output with the checker")


def mismatch(what):
    sys.exit("bench verification FAILED: " + what)


def same(want, got, what):
    bad = int((np.asarray(want) != np.asarray(got)).sum())
    if bad:
        mismatch("%s: %d bytes differ" % (what, bad))


def sample_frames(n):
    return sorted(set(k for k in (0, 1, n // 2, n - 1) if 0 <= k < n))


def verify_frames(n, want, got, what):
    """want(k), got(k): output frame k by the checker and as timed.  Returns the keys for the case's entry."""
    t0 = time.time()
    idx = sample_frames(n)
    for k in idx:
        same(want(k), got(k), "%s, output frame %d" % (what, k))
    return {"frames_verified": idx, "verify_s": time.time() - t0}


def verify_clip(T, delay, shape, step, got, got_ring, what):
    """step(dst, t): the checker's frame t onto ring frame dst (numpy, in place); got(t): output frame t of the device
    run from a zeroed ring; got_ring(i): ring frame i behind it.  Returns the keys for the case's entry."""
    t0 = time.time()
    ring = [np.zeros(shape, np.uint8) for _ in range(delay)]
    prefix = min(T, 2 * delay + 3)
    done = []
    for t in range(T):
        if t == prefix and (time.time() - t0) / prefix * T > WHOLE_CLIP_S:
            break
        step(ring[t % delay], t)
        same(ring[t % delay], got(t), "%s, output frame %d" % (what, t))
        done.append(t)
    if len(done) == T:
        for i in range(delay):
            same(ring[i], got_ring(i), "%s, ring frame %d behind the clip" % (what, i))
    return {"frames_verified": done, "verify_s": time.time() - t0}


def _mulmod(a, b):
    """a * b modulo x^31 - x^28 - 1, coefficients modulo 2^32"""
    prod = [0] * 61
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                prod[i + j] += x * y
    for k in range(60, 30, -1):                          # x^k = x^(k - 3) + x^(k - 31)
        c = prod[k]
        prod[k - 3] += c
        prod[k - 31] += c
    return [p & M32 for p in prod[:31]]


def _xpow(n):
    r, b = [1] + [0] * 30, [0, 1] + [0] * 29
    while n:
        if n & 1:
            r = _mulmod(r, b)
        b = _mulmod(b, b)
        n >>= 1
    return r


def block_rand(base, maxlog=22, slack=1 << 24):
    """tests/_key_ref.py's rand() stream held as a uint32 array and extended a block at a time: a noisy 1920 x 1080
    frame takes 6.2 million draws, too many for the checker's own list of Python integers.  s[i] = s[i-31] + s[i-3]
    means x^31 = x^28 + 1, so x^N = sum c[j] x^j (j < 31) gives s[n] = sum c[j] s[n - N + j]: N - 30 new words from 31
    array products.  The first words and their meaning are the checker's (`base` is its GlibcRand).

    Only a stretch of the stream is held: the checker walks a clip forwards, so words more than `slack` behind the ones
    asked for are dropped, except the 2^maxlog + 31 last ones the next block is made from.  With the defaults that is
    the words of one request (3 * W * H: 25 MB at 1920 x 1080) and at most 2 * slack + 2^maxlog more, about 150 MB,
    whatever the position.  A request behind the held stretch starts again from the first words.

    Measured: the 19 frames of a noisy 1920 x 1080, delay 8 prefix (118 million draws) take 3.2 s of stream on the build
    machine's CPU with the process at 186 MB; tools/bench_key.py --sizes 1920x1080 --frames 24 on the MI355X host
    verified all 24 frames of that case in 2.9 s (0.12 s per frame, the checker included: a 600-frame clip stays with
    its prefix), the process peaking at 2.3 GB resident with torch and the HIP runtime loaded."""
    keep = (1 << maxlog) + 31

    class BlockRand(base):
        def __init__(self):
            self.a = None
            super().__init__()                           # the checker's own first 344 words
            self.first = np.array(self.s[:344], dtype=np.uint64).astype(np.uint32)
            self.coef = {}
            self._restart()

        def _restart(self):
            self.a = self.first.copy()
            self.at = 0                                  # self.a[:self.have] is s[self.at : self.at + self.have]
            self.have = len(self.a)

        def _fill(self, n):
            """s up to self.at + n"""
            if n > len(self.a):
                grown = np.empty(max(n, 2 * len(self.a)), np.uint32)
                grown[:self.have] = self.a[:self.have]
                self.a = grown
            while self.have < n:
                have = self.have
                N = 1 << min(maxlog, have.bit_length() - 1)
                if N not in self.coef:
                    self.coef[N] = _xpow(N)
                B = min(N - 30, n - have)
                new = self.a[have:have + B]
                new[...] = 0
                for j, c in enumerate(self.coef[N]):
                    if c:
                        new += np.uint32(c) * self.a[have - N + j:have - N + j + B]
                self.have = have + B

        def _span(self, lo, hi):
            """s[lo:hi], a view"""
            if lo < self.at:
                self._restart()
            while True:
                end = self.at + self.have
                drop = min(lo, end - keep) - self.at
                if drop > slack:
                    self.a = self.a[drop:self.have].copy()
                    self.at += drop
                    self.have -= drop
                if end >= hi:
                    break
                self._fill(min(hi, end + slack) - self.at)
            return self.a[lo - self.at:hi - self.at]

        def _extend(self, n):
            if self.a is None:
                return super()._extend(n)
            self._span(max(self.at, n - 1), n)

        def draws(self, pos, n):
            return self._span(344 + pos, 344 + pos + n) >> np.uint32(1)

        def window(self, pos):
            return [int(x) for x in self._span(313 + pos, 344 + pos)]

    fast, slow = BlockRand(), base()
    for pos, n in ((0, 3000), (70000, 64)):
        assert fast.draws(pos, n).tolist() == slow.draws(pos, n).tolist()
    assert fast.window(70000) == slow.window(70000)
    return fast
