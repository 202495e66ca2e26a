"""Checker of the frameblend stage: a NumPy / pure-Python restatement of what frameblend.cpp computes, written from
its semantics (frame time :100-110, the weight planner :929-1028 with the erase of :1107-1120, the gamma tables
:724-732, the pixel loops :1032-1081).  It is pinned by tests/golden/frameblend_golden.npz, which
tests/golden/make_golden_frameblend.py produced from the reference's own lines (test_blend_plan.py)."""
import math

import numpy as np


def frame_time(pts, tb_num, tb_den, rate_num, rate_den):
    """:100-110 -- the double pts times one integer product, then divided by the other: two roundings."""
    n = float(pts)
    n *= float(int(tb_num) * int(rate_num))
    n /= float(int(tb_den) * int(rate_den))
    return n


def clip_periods(last_t):
    """Output periods rendered for a clip whose last frame has time last_t (:924-927)."""
    return max(0, int(math.ceil(last_t))) + 1


def tables(gamma):
    """:724-732 -- truncating conversions of libm pow()."""
    dec = np.array([int(math.pow(i / 255.0, gamma) * 8192) for i in range(256)], dtype=np.uint16)
    enc = np.array([int(math.pow(i / 8192.0, 1.0 / gamma) * 255) for i in range(8193)], dtype=np.uint8)
    return dec, enc


class Planner:
    """The tool's two vectors and the per-period scan.  ids returned by next() are stable (counted from the start of
    the clip); internally the list is renumbered by the erase exactly as the tool's vectors are."""

    def __init__(self, sqnr=False, ffa=False, fa=1):
        self.sqnr, self.ffa, self.fa = bool(sqnr), bool(ffa), int(fa)
        self.t = []
        self.base = 0
        self.erases = 0

    def push(self, t):
        self.t.append(float(t))
        return self.base + len(self.t) - 1

    def next(self, current):
        t, fa = self.t, self.fa
        n = len(t)
        weights = []
        cutoff = 0
        if n > 1:
            if fa > 1:
                span = fa if self.ffa else 1
                i = current % fa
                while i + fa < n:
                    bt, et = t[i], t[i + fa]
                    if i != 0 and (et + 2.0) < current:
                        cutoff = i - (i % fa)
                    bt = min(max(bt, float(current)), float(current + span))
                    et = min(max(et, float(current)), float(current + span))
                    if bt < et:
                        weights.append([i, (et - bt) / span])
                    i += fa
            else:
                for i in range(n - 1):
                    bt, et = t[i], t[i + 1]
                    if i != 0 and (et + 2.0) < current:
                        cutoff = i
                    bt = min(max(bt, float(current)), float(current + 1))
                    et = min(max(et, float(current)), float(current + 1))
                    if bt < et:
                        weights.append([i, et - bt])
        if not weights and n > cutoff:
            weights.append([cutoff, 1.0])
        if self.sqnr and len(weights) in (2, 3):
            sq = abs((t[weights[1][0]] - t[weights[0][0]]) - 1.0) / 0.01
            if sq < 1.0:
                sq = math.pow(sq, 2.0)
                if sq > 0.01:
                    if weights[0][1] > sq:
                        weights[0][1] = sq
                    weights[0][1] /= sq
                    weights[1][1] = 1.0 - weights[0][1]
                else:
                    weights[0][1] = 1.0
                    weights[1][1] = 0.0
                if len(weights) > 2:
                    weights[2][1] = 0.0
        ids = [self.base + i for i, _ in weights]
        w16 = [int(math.floor(w * 0x10000 + 0.5)) & 0xFFFFFFFF for _, w in weights]
        if cutoff >= 32:
            del t[:cutoff]
            self.base += cutoff
            self.erases += 1
        return ids, w16


def plan_clip(times, sqnr=False, ffa=False, fa=1, last=None):
    """Whole clip with the tool's read-ahead (:910): [(ids, weight16)] for periods 0 .. last - 1."""
    times = [float(x) for x in times]
    if last is None:
        last = clip_periods(times[-1])
    pl = Planner(sqnr, ffa, fa)
    pl.push(times[0])
    pushed = 1
    out = []
    for current in range(last):
        while pushed < len(times) and times[pushed - 1] < current + 30:
            pl.push(times[pushed])
            pushed += 1
        out.append(pl.next(current))
    return out


def blend_pixels(srcs, w16, gamma=None):
    """:1032-1081 -- srcs: list of uint8 [H, W, 4] BGRA, w16: their weights; gamma: None or a value <= 1 = the plain
    path, otherwise the table path.  Returns uint8 [H, W, 4], alpha 0xFF.  No taps: black."""
    h, w = srcs[0].shape[:2] if srcs else (0, 0)
    use_gamma = gamma is not None and gamma > 1
    if use_gamma:
        dec, enc = tables(gamma)
    # 64-bit sums, as the tool's: exact for every weight list the library accepts (sum(weight16) < 2^38)
    assert sum(int(x) for x in w16) < (1 << 38)
    acc = np.zeros((h, w, 3), dtype=np.uint64)
    for s, wt in zip(srcs, w16):
        v = s[:, :, :3]
        acc += (dec[v].astype(np.uint64) if use_gamma else v.astype(np.uint64)) * np.uint64(int(wt))
    idx = acc >> np.uint64(16)
    out = np.empty((h, w, 4), dtype=np.uint8)
    if use_gamma:
        out[:, :, :3] = enc[np.minimum(idx, 8192).astype(np.int64)]
    else:
        out[:, :, :3] = np.minimum(idx, 255).astype(np.uint8)
    out[:, :, 3] = 0xFF
    return out


def blend_frame(shape, srcs, w16, gamma=None):
    """blend_pixels for a frame of `shape` = (H, W): an empty tap list gives black with alpha 0xFF."""
    if not srcs:
        out = np.zeros((shape[0], shape[1], 4), dtype=np.uint8)
        out[:, :, 3] = 0xFF
        return out
    return blend_pixels(srcs, w16, gamma)


def noise_frame(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 4), dtype=np.uint8)
