"""The device half of the vhsled stage (ntscsim_led_frames_device / _frames_host, the edges tap and the hand-off from
the field simulator) against the checker tests/_led_ref.py, byte for byte: the stage is 32-bit integer arithmetic, so
the tolerance is zero.  Every byte of every destination buffer is compared -- row padding and the guard bytes around
the frame included --, the sources are checked to be untouched, and e[y] and x[y] of every row are compared through the
debug tap, so that a wrong scan is told from a wrong copy.

A workgroup owns a band of 16 rows and a wave looks at 64 pixels per load, 128 before its first wait: the shapes
straddle those numbers (263 wide lies behind the probe and behind the first group of the walk; 40 rows are two bands
and a half)."""
import ctypes as C

import numpy as np
import pytest

import _led_ref as R
import _libs as L
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (64, 16), (65, 17), (72, 16), (130, 21), (263, 24), (100, 40)]
# (destination, source): rows and base 16-byte aligned (the vector path) | linesize and base only 4-byte aligned (dwords)
LAYOUTS = {"aligned": ("v", "v"), "unaligned": ("d", "d"), "mixed": ("v", "d")}


def geometry(w, kind):
    return ((4 * w + 15) // 16 * 16 + 16, 0) if kind == "v" else (4 * w + 4, 4)


def host_frame(w, h, ls, off, frame=None, seed=0):
    """A frame inside a padded byte buffer: rows of `ls` bytes starting `off` bytes in; padding random."""
    buf = np.random.RandomState(seed).randint(0, 256, size=off + h * ls + 16, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w, 4), strides=(ls, 4, 1))
    if frame is not None:
        view[...] = frame
    return buf, view


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


class Rig:
    def __init__(self, sim, w, h, layout):
        import torch
        self.torch = torch
        self.w, self.h = w, h
        self.dgeo, self.sgeo = geometry(w, LAYOUTS[layout][0]), geometry(w, LAYOUTS[layout][1])
        self.led = ntscsim.EdgeAligner(width=w, height=h, sim=sim)
        self.led.debug_keep_edges(True)
        self.rng = np.random.RandomState(w * 1000 + h)
        self.seed = 5000

    def put(self, geo, content=None):
        """(host buffer, host view, device buffer, device view)"""
        self.seed += 1
        ls, off = geo
        buf, view = host_frame(self.w, self.h, ls, off, content, self.seed)
        t = self.torch.from_numpy(buf).cuda()
        return buf, view, t, self.torch.as_strided(t, (self.h, self.w, 4), (ls, 4, 1), off)

    def want_buf(self, f, geo, content):
        want = f[0].copy()
        np.lib.stride_tricks.as_strided(want[geo[1]:], shape=(self.h, self.w, 4), strides=(geo[0], 4, 1))[...] = content
        return want

    def check(self, frames, what="", kernels=("k_led_frames",)):
        """All frames through one ntscsim_led_frames_device call against the checker; returns [(out, e, x)]."""
        src = [self.put(self.sgeo, f) for f in frames]
        dst = [self.put(self.dgeo) for _ in frames]
        self.led.align_frames([(d[3], s[3]) for d, s in zip(dst, src)])
        self.led.sync()
        assert self.led.last_kernels() == list(kernels), what
        res = []
        for i, f in enumerate(frames):
            want, e, x = R.align_frame(f)
            ge, gx = self.led.edges(i)
            assert (ge == e).all(), "%s: e of frame %d: rows %r" % (what, i, np.nonzero(ge != e)[0][:8])
            assert (gx == x).all(), "%s: x of frame %d: rows %r" % (what, i, np.nonzero(gx != x)[0][:8])
            bad = int((dst[i][2].cpu().numpy() != self.want_buf(dst[i], self.dgeo, want)).sum())
            assert bad == 0, "%s: frame %d: %d bytes differ" % (what, i, bad)
            assert int((src[i][2].cpu().numpy() != src[i][0]).sum()) == 0, "%s: source %d written" % (what, i)
            res.append((want, e, x))
        return res

    def frames_of_rows(self, rows):
        """rows -> frames of h rows each; the last one is filled up with dark rows"""
        rows = list(rows)
        while len(rows) % self.h:
            rows.append(R.dark_row(self.rng, self.w))
        return [np.stack(rows[i:i + self.h]) for i in range(0, len(rows), self.h)]


@pytest.fixture(params=[(w, h, lay) for (w, h) in SIZES for lay in sorted(LAYOUTS)], ids=lambda p: "%dx%d-%s" % p)
def rig(request, sim):
    return Rig(sim, *request.param)


def test_edge_at_every_position(rig):
    """e = 0 .. w - 9, one per row: the runs that start at 56 .. 63 cross a chunk boundary, the one at w - 9 ends with
    the row; a run of eight that ends the row is not one."""
    w = rig.w
    rows = [R.row_with_edge(rig.rng, w, e) for e in range(0, w - 8)]
    eight = R.dark_row(rig.rng, w)
    eight[w - 8:] = R.bright(rig.rng, 8, int(eight[0, 0]))
    rows.append(eight)
    frames = rig.frames_of_rows(rows)
    res = rig.check(frames, "every position")
    e = np.concatenate([r[1] for r in res])
    assert (e[:w - 8] == np.arange(w - 8)).all() and e[w - 8] == w


def test_run_of_eight_then_a_blackish_pixel_then_nine(rig):
    """Eight bright pixels at a, a blackish one, nine bright ones: the edge is a + 9, for every a that fits (in 16
    pixels none does: there the eight stand alone and the row has no edge)."""
    w = rig.w
    starts = list(range(1, w - 17))
    rows = []
    for a in starts:
        row = R.dark_row(rig.rng, w)
        b = int(row[0, 0])
        row[a:a + 8] = R.bright(rig.rng, 8, b)
        row[a + 9:a + 18] = R.bright(rig.rng, 9, b)
        rows.append(row)
    alone = R.dark_row(rig.rng, w)
    alone[1:9] = R.bright(rig.rng, 8, int(alone[0, 0]))
    rows.append(alone)
    res = rig.check(rig.frames_of_rows(rows), "8 + 1 + 9")
    e = np.concatenate([r[1] for r in res])
    assert list(e[:len(starts)]) == [a + 9 for a in starts] and e[len(starts)] == w


def test_threshold_and_channels(rig):
    """Differences of 15 and 16 and negative ones, per channel, against the first pixel's BLUE; a first pixel with high
    green / red and blue 0 is not blackish itself; a first pixel with blue 255 makes the whole row blackish."""
    w, h = rig.w, rig.h
    f = np.zeros((h, w, 4), np.uint8)
    f[:, :, 3] = rig.rng.randint(0, 256, size=(h, w))
    want_e = []
    for y in range(h):
        b = 40 + y
        at = 2 + (y % (w - 11))
        f[y, :, :3] = b + 15                                                      # 15 in every channel: blackish
        f[y, 0, 0] = b
        f[y, 1, :3] = (0, 3, b - 30)                                              # negative differences: blackish
        ch = y % 3
        kind = (y // 3) % 4
        if kind == 0:
            f[y, at:at + 9, ch] = b + 16                                          # 16 in one channel alone (blue, green or red)
            want_e.append(at)
        elif kind == 1:
            f[y, at:at + 9, ch] = 255
            f[y, at + 4, ch] = b + 15                                             # the run is cut: 4 + 4
            want_e.append(w)
        elif kind == 2:
            f[y, 0] = (0, 200, 0, 7) if ch else (0, 0, 200, 7)                    # blue 0, high green or red
            f[y, 1:, :3] = 16
            f[y, 1, :3] = 15
            want_e.append(2 if w >= 11 else w)
        else:
            f[y] = rig.rng.randint(0, 256, size=(w, 4))
            f[y, 0, 0] = 255                                                      # nothing exceeds 255 by 16
            want_e.append(w)
    res = rig.check([f], "threshold")
    assert list(res[0][1]) == want_e
    g = f.copy()                                                                  # first pixel not blackish against its own blue: e = 0
    g[:, :, :3] = 90
    g[:, :, 1] = 120
    g[:, 0, 0] = 100
    res = rig.check([g], "pixel 0 by green alone")
    assert (res[0][1] == 0).all()


def test_smoothing(rig):
    """Nine-row sums of every residue modulo 9; rows 0 .. 3 and h - 4 .. h - 1 keep their own edge; x = w / 2 - 1 moves
    and x = w / 2 does not; one row without an edge among rows with a small one."""
    w, h = rig.w, rig.h
    hi = min(w - 8, 40)
    frames = [R.frame_with_edges(rig.rng, w, rig.rng.randint(0, hi, size=h)) for _ in range(5)]
    es = rig.rng.randint(0, min(6, hi), size=h)
    es[h // 2] = w
    frames.append(R.frame_with_edges(rig.rng, w, es))
    half = w // 2
    frames.append(R.frame_with_edges(rig.rng, w, [half - 1] * h))
    if half + 9 <= w:
        frames.append(R.frame_with_edges(rig.rng, w, [half] * h))
    else:                                                                         # w = 16: (8 * 7 + 16 + 5 / 65536) / 9 = 8
        es = [half - 1] * h
        es[h // 2] = w
        frames.append(R.frame_with_edges(rig.rng, w, es))
    res = rig.check(frames, "smoothing")
    residues, xs = set(), np.concatenate([r[2] for r in res])
    for _, e, x in res:
        assert (x[:4] == e[:4]).all() and (x[-4:] == e[-4:]).all()
        for y in range(4, h - 4):
            residues.add((sum(int(v) << 16 for v in e[y - 4:y + 5]) + 5) % 9)
    assert residues == set(range(9))
    assert (xs == half - 1).any() and (xs == half).any()
    want, e, x = res[-2]
    assert (want[:, :w - (half - 1)] == frames[-2][:, half - 1:]).all()           # moved, top bytes with the pixels
    assert int((want[:, :, 3] != frames[-2][:, :, 3]).sum()) > 0
    want, e, x = res[-1]
    rows = x == half
    assert (want[rows] == frames[-1][rows]).all()                                 # not moved
    assert (res[5][1] == w).sum() == 1 and (res[5][2] < w // 2).all()


def test_all_dark_frame_comes_out_as_it_went_in(rig):
    f = np.stack([R.dark_row(rig.rng, rig.w) for _ in range(rig.h)])
    res = rig.check([f], "all dark")
    assert (res[0][1] == rig.w).all() and (res[0][0] == f).all()


def test_five_frames_in_one_call_and_order(rig):
    frames = [R.capture_frame(rig.rng, rig.w, rig.h) for _ in range(4)] + [np.stack([R.dark_row(rig.rng, rig.w) for _ in range(rig.h)])]
    rig.check(frames, "five frames")
    # b = aligned(a), c = aligned(b) in one call: the second descriptor reads what the first wrote
    a, b, c = rig.put(rig.sgeo, frames[0]), rig.put(rig.dgeo), rig.put(rig.dgeo)
    rig.led.align_frames([(b[3], a[3]), (c[3], b[3])])
    rig.led.sync()
    assert rig.led.last_kernels() == ["k_led_frames"] * 2
    once = R.align_frame(frames[0])[0]
    twice = R.align_frame(once)[0]
    assert int((c[2].cpu().numpy() != rig.want_buf(c, rig.dgeo, twice)).sum()) == 0
    assert int((b[2].cpu().numpy() != rig.want_buf(b, rig.dgeo, once)).sum()) == 0


def test_host_frames_equal_device_call(rig):
    frames = [R.capture_frame(rig.rng, rig.w, rig.h) for _ in range(3)]
    src = [rig.put(rig.sgeo, f) for f in frames]
    dst = [rig.put(rig.dgeo) for _ in frames]
    rig.led.align_frames([(d[3], s[3]) for d, s in zip(dst, src)])
    rig.led.sync()
    hbuf = [d[0].copy() for d in dst]
    hview = [np.lib.stride_tricks.as_strided(bf[rig.dgeo[1]:], shape=(rig.h, rig.w, 4), strides=(rig.dgeo[0], 4, 1)) for bf in hbuf]
    rig.led.align_frames_host([(hv, s[1]) for hv, s in zip(hview, src)])
    for i in range(3):
        assert int((dst[i][2].cpu().numpy() != hbuf[i]).sum()) == 0, "host call, frame %d" % i
        assert int((hview[i] != R.align_frame(frames[i])[0]).sum()) == 0
        assert int((src[i][1] != frames[i]).sum()) == 0


def test_host_call_whose_descriptors_depend_on_each_other(sim):
    """b = aligned(a), c = aligned(b), d = aligned(c) in one ntscsim_led_frames_host call on host arrays: every
    descriptor reads what the one before it wrote, so each is a batch of its own and a launch of its own."""
    w, h = 96, 32
    led = ntscsim.EdgeAligner(width=w, height=h, sim=sim)
    frame = R.capture_frame(np.random.RandomState(9632), w, h)
    a = frame.copy()
    b, c, d = (np.full((h, w, 4), fill, np.uint8) for fill in (0x11, 0x22, 0x33))
    led.align_frames_host([(b, a), (c, b), (d, c)])
    assert led.last_kernels() == ["k_led_frames"] * 3
    want = frame
    for i, got in enumerate((b, c, d)):
        before, want = want, R.align_frame(want)[0]
        assert int((want != before).sum()) > 0                                    # every pass moves rows: the order shows
        assert int((got != want).sum()) == 0, "the checker applied %d times" % (i + 1)
    assert int((a != frame).sum()) == 0


def test_simulator_output_is_aligned_without_leaving_the_device():
    """A few -vhs fields from ntscsim_fields_device stay in device memory and are the sources of the stage: the result
    is the checker applied to the simulator's downloaded output."""
    import torch
    w, h, n = 96, 32, 4
    p = L.make_params(["-vhs"])
    fs = ntscsim.FieldSimulator(params=p, device=0)
    try:
        led = ntscsim.EdgeAligner(width=w, height=h, sim=fs)
        frames = np.stack([L.noise_frame(w, h, 0x71 + i) for i in range(n // 2)])
        frames[:, :, :20, :3] //= 16                                              # a dark left border in the source picture
        jobs = [(k // 2, k, (k & 1) ^ 1, k) for k in range(n)]
        src = torch.from_numpy(frames).cuda()
        fields = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
        fs.fields(src, fields, jobs)
        out = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
        led.align_frames([(out[t], fields[t]) for t in range(n)])
        led.sync()
        assert led.last_kernels() == ["k_led_frames"]
        sim_out = fields.cpu().numpy()
        want = np.stack([R.align_frame(sim_out[t])[0] for t in range(n)])
        assert int((out.cpu().numpy() != want).sum()) == 0
    finally:
        fs.close()


def test_error_codes():
    import torch
    fs = ntscsim.FieldSimulator(device=0)
    try:
        lib = fs._lib
        d = _capi.LedDesc()
        assert lib.ntscsim_led_frames_device(fs._h, C.byref(d), 1, None) == _capi.E_ARG      # no bind
        assert lib.ntscsim_led_frames_host(fs._h, C.byref(d), 1) == _capi.E_ARG
        assert lib.ntscsim_led_debug_keep_edges(fs._h, 1) == _capi.E_ARG
        for wh in ((15, 16), (16, 15), (3641, 16), (16, 65537), (-1, -1)):
            with pytest.raises(ntscsim.NtscsimError) as e:
                ntscsim.EdgeAligner(width=wh[0], height=wh[1], sim=fs)
            assert e.value.code == _capi.E_SIZE, wh
        ntscsim.EdgeAligner(width=3640, height=16, sim=fs)
        led = ntscsim.EdgeAligner(width=96, height=32, sim=fs)
        a = torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda")
        b = torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda")
        small = torch.zeros((32, 64, 4), dtype=torch.uint8, device="cuda")

        def code(jobs):
            with pytest.raises(ntscsim.NtscsimError) as e:
                led.align_frames(jobs)
            return e.value.code

        assert code([(small, small.clone())]) == _capi.E_SIZE                      # not the bound size
        wide = torch.zeros((32, 97, 4), dtype=torch.uint8, device="cuda")
        odd = torch.as_strided(wide, (32, 96, 4), (386, 4, 1), 0)
        assert code([(odd, b)]) == _capi.E_SIZE and code([(a, odd)]) == _capi.E_SIZE   # linesize not a multiple of 4
        narrow = torch.as_strided(wide, (32, 96, 4), (380, 4, 1), 0)
        assert code([(narrow, b)]) == _capi.E_SIZE                                 # linesize below 4 * width
        assert code([(a, a)]) == _capi.E_ARG                                       # in place
        big = torch.zeros((40, 96, 4), dtype=torch.uint8, device="cuda")
        assert code([(big[:32], big[8:])]) == _capi.E_ARG                          # overlapping by some rows
        assert code([(b, a), (a, a)]) == _capi.E_ARG                               # checked before anything is launched
        dd = (_capi.LedDesc * 1)()
        dd[0].dst_dev, dd[0].dst_linesize, dd[0].src_linesize, dd[0].width, dd[0].height = a.data_ptr(), 384, 384, 96, 32
        assert lib.ntscsim_led_frames_device(fs._h, dd, 1, None) == _capi.E_ARG    # NULL source
        assert lib.ntscsim_led_frames_device(fs._h, None, 1, None) == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            led.edges(0)                                                           # nothing kept
        assert e.value.code == _capi.E_ARG
        led.align_frames([])
        led.debug_keep_edges(True)
        led.align_frames([(a, b)])
        led.sync()
        led.edges(0)
        with pytest.raises(ntscsim.NtscsimError) as e:
            led.edges(1)                                                           # outside the last call
        assert e.value.code == _capi.E_ARG
    finally:
        fs.close()
