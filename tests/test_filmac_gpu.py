"""The device half of the filmac stage (ntscsim_filmac_frames_device / _frames_host, the level state and the levels tap)
against the checker tests/_filmac_ref.py, byte for byte: the stage is integer arithmetic, so the tolerance is zero.
Every byte of every destination buffer is compared -- row padding and the guard bytes around the frame included --, the
sources are checked to be untouched, and minv, maxv, final_minv and final_maxv of every frame are compared through the
tap, so that wrong statistics are told from a wrong recurrence from a wrong map.

A workgroup of the statistics pass owns a 128 x 128 block that starts at width*15/100 and is clipped by the frame
alone; the shapes straddle that: 32x32 is one block that runs past width*90/100, 160x130 has a second row of blocks of
two rows, 345x129 a width that is no multiple of 4 and a last block clipped by the width, 1000x16 a last block that
crosses width*90/100 and ends inside the frame, 900x140 six blocks by two."""
import ctypes as C
import os

import numpy as np
import pytest

import _filmac_ref as R
import _libs as L  # noqa: F401  (puts the package on the path)
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

SIZES = [(32, 32), (160, 130), (345, 129), (1000, 16), (900, 140)]
# tight rows | rows padded to a 16-byte pitch and more | linesize and base only 4-byte aligned
LAYOUTS = ("tight", "padded", "unaligned")
GAMMAS = {"plain": [], "gamma": ["-gamma", "ntsc"]}
KERNELS = ["k_filmac_stats", "k_filmac_frame_levels", "k_filmac_levels", "k_filmac_tables", "k_filmac_apply"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filmac_ref.npz")


def geometry(w, layout):
    """(linesize, offset of the frame in its buffer)"""
    return {"tight": (4 * w, 0), "padded": ((4 * w + 15) // 16 * 16 + 16, 0), "unaligned": (4 * w + 4, 4)}[layout]


def gamma_of(flags):
    return 2.2 if flags else -1.0


@pytest.fixture(scope="module")
def sim():
    s = ntscsim.FieldSimulator(device=0)
    yield s
    s.close()


class Rig:
    def __init__(self, sim, w, h, layout="tight", flags=()):
        import torch
        self.torch = torch
        self.w, self.h, self.geo, self.flags = w, h, geometry(w, layout), list(flags)
        self.ac = ntscsim.AutoContrast(flags=flags, width=w, height=h, sim=sim)
        self.rng = np.random.RandomState(w * 1000 + h)
        self.seed = 9000

    def put(self, content=None):
        """(host buffer, device buffer, device view): a frame inside a padded byte buffer, padding random"""
        self.seed += 1
        ls, off = self.geo
        buf = np.random.RandomState(self.seed).randint(0, 256, size=off + self.h * ls + 16, dtype=np.uint8)
        if content is not None:
            self.view(buf)[...] = content
        t = self.torch.from_numpy(buf).cuda()
        return buf, t, self.torch.as_strided(t, (self.h, self.w, 4), (ls, 4, 1), off)

    def view(self, buf):
        ls, off = self.geo
        return np.lib.stride_tricks.as_strided(buf[off:], shape=(self.h, self.w, 4), strides=(ls, 4, 1))

    def want_buf(self, before, content):
        want = before.copy()
        self.view(want)[...] = content
        return want

    def compare(self, dst, src, outs, levels, what, first=0):
        """dst / src: put() results of the frames of the last call; outs / levels: the checker's"""
        for i in range(len(dst)):
            got = self.ac.levels(first + i)
            for name, g, wnt in zip(("minv", "maxv", "final_minv", "final_maxv"), got, levels[i]):
                assert g == wnt, "%s: %s of frame %d: %d, want %d" % (what, name, i, g, wnt)
            bad = int((dst[i][1].cpu().numpy() != self.want_buf(dst[i][0], outs[i])).sum())
            assert bad == 0, "%s: frame %d: %d bytes differ" % (what, i, bad)
            if src[i] is not dst[i]:
                assert int((src[i][1].cpu().numpy() != src[i][0]).sum()) == 0, "%s: source %d written" % (what, i)

    def check(self, frames, what="", stream=None):
        """All frames through one ntscsim_filmac_frames_device call against the checker (a fresh run unless `stream`)."""
        src = [self.put(f) for f in frames]
        dst = [self.put() for _ in frames]
        self.ac.stretch_frames([(d[2], s[2]) for d, s in zip(dst, src)])
        self.ac.sync()
        assert self.ac.last_kernels() == KERNELS, what
        outs, levels, s = R.run(frames, gamma_of(self.flags), stream)
        self.compare(dst, src, outs, levels, what)
        return outs, levels, s


def noise_frame(rng, w, h, lo=0, hi=256):
    return rng.randint(lo, hi, size=(h, w, 4)).astype(np.uint8)


@pytest.mark.parametrize("gamma", sorted(GAMMAS))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_sizes_layouts_gamma(sim, size, layout, gamma):
    """Three frames in one call: flat tiles, noise in a narrow band (every block mean differs, the stretch is steep and
    runs into both clamps), full-range noise."""
    w, h = size
    rig = Rig(sim, w, h, layout, GAMMAS[gamma])
    frames = [R.flat_frame(w, h, 60, 190, rig.rng), noise_frame(rig.rng, w, h, 90, 150), noise_frame(rig.rng, w, h)]
    frames[1][h // 2, 0, :3] = (0, 255, 128)                                      # outside the blocks: clamped both ways
    rig.check(frames, "%dx%d %s %s" % (w, h, layout, gamma))


def recorded_keys():
    return sorted(k[3:] for k in np.load(GOLDEN).files if k.startswith("io_"))


@pytest.mark.parametrize("key", recorded_keys())
def test_recorded_runs_on_the_device(sim, key):
    """The clips recorded from the reference's own lines (tests/test_filmac_ref.py lists the kinds of frame they keep:
    the first frame, the four branches, minv == maxv, a brightest pixel left of the blocks and one right of
    width*90/100, rows of blocks clipped by the height, results below 0 and beyond the clamp): device output against
    the RECORDED output and levels, field by field."""
    z = np.load(GOLDEN)
    io, lv = z["io_" + key], z["lv_" + key]
    size, tag, _ = key.split("_")
    w, h = (int(v) for v in size.split("x"))
    rig = Rig(sim, w, h, "tight", GAMMAS["gamma" if tag == "g" else "plain"])
    src = [rig.put(f) for f in io[:, 0]]
    dst = [rig.put() for _ in src]
    rig.ac.stretch_frames([(d[2], s[2]) for d, s in zip(dst, src)])
    rig.ac.sync()
    rig.compare(dst, src, io[:, 1], [tuple(int(v) for v in row) for row in lv], key)


def test_pixels_behind_the_last_block_do_not_count(sim):
    """1000 wide: blocks start at 150, 278, ... 790 and the last one ends at 918, inside the frame.  A bright pixel at
    917 (right of 900 = width*90/100) is measured, one at 918 is not, one at 149 is not."""
    w, h = 1000, 16
    assert R.block_origins(w, h)[0][-1] + R.BLOCK == 918 and R.last_measured_x(w) == 917
    for x, counts in ((917, True), (918, False), (149, False), (150, True)):
        rig = Rig(sim, w, h)
        f = R.flat_frame(w, h, 80, 120, rig.rng)
        f[7, x, 1] = 250
        _, levels, s = rig.check([f], "bright pixel at %d" % x)
        assert (levels[0][1] == 250 << 16) == counts, x


def nine(w=160, h=130):
    frames = R.branch_clip(w, h, 4242)
    _, _, s = R.run(frames)
    assert all(v > 0 for v in s.branches.values()), s.branches
    return frames


@pytest.mark.parametrize("gamma", sorted(GAMMAS))
def test_state_carries_from_frame_to_frame_and_from_call_to_call(sim, gamma):
    """Nine frames that take every branch of the recurrence: as one call, as nine calls and as 4 + 5 -- the same bytes,
    the same levels and the same final state, which is the checker's."""
    frames = nine()
    rig = Rig(sim, 160, 130, "padded", GAMMAS[gamma])
    outs, levels, s = R.run(frames, gamma_of(rig.flags))
    assert all(v > 0 for v in s.branches.values()), s.branches
    src = [rig.put(f) for f in frames]
    for split in ([9], [1] * 9, [4, 5]):
        rig.ac.reset()
        assert rig.ac.state[0] is False
        dst = [rig.put() for _ in frames]
        at = 0
        for m in split:
            rig.ac.stretch_frames([(dst[i][2], src[i][2]) for i in range(at, at + m)])
            rig.ac.sync()
            rig.compare(dst[at:at + m], src[at:at + m], outs[at:at + m], levels[at:at + m], "split %r at %d" % (split, at))
            at += m
        assert rig.ac.state == (True, s.fmin, s.fmax), split


def test_reset_set_state_and_get_state(sim):
    rig = Rig(sim, 160, 130)
    frames = nine()
    outs, levels, s = rig.check(frames[:3], "first three")
    mid = rig.ac.state
    assert mid == (True, s.fmin, s.fmax)
    rig.check(frames[3:], "the rest, state kept", stream=s)
    # back to the state after three frames: the rest comes out as before; reset: as a fresh run
    rig.ac.state = mid
    assert rig.ac.state == mid
    s2 = R.Stream()
    s2.init, s2.fmin, s2.fmax = mid
    rig.check(frames[3:], "the rest, state restored", stream=s2)
    rig.ac.reset()
    assert rig.ac.state[0] is False
    rig.check(frames[3:], "after reset")
    # binding again resets as well
    rig2 = Rig(sim, 160, 130)
    assert rig2.ac.state[0] is False
    rig2.check(frames[:2], "after bind")


def test_states_only_set_state_can_produce_do_not_fault(sim):
    """final_maxv == final_minv after the step (flat grey 128 on a state of 128 << 16 twice): the denominator counts as
    1 and the frame comes out black.  final_maxv below final_minv: divided as the tool's signed division does."""
    w, h = 32, 32
    rig = Rig(sim, w, h)
    a = 128 << 16
    grey = R.grey_clip(w, h)[0]
    rig.ac.state = (True, a, a)
    s = R.Stream(strict=False)
    s.init, s.fmin, s.fmax = True, a, a
    outs, levels, _ = rig.check([grey], "zero denominator", stream=s)
    assert levels[0] == (a, a + 1, a, a) and (outs[0][:, :, :3] == 0).all()
    rig.ac.state = (True, 200 << 16, 100 << 16)
    s = R.Stream(strict=False)
    s.init, s.fmin, s.fmax = True, 200 << 16, 100 << 16
    _, levels, _ = rig.check([noise_frame(rig.rng, w, h, 150, 160)], "negative denominator", stream=s)
    assert levels[0][3] < levels[0][2]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_in_place_equals_out_of_place(sim, layout):
    w, h = 345, 129
    rig = Rig(sim, w, h, layout, GAMMAS["gamma"])
    frames = [noise_frame(rig.rng, w, h, 40, 200), R.flat_frame(w, h, 10, 250, rig.rng)]
    outs, levels, _ = R.run(frames, 2.2)
    bufs = [rig.put(f) for f in frames]
    rig.ac.stretch_frames([(b[2], b[2]) for b in bufs])
    rig.ac.sync()
    assert rig.ac.last_kernels() == KERNELS
    rig.compare(bufs, bufs, outs, levels, "in place")


def test_a_later_descriptor_reads_what_an_earlier_one_wrote(sim):
    """b = stretch(a), c = stretch(b) in one call: two launch groups, the second frame of the run is the first's output."""
    w, h = 160, 130
    rig = Rig(sim, w, h)
    f = noise_frame(rig.rng, w, h, 70, 140)
    s = R.Stream()
    once, l1 = s.frame(f)
    twice, l2 = s.frame(once)
    a, b, c = rig.put(f), rig.put(), rig.put()
    rig.ac.stretch_frames([(b[2], a[2]), (c[2], b[2])])
    rig.ac.sync()
    assert rig.ac.last_kernels() == KERNELS * 2
    rig.compare([b, c], [a, a], [once, twice], [l1, l2], "chain")
    assert int((once != twice).sum()) > 0


def test_65539_frames_in_one_call(sim):
    """More frames than one grid takes: the planner splits the call into 65535 + 4.  16 x 16 frames have one block,
    columns 2 .. 15; their levels are computed for all frames at once here, the recurrence is walked in Python, and the
    final state, three sampled frames and their levels are compared."""
    import torch
    n, w, h = 65539, 16, 16
    rng = np.random.RandomState(65539)
    clip = (rng.randint(0, 160, size=(n, 1, 1, 1)) + rng.randint(0, 96, size=(n, h, w, 4))).astype(np.uint8)
    s = R.Stream()
    region = clip[:, :, 2:, :3]
    grd = h * (w - 2)
    minv = np.minimum((s.scale * 6) // 10, (s.lut[region.min(axis=3)].sum(axis=(1, 2)) + grd // 2) // grd)
    maxv = np.maximum((s.scale * 4) // 10, s.lut[region.max(axis=3)].max(axis=(1, 2)))
    maxv = maxv + (minv == maxv)
    samples, want = (0, 40000, n - 1), {}
    for i in range(n):
        s.step(int(minv[i]), int(maxv[i]))
        if i in samples:
            assert R.Stream().frame_levels(clip[i]) == (int(minv[i]), int(maxv[i]))
            want[i] = (s.table(), (int(minv[i]), int(maxv[i]), s.fmin, s.fmax))
    assert all(v > 0 for v in s.branches.values())
    ac = ntscsim.AutoContrast(width=w, height=h, sim=sim)
    src = torch.from_numpy(clip).cuda()
    dst = torch.zeros_like(src)
    ac.stretch_frames([(dst[i], src[i]) for i in range(n)])
    ac.sync()
    assert ac.last_kernels() == KERNELS * 2
    assert ac.state == (True, s.fmin, s.fmax)
    for i in samples:
        table, levels = want[i]
        assert ac.levels(i) == levels, i
        out = np.empty_like(clip[i])
        out[:, :, :3] = table[clip[i][:, :, :3]]
        out[:, :, 3] = 0xFF
        assert int((dst[i].cpu().numpy() != out).sum()) == 0, i


def test_host_frames_equal_the_device_call(sim):
    """ntscsim_filmac_frames_host on padded host frames: the same bytes, levels and state as the device call, and the
    bytes outside 4 * width of a row keep what they held."""
    w, h = 345, 129
    rig = Rig(sim, w, h, "padded", GAMMAS["gamma"])
    frames = [noise_frame(rig.rng, w, h, 30, 220) for _ in range(3)]
    outs, levels, s = rig.check(frames, "device call")
    rig.ac.reset()
    src = [rig.put(f) for f in frames]
    hbuf = [rig.put()[0] for _ in frames]
    before = [b.copy() for b in hbuf]
    rig.ac.stretch_frames_host([(rig.view(b), rig.view(sb[0])) for b, sb in zip(hbuf, src)])
    assert rig.ac.last_kernels() == KERNELS
    for i in range(3):
        assert int((hbuf[i] != rig.want_buf(before[i], outs[i])).sum()) == 0, "host call, frame %d" % i
        assert rig.ac.levels(i) == levels[i]
        assert int((rig.view(src[i][0]) != frames[i]).sum()) == 0
    assert rig.ac.state == (True, s.fmin, s.fmax)
    # in place on the host, and a chain through host memory
    rig.ac.reset()
    a = frames[0].copy()
    rig.ac.stretch_frames_host([(a, a)])
    assert int((a != outs[0]).sum()) == 0


def test_kernel_times_tap(sim):
    rig = Rig(sim, 160, 130)
    f = noise_frame(rig.rng, 160, 130)
    with pytest.raises(ntscsim.NtscsimError) as e:
        rig.ac.kernel_ms()                                                         # nothing timed
    assert e.value.code == _capi.E_ARG
    rig.ac.debug_time_kernels(True)
    outs, _, s = rig.check([f, f], "timed")                                        # the same bytes while timed
    ms = rig.ac.kernel_ms()
    assert len(ms) == 5 and all(0 < t < 1000 for t in ms), ms
    rig.ac.debug_time_kernels(False)
    with pytest.raises(ntscsim.NtscsimError):
        rig.ac.kernel_ms()


def test_error_codes():
    import torch
    fs = ntscsim.FieldSimulator(device=0)
    try:
        lib = fs._lib
        d = _capi.FilmacDesc()
        st = _capi.FilmacState()
        lv = (C.c_int64 * 4)()
        assert lib.ntscsim_filmac_frames_device(fs._h, C.byref(d), 1, None) == _capi.E_ARG     # no bind
        assert lib.ntscsim_filmac_frames_host(fs._h, C.byref(d), 1) == _capi.E_ARG
        assert lib.ntscsim_filmac_reset(fs._h) == _capi.E_ARG
        assert lib.ntscsim_filmac_get_state(fs._h, C.byref(st)) == _capi.E_ARG
        assert lib.ntscsim_filmac_debug_levels(fs._h, 0, lv) == _capi.E_ARG
        for wh in ((15, 16), (16, 15), (16385, 16), (16, 16385), (-1, -1)):
            with pytest.raises(ntscsim.NtscsimError) as e:
                ntscsim.AutoContrast(width=wh[0], height=wh[1], sim=fs)
            assert e.value.code == _capi.E_SIZE, wh
        ntscsim.AutoContrast(width=16384, height=16, sim=fs)
        ac = ntscsim.AutoContrast(width=96, height=32, sim=fs)
        a = torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda")
        b = torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda")

        def code(jobs):
            with pytest.raises(ntscsim.NtscsimError) as e:
                ac.stretch_frames(jobs)
            return e.value.code

        small = torch.zeros((32, 64, 4), dtype=torch.uint8, device="cuda")
        assert code([(small, small.clone())]) == _capi.E_SIZE                      # not the bound size (the binding checks: a descriptor carries none)
        wide = torch.zeros((33, 97, 4), dtype=torch.uint8, device="cuda")
        odd = torch.as_strided(wide, (32, 96, 4), (386, 4, 1), 0)
        assert code([(odd, b)]) == _capi.E_SIZE and code([(a, odd)]) == _capi.E_SIZE   # linesize not a multiple of 4
        narrow = torch.as_strided(wide, (32, 96, 4), (380, 4, 1), 0)
        assert code([(narrow, b)]) == _capi.E_SIZE                                 # linesize below 4 * width
        off2 = torch.as_strided(wide, (32, 96, 4), (388, 4, 1), 2)
        assert code([(off2, b)]) == _capi.E_SIZE and code([(a, off2)]) == _capi.E_SIZE   # pointer not a multiple of 4
        big = torch.zeros((40, 96, 4), dtype=torch.uint8, device="cuda")
        assert code([(big[:32], big[8:])]) == _capi.E_ARG                          # overlapping by some rows
        same_rows = torch.zeros((32 * 768,), dtype=torch.uint8, device="cuda")
        x = torch.as_strided(same_rows, (32, 96, 4), (768, 4, 1), 0)
        y = torch.as_strided(same_rows, (32, 96, 4), (384, 4, 1), 0)
        assert code([(x, y)]) == _capi.E_ARG                                       # same pointer, another linesize: not in place
        assert code([(b, a), (big[:32], big[8:])]) == _capi.E_ARG                  # checked before anything is launched
        assert ac.state[0] is False
        dd = (_capi.FilmacDesc * 1)()
        dd[0].dst, dd[0].dst_linesize, dd[0].src_linesize = a.data_ptr(), 384, 384
        assert lib.ntscsim_filmac_frames_device(fs._h, dd, 1, None) == _capi.E_ARG   # NULL source
        assert lib.ntscsim_filmac_frames_device(fs._h, None, 1, None) == _capi.E_ARG
        assert lib.ntscsim_filmac_frames_device(fs._h, dd, -1, None) == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            ac.levels(0)                                                           # no call yet
        assert e.value.code == _capi.E_ARG
        ac.stretch_frames([])
        ac.stretch_frames([(a, b)])
        ac.sync()
        ac.levels(0)
        with pytest.raises(ntscsim.NtscsimError) as e:
            ac.levels(1)                                                           # outside the last call
        assert e.value.code == _capi.E_ARG
        for bad in ((True, (1 << 32) + 1, 0), (True, 0, -(1 << 32) - 1)):
            with pytest.raises(ntscsim.NtscsimError) as e:
                ac.state = bad
            assert e.value.code == _capi.E_PARAM
        ac.state = (True, -(1 << 32), 1 << 32)
        assert ac.state == (True, -(1 << 32), 1 << 32)
    finally:
        fs.close()
