"""The device half of the average_delay stage (ntscsim_avg_frames_device / _clip_device / _frames_host and the hand-off
from the field simulator) against the checker tests/_avg_ref.py, byte for byte: the stage is 32-bit integer
arithmetic, so the tolerance is zero.  Every byte of every destination buffer is compared -- row padding and the
guard bytes around the frame included -- and the sources are checked to be untouched."""
import ctypes as C

import numpy as np
import pytest

import _avg_ref as R
import _libs as L
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

SIZES = [(96, 32), (100, 35), (99, 33)]
# rows 16-byte aligned (the vector path) | linesize and base pointer only 4-byte aligned (the dword path)
LAYOUTS = {"aligned": (0, 0), "unaligned": (4, 4)}
LEVELS = [0, 1, 128, 255, 256]
WRAPPING = [257, 1000, -1, 65536]


def geometry(w, layout):
    extra, off = LAYOUTS[layout]
    return 4 * w + extra + (16 if layout == "aligned" else 0), off          # padded rows in both layouts


def host_frame(w, h, ls, off, frame=None, seed=0):
    """A frame inside a padded byte buffer: rows of `ls` bytes starting `off` bytes in; padding random."""
    buf = np.random.RandomState(seed).randint(0, 256, size=off + h * ls + 16, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w, 4), strides=(ls, 4, 1))
    if frame is not None:
        view[...] = frame
    return buf, view


def dev_view(torch, buf, w, h, ls, off):
    t = torch.from_numpy(buf).cuda()
    return t, torch.as_strided(t, (h, w, 4), (ls, 4, 1), off)


def flags_of(levels, delay=1):
    f = ["-d", str(delay)]
    for n in levels:
        f += R.layer_flags(n)
    return f


class Rig:
    """One context, rebound for every layer list; frames in padded buffers of one layout."""

    def __init__(self, w, h, layout):
        import torch
        self.torch = torch
        self.w, self.h = w, h
        self.ls, self.off = geometry(w, layout)
        self.sim = ntscsim.FieldSimulator(device=0)
        self.seed = 2000

    def close(self):
        self.sim.close()

    def averager(self, levels, delay=1):
        return ntscsim.FrameAverager(flags_of(levels, delay), width=self.w, height=self.h, sim=self.sim)

    def frame(self, content=None):
        """(host buffer, host view, device buffer, device view); content None: a test frame with 0xFFFFFFFF and 0 pixels"""
        self.seed += 1
        if content is None:
            content = R.make_frame(self.w, self.h, self.seed)
        buf, view = host_frame(self.w, self.h, self.ls, self.off, content, self.seed)
        dbuf, dview = dev_view(self.torch, buf, self.w, self.h, self.ls, self.off)
        return buf, view, dbuf, dview

    def want_buf(self, f, content):
        want = f[0].copy()
        np.lib.stride_tricks.as_strided(want[self.off:], shape=(self.h, self.w, 4), strides=(self.ls, 4, 1))[...] = content
        return want

    def same(self, dbuf, want_buf, what):
        bad = int((dbuf.cpu().numpy() != want_buf).sum())
        assert bad == 0, "%s: %d bytes differ" % (what, bad)

    def check_frames(self, levels, present=None, field=0, delay=1, kernels=None, what=""):
        """One descriptor through ntscsim_avg_frames_device against the checker.  The destination is a random frame:
        its top bytes are not zero."""
        nl = len(levels)
        present = [1] * nl if present is None else present
        av = self.averager(levels, delay)
        srcs = [self.frame() if present[l] else None for l in range(nl)]
        dst = self.frame()
        assert int(dst[1][:, :, 3].max()) > 0
        av.average_frames([(dst[3], [s[3] if s else None for s in srcs], field)])
        av.sync()
        if kernels is not None:
            assert av.last_kernels() == kernels, what
        frame = np.ascontiguousarray(dst[1])
        R.avg_frame(frame, [s[1] if s else None for s in srcs], levels, field, delay)
        self.same(dst[2], self.want_buf(dst, frame), what)
        for s in srcs:
            if s:
                self.same(s[2], s[0], what + " (source)")
        return frame, np.ascontiguousarray(dst[1])


@pytest.fixture(params=[(w, h, lay) for (w, h) in SIZES for lay in sorted(LAYOUTS)], ids=lambda p: "%dx%d-%s" % p)
def rig(request):
    r = Rig(*request.param)
    yield r
    r.close()


def test_newlevels_in_range_and_wrapping(rig):
    """0, 1, 128, 255, 256 leave the top byte 0 whatever the destination held; 257, 1000, -1, 65536 wrap modulo 2^32
    and carry between the channels and into the top byte: the checker itself must show that, and the device returns
    those bytes."""
    for n in LEVELS:
        got, _ = rig.check_frames([n], field=3, kernels=["k_avg_fast"], what="newlevel %d" % n)
        assert int(got[:, :, 3].max()) == 0
    tops = 0
    for n in WRAPPING:
        got, _ = rig.check_frames([n], field=2, kernels=["k_avg_fast"], what="newlevel %d" % n)
        tops += int((got[:, :, 3] != 0).sum())
    assert tops > 0
    rig.check_frames([128, 300, 0, -7], field=9, kernels=["k_avg_fast"], what="in range and wrapping layers mixed")


def test_fields_and_dither_phases(rig):
    """field 0 .. 11 with delay 3: field / delay differs from field and takes all four phases; one field above 2^32."""
    phases = set()
    for field in range(12):
        rig.check_frames([128], field=field, delay=3, what="field %d" % field)
        phases.add(int(R.dither(1, 1, field, 3)[0, 0]))
    assert phases == {0, 85, 170, 255}
    big = (1 << 32) + 7                                                           # the quotient's low bits differ from those of 7 / 3
    assert int(R.dither(1, 1, big, 3)[0, 0]) != int(R.dither(1, 1, big & 0xFFFFFFFF, 3)[0, 0])
    rig.check_frames([100, 200], field=big, delay=3, what="field 2^32 + 7")
    rig.check_frames([100], field=(1 << 63) + 12345, delay=7, what="field 2^63 + 12345")


def test_layer_counts_and_absent_layers(rig):
    """1, 2, 4 and 5 layers (fast and general form), an absent layer in the middle, and a frame with every layer
    absent: the destination keeps every byte, top bytes included."""
    def levels(n):
        return [(128, 64, 300, 255, 1, -1, 17)[k % 7] for k in range(n)]
    for n in (1, 2, 4, 5):
        rig.check_frames(levels(n), field=n, kernels=["k_avg_general" if n > 4 else "k_avg_fast"], what="%d layers" % n)
    rig.check_frames(levels(3), present=[1, 0, 1], field=5, kernels=["k_avg_fast"], what="absent in the middle")
    rig.check_frames(levels(5), present=[1, 1, 0, 1, 1], field=6, kernels=["k_avg_general"], what="absent in the middle, general")
    for n in (2, 5):
        got, before = rig.check_frames(levels(n), present=[0] * n, field=1, what="every layer absent")
        assert int((got != before).sum()) == 0 and int(got[:, :, 3].max()) > 0


CLIP_LEVELS = {
    "fast1": [128],
    "fast2_wrap": [200, 300],
    "fast3": [64, 256, 1000],
    "fast4": [255, 1, -1, 128],
    "general5": [128, 64, 65536, 0, 200],
}


def _clip_setup(rig, nl, delay, T, absent=()):
    ring = [rig.frame(np.zeros((rig.h, rig.w, 4), np.uint8)) for _ in range(delay)]          # zeroed once :948-970
    src = [[None if (t, l) in absent else rig.frame() for t in range(T)] for l in range(nl)]
    out = [rig.frame(np.full((rig.h, rig.w, 4), 0x5A, np.uint8)) for _ in range(T)]
    return ring, src, out


def _clip_names(nl):
    return ["k_avg_clip_general"] if nl > 4 else ["k_avg_clip_fast<%d>" % nl]


@pytest.mark.parametrize("delay, T", [(1, 11), (2, 11), (3, 11), (5, 11), (9, 11), (9, 5)])
def test_clip_equals_checker_frames_form_and_split_calls(rig, delay, T):
    for form in sorted(CLIP_LEVELS):
        _clip_case(rig, delay, T, form)


def _clip_case(rig, delay, T, form):
    """One clip call, the same clip as two calls (4 frames then the rest; ring, ring index and field carried over) and
    the frames form called frame by frame all give the checker's outputs and leave the checker's ring."""
    levels = CLIP_LEVELS[form]
    nl = len(levels)
    absent = {(2, 0), (4, nl - 1), (6, 0), (6, nl - 1)} if delay in (2, 5) else set()
    field0 = 5
    av = rig.averager(levels, delay)
    ring, src, out = _clip_setup(rig, nl, delay, T, absent)
    cring = [np.zeros((rig.h, rig.w, 4), np.uint8) for _ in range(delay)]
    frames = [[src[l][t][1] if src[l][t] else None for l in range(nl)] for t in range(T)]
    want, want_ri, want_field = R.avg_clip(cring, frames, levels, 0, field0)

    def run(pieces):
        for f in ring:
            f[2].copy_(rig.torch.from_numpy(f[0]))
        for f in out:
            f[2].copy_(rig.torch.from_numpy(f[0]))
        ri, field = 0, field0
        for a, b in pieces:
            ri, field = av.average_clip([f[3] for f in ring], [[(s[3] if s else None) for s in lay[a:b]] for lay in src],
                                        [f[3] for f in out[a:b]], ri, field)
            assert av.last_kernels() == (_clip_names(nl) if b > a else [])
        av.sync()
        assert (ri, field) == (want_ri, want_field)
        for t in range(T):
            rig.same(out[t][2], rig.want_buf(out[t], want[t]), "%s out[%d] %r" % (form, t, pieces))
        for i in range(delay):
            rig.same(ring[i][2], rig.want_buf(ring[i], cring[i]), "%s ring[%d] %r" % (form, i, pieces))

    run([(0, T)])
    run([(0, 4), (4, T)])
    run([(0, 0), (0, 1), (1, T)])
    # the frames form, one call per frame, on the same ring
    for f in ring:
        f[2].copy_(rig.torch.from_numpy(f[0]))
    for t in range(T):
        av.average_frames([(ring[t % delay][3], [(src[l][t][3] if src[l][t] else None) for l in range(nl)], field0 + t)])
        av.sync()
        rig.same(ring[t % delay][2], rig.want_buf(ring[t % delay], want[t]), "%s frames form, frame %d" % (form, t))
    for l in range(nl):
        for s in src[l]:
            if s:
                rig.same(s[2], s[0], "source")


def test_descriptors_of_one_call_take_effect_in_order(rig):
    """Three descriptors, the first and the last on the same destination, the second reading what the first wrote."""
    levels = [128, 300]
    av = rig.averager(levels, 2)
    a, b = rig.frame(), rig.frame()
    s = [rig.frame() for _ in range(5)]
    av.average_frames([(a[3], [s[0][3], s[1][3]], 4), (b[3], [a[3], s[2][3]], 5), (a[3], [s[3][3], s[4][3]], 6)])
    av.sync()
    assert av.last_kernels() == ["k_avg_fast"] * 3
    fa, fb = np.ascontiguousarray(a[1]), np.ascontiguousarray(b[1])
    R.avg_frame(fa, [s[0][1], s[1][1]], levels, 4, 2)
    R.avg_frame(fb, [fa, s[2][1]], levels, 5, 2)
    R.avg_frame(fa, [s[3][1], s[4][1]], levels, 6, 2)
    rig.same(a[2], rig.want_buf(a, fa), "a")
    rig.same(b[2], rig.want_buf(b, fb), "b")
    # independent descriptors share one launch
    c = rig.frame()
    av.average_frames([(a[3], [s[0][3], s[1][3]], 0), (c[3], [s[2][3], s[3][3]], 1)])
    av.sync()
    assert av.last_kernels() == ["k_avg_fast"]


def test_host_frames_equal_device_call(rig):
    levels = [128, -1]
    av = rig.averager(levels, 3)
    w, h = rig.w, rig.h
    dst = [rig.frame(), rig.frame()]
    src = [rig.frame() for _ in range(3)]
    jobs = [(0, [0, 1], 0), (1, [2, None], 4), (0, [1, 2], (1 << 32) + 8)]
    av.average_frames([(dst[d][3], [(src[k][3] if k is not None else None) for k in ss], f) for d, ss, f in jobs])
    av.sync()
    hbuf = [f[0].copy() for f in dst]
    hview = [np.lib.stride_tricks.as_strided(bf[rig.off:], shape=(h, w, 4), strides=(rig.ls, 4, 1)) for bf in hbuf]
    av.average_frames_host([(hview[d], [(src[k][1] if k is not None else None) for k in ss], f) for d, ss, f in jobs])
    for d in range(2):
        rig.same(dst[d][2], hbuf[d], "host call, destination %d" % d)
    want = [np.ascontiguousarray(f[1]) for f in dst]
    for d, ss, f in jobs:
        R.avg_frame(want[d], [(src[k][1] if k is not None else None) for k in ss], levels, f, 3)
    for d in range(2):
        assert int((hview[d] != want[d]).sum()) == 0


def test_full_size_frame():
    """720 x 480, two layers: the frames form and a short clip."""
    r = Rig(720, 480, "aligned")
    try:
        levels = [128, 200]
        r.check_frames(levels, field=7, delay=2, kernels=["k_avg_fast"], what="720x480")
        av = r.averager(levels, 2)
        ring, src, out = _clip_setup(r, 2, 2, 3)
        ri, field = av.average_clip([f[3] for f in ring], [[s[3] for s in lay] for lay in src], [f[3] for f in out], 0, 0)
        av.sync()
        assert av.last_kernels() == ["k_avg_clip_fast<2>"]
        cring = [np.zeros((480, 720, 4), np.uint8) for _ in range(2)]
        want, wri, wfield = R.avg_clip(cring, [[src[l][t][1] for l in range(2)] for t in range(3)], levels, 0, 0)
        assert (ri, field) == (wri, wfield)
        for t in range(3):
            r.same(out[t][2], r.want_buf(out[t], want[t]), "out[%d]" % t)
        for i in range(2):
            r.same(ring[i][2], r.want_buf(ring[i], cring[i]), "ring[%d]" % i)
    finally:
        r.close()


def test_error_codes():
    import torch
    sim = ntscsim.FieldSimulator(device=0)
    try:
        lib = sim._lib
        a = torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda")
        b = torch.zeros((32, 96, 4), dtype=torch.uint8, device="cuda")
        small = torch.zeros((32, 64, 4), dtype=torch.uint8, device="cuda")
        # unbound ctx
        d = _capi.AvgDesc()
        assert lib.ntscsim_avg_frames_device(sim._h, C.byref(d), 1, None) == _capi.E_ARG
        assert lib.ntscsim_avg_frames_host(sim._h, C.byref(d), 1) == _capi.E_ARG
        # bad delay, bad sizes
        for delay in (0, 257):
            p = _capi.make_avg_params(["-i", "x"], width=96, height=32)
            p.delay = delay
            with pytest.raises(ntscsim.NtscsimError) as e:
                ntscsim.FrameAverager(params=p, sim=sim)
            assert e.value.code == _capi.E_PARAM
        for wh in ((0, 32), (96, 0), (65537, 32), (65536, 32768)):
            with pytest.raises(ntscsim.NtscsimError) as e:
                ntscsim.FrameAverager(["-i", "x"], width=wh[0], height=wh[1], sim=sim)
            assert e.value.code == _capi.E_SIZE
        av = ntscsim.FrameAverager(["-i", "x", "-n", "96", "-i", "y"], width=96, height=32, sim=sim)
        with pytest.raises(ntscsim.NtscsimError) as e:
            av.average_frames([(small, [small, small], 0)])                       # not the bound size
        assert e.value.code == _capi.E_SIZE
        with pytest.raises(ntscsim.NtscsimError) as e:
            av.average_frames([(a, [b], 0)])                                      # not the bound layer count
        assert e.value.code == _capi.E_SIZE
        wide = torch.zeros((32, 97, 4), dtype=torch.uint8, device="cuda")
        odd = torch.as_strided(wide, (32, 96, 4), (386, 4, 1), 0)
        with pytest.raises(ntscsim.NtscsimError) as e:
            av.average_frames([(odd, [b, b], 0)])                                 # linesize not a multiple of 4
        assert e.value.code == _capi.E_SIZE
        with pytest.raises(ntscsim.NtscsimError) as e:
            av.average_frames([(a, [b, a], 0)])                                   # a source overlaps the destination
        assert e.value.code == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            av.average_clip([a], [[b], [a]], [torch.zeros_like(a)])               # a source overlaps the ring
        assert e.value.code == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            av.average_clip([a], [[b], [b]], [a])                                 # an output overlaps the ring
        assert e.value.code == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:
            av.average_clip([a], [[b], [b]], [torch.zeros_like(a)], ring_index=1)  # ring index outside the ring
        assert e.value.code == _capi.E_ARG
        av.average_frames([])
        av.average_frames([(a, [b, None], 0)])
        av.sync()
    finally:
        sim.close()


def test_simulator_output_is_averaged_without_leaving_the_device():
    """A few -vhs fields from ntscsim_fields_device stay in device memory and go into the average stage as its only
    layer: the result is the checker applied to the simulator's downloaded output, and it trails."""
    import torch
    w, h, n = 96, 32, 4
    p = L.make_params(["-vhs"])
    sim = ntscsim.FieldSimulator(params=p, device=0)
    try:
        levels = [96]
        av = ntscsim.FrameAverager(flags_of(levels, 2), width=w, height=h, sim=sim)
        frames = np.stack([L.noise_frame(w, h, 0x51 + i) for i in range(n // 2)])
        jobs = [(k // 2, k, (k & 1) ^ 1, k) for k in range(n)]
        src = torch.from_numpy(frames).cuda()
        fields = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
        sim.fields(src, fields, jobs)
        ring = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
        out = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda") for _ in range(n)]
        ri, field = av.average_clip(ring, [[fields[t] for t in range(n)]], out)
        av.sync()
        sim_out = fields.cpu().numpy()
        cring = [np.zeros((h, w, 4), np.uint8) for _ in range(2)]
        want, wri, wfield = R.avg_clip(cring, [[sim_out[t]] for t in range(n)], levels)
        assert (ri, field) == (wri, wfield) == (0, n)
        got = np.stack([o.cpu().numpy() for o in out])
        assert int((got != want).sum()) == 0
        assert int((got[:, :, :, :3] != sim_out[:, :, :, :3]).sum()) > 0            # an average, not a copy
    finally:
        sim.close()
