"""The device half of the scanimate stage (ntscsim_scan_frames_device / _clip_device / _frames_host) against the
checker tests/_scan_ref.py.  The stage is bit-identical to the tool -- an integer accumulator, IEEE fp64 in the tool's
order, the tool's sin / cos from the host's libm -- so the tolerance is zero: the accumulator tap is compared word for
word, every byte of every destination buffer is compared (row padding, guard bytes and the untouched row 0 included)
and the sources are checked to be unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

import _libs as L  # noqa: F401
import _scan_ref as R
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

# name: (src_w, src_h, dst_w, dst_h, -inntsc)
SHAPES = {
    "mono24x40": (24, 40, 36, 24, 0),
    "ntsc24x24": (24, 24, 36, 24, 1),
    "ntsc20x16": (20, 16, 64, 48, 1),       # radius 6.15: dot boxes of 13 x 14 pixels and more
    "odd25x37": (25, 37, 37, 23, 0),        # nothing is a multiple of anything
    "multi150x200": (150, 200, 180, 120, 0),   # two tiles across, thirteen strips down: windows overlap, the flushes must add
}
# trapezoid | rotate, 270: signal exactly 0, 271 / 359: flipped | stretch, mostly off the screen | sine tables, ef_t of
# both signs | the wrap to effect 0 | beyond 32 bits
FIELDNOS = [0, 45, 179, 181, 269, 270, 271, 359, 361, 500, 539, 541, 585, 700, 720, (1 << 32) + 5]
SPILL_FIELDNOS = [0, 500, 585]
# rows 16-byte aligned (the vector path) | linesize and base pointer only 4-byte aligned (the dword path)
LAYOUTS = {"aligned": (16, 0), "unaligned": (4, 4)}
KERNELS = ["k_scan_splat", "k_scan_resolve"]
KERNELS_SPILL = ["k_scan_splat+spill", "k_scan_resolve"]


@functools.lru_cache(maxsize=None)
def source(sw, sh, seed=0):
    f = R.make_source(sw, sh, 5000 + sw * 131 + sh + seed)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(name, fieldno, seed=0):
    """(accumulator, BGRA field) of the checker: computed once, shared by the tests, never written."""
    sw, sh, dw, dh, inntsc = SHAPES[name]
    acc, out = R.scan_field(source(sw, sh, seed), dw, dh, inntsc, fieldno)
    acc.setflags(write=False)
    out.setflags(write=False)
    return acc, out


def host_frame(w, h, ls, off, frame=None, seed=0):
    """A frame inside a padded byte buffer: rows of `ls` bytes starting `off` bytes in; padding and guards random."""
    buf = np.random.RandomState(seed).randint(0, 256, size=off + h * ls + 16, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w, 4), strides=(ls, 4, 1))
    if frame is not None:
        view[...] = frame
    return buf, view


class Rig:
    """One context bound for one shape; frames in padded buffers of one layout."""

    def __init__(self, name, layout="aligned"):
        import torch
        self.torch = torch
        self.name = name
        self.sw, self.sh, self.dw, self.dh, self.inntsc = SHAPES[name]
        self.pad, self.off = LAYOUTS[layout]
        self.sc = ntscsim.Scanimator(["-inntsc"] if self.inntsc else [], width=self.dw, height=self.dh)
        self.sc.debug_keep_raster(True)
        self.seed = 100

    def close(self):
        self.sc.close()

    def frame(self, w, h, content=None):
        """(host buffer, host view, device buffer, device view)"""
        self.seed += 1
        ls = 4 * w + self.pad
        buf, view = host_frame(w, h, ls, self.off, content, self.seed)
        t = self.torch.from_numpy(buf).cuda()
        return buf, view, t, self.torch.as_strided(t, (h, w, 4), (ls, 4, 1), self.off)

    def src(self, seed=0):
        return self.frame(self.sw, self.sh, source(self.sw, self.sh, seed))

    def dst(self):
        return self.frame(self.dw, self.dh)

    def want_buf(self, f, out, field, zero_row0=False):
        """The destination buffer behind the call: rows field .. replaced, everything else as it was."""
        want = f[0].copy()
        v = np.lib.stride_tricks.as_strided(want[self.off:], shape=(self.dh, self.dw, 4), strides=(4 * self.dw + self.pad, 4, 1))
        v[field:] = out[field:]
        if zero_row0:
            v[:field] = 0
        return want

    def same(self, dbuf, want, what):
        bad = int((dbuf.cpu().numpy() != want).sum())
        assert bad == 0, "%s %s: %d bytes differ" % (self.name, what, bad)

    def check(self, fieldno, kernels=None, what=""):
        acc, out = reference(self.name, fieldno)
        s, d = self.src(), self.dst()
        self.sc.scan_frames([(d[3], s[3], fieldno)])
        self.sc.sync()
        what = "%s field %d" % (what, fieldno)
        if kernels is not None:
            assert self.sc.last_kernels() == kernels, what
        bad = int((self.sc.debug_raster() != acc).sum())
        assert bad == 0, "%s %s: %d accumulator words differ" % (self.name, what, bad)
        self.same(d[2], self.want_buf(d, out, R.field_of(fieldno)), what)
        self.same(s[2], s[0], what + " (source)")


@pytest.fixture(params=[(n, lay) for n in SHAPES for lay in sorted(LAYOUTS)], ids=lambda p: "%s-%s" % p)
def rig(request):
    r = Rig(*request.param)
    yield r
    r.close()


def test_every_effect_and_parity(rig):
    assert set(R.effect_of(f)[0] for f in FIELDNOS) == {0, 1, 2, 3} and set(R.field_of(f) for f in FIELDNOS) == {0, 1}
    for fieldno in FIELDNOS:
        rig.check(fieldno)
    acc, out = reference(rig.name, 270)
    assert int(acc.max()) == 0 and int(out[..., :3].max()) == 0                  # |1 - 2 * 90 / 180| = 0: a black field


def test_window_and_spill_give_the_same_bytes(rig):
    """ntscsim_scan_debug_set_window_rows: 0 sends every add to the plane, 2 leaves a window that holds part of every
    dot; the kernel says that it spilled and the bytes stay the checker's."""
    for rows in (0, 2):
        rig.sc.debug_set_window_rows(rows)
        for fieldno in SPILL_FIELDNOS:
            rig.check(fieldno, KERNELS_SPILL, "window of %d rows" % rows)
    rig.sc.debug_set_window_rows(-1)
    rig.check(585)


def test_default_window_holds_a_small_field():
    r = Rig("mono24x40")
    try:
        r.check(0, KERNELS, "default window")
        wgs, spilled = r.sc.debug_spill()
        assert wgs >= 1 and spilled == 0
        r.sc.debug_set_window_rows(0)
        r.check(0, KERNELS_SPILL, "no window")
        wgs, spilled = r.sc.debug_spill()
        assert wgs >= 1 and spilled == wgs
    finally:
        r.close()


def test_the_output_compare_means_something():
    """The clamp at 255 hides accumulator errors in saturated pixels.  The share of saturated pixels is asserted on the
    checker's field: the mono 24 x 40 -> 36 x 24 shape with a uniform-random source has none up to field number 500."""
    some = 0
    for fieldno in [f for f in FIELDNOS if f <= 500]:
        acc, out = reference("mono24x40", fieldno)
        lit = out[R.field_of(fieldno):, :, 0] > 0
        sat = out[R.field_of(fieldno):, :, 0] == 255
        assert int(sat.sum()) == 0, fieldno
        some += int(lit.sum())
    assert some > 1000


def test_clip_crosses_an_effect_boundary(rig):
    """Six fields from field number 177: effects 0 and 1, both parities.  Against six scan_frames calls on zeroed
    frames and against the checker; row 0 of the field == 1 outputs is zero; the field number ends six higher."""
    r = rig
    T, first = 6, 177
    srcs = [r.src(seed=t) for t in range(T)]
    outs = [r.dst() for _ in range(T)]
    assert r.sc.scan_clip([s[3] for s in srcs], [o[3] for o in outs], fieldno=first) == first + T
    r.sc.sync()
    assert r.sc.last_kernels() == KERNELS
    singles = [r.dst() for _ in range(T)]
    for t in range(T):
        singles[t][3].zero_()
        r.sc.scan_frames([(singles[t][3], srcs[t][3], first + t)])
    r.sc.sync()
    parities = set()
    for t in range(T):
        fieldno = first + t
        field = R.field_of(fieldno)
        parities.add(field)
        acc, out = R.scan_field(source(r.sw, r.sh, t), r.dw, r.dh, r.inntsc, fieldno)
        r.same(outs[t][2], r.want_buf(outs[t], out, field, zero_row0=True), "clip frame %d" % t)
        got = outs[t][3].cpu().numpy()
        assert int((got != singles[t][3].cpu().numpy()).sum()) == 0, t
        if field == 1:
            assert int(got[0].max()) == 0 and int(got[1:, :, 3].min()) == 255
        r.same(srcs[t][2], srcs[t][0], "clip source %d" % t)
    assert parities == {0, 1}


def test_a_call_of_many_descriptors_takes_effect_in_order():
    """More descriptors than accumulator planes, sources of two sizes, a destination written twice (the later field
    stays) and a destination that is a later descriptor's source: the call is cut into launches where it has to be."""
    r = Rig("mono24x40")
    try:
        other = r.frame(25, 37, source(25, 37))
        s = r.src()
        dsts = [r.dst() for _ in range(14)]
        view = lambda buf: np.lib.stride_tricks.as_strided(buf[r.off:], shape=(r.dh, r.dw, 4), strides=(4 * r.dw + r.pad, 4, 1))
        jobs, want = [], {}

        def job(i, src_dev, src_host, fieldno):
            jobs.append((dsts[i][3], src_dev, fieldno))
            acc, out = R.scan_field(np.ascontiguousarray(src_host), r.dw, r.dh, 0, fieldno)
            want[i] = r.want_buf(dsts[i], out, R.field_of(fieldno))
            return acc

        job(0, s[3], s[1], 0)
        job(1, other[3], other[1], 181)
        job(0, s[3], s[1], 45)                      # the same destination again: field 0 of both, so the later one stays whole
        job(3, dsts[0][3], view(want[0]), 361)      # reads what the descriptor before it wrote
        for i in range(4, 14):                      # ten more: over the plane count
            acc = job(i, (other if i % 3 == 1 else s)[3], (other if i % 3 == 1 else s)[1], FIELDNOS[i])
        r.sc.scan_frames(jobs)
        r.sc.sync()
        assert r.sc.last_kernels() == KERNELS * 4   # descriptors 0 1 | 2 | 3 .. 10 | 11 .. 13
        for i, w in want.items():
            r.same(dsts[i][2], w, "destination %d" % i)
        assert int((r.sc.debug_raster() != acc).sum()) == 0
        r.same(s[2], s[0], "source")
        r.same(other[2], other[0], "source of the other size")
    finally:
        r.close()


def test_sine_tables_of_more_source_sizes_than_the_ctx_keeps():
    """The ctx keeps the sine effect's tables of four source sizes.  Six sizes on one ctx: the cache filled one call at a
    time, then one call that mixes the oldest cached size with a new one (the new one must not push out what the
    launch being built already points at), one call with all six in a single launch, and the first size once more."""
    r = Rig("mono24x40", "unaligned")
    try:
        sizes = [(24, 40), (25, 37), (20, 16), (24, 24), (30, 22), (18, 26)]
        frames = [r.frame(w, h, source(w, h)) for (w, h) in sizes]

        def scan(which, fieldnos, what):
            dsts = [r.dst() for _ in which]
            r.sc.scan_frames([(d[3], frames[i][3], f) for d, i, f in zip(dsts, which, fieldnos)])
            r.sc.sync()
            assert r.sc.last_kernels() == KERNELS, what
            for d, i, f in zip(dsts, which, fieldnos):
                assert R.effect_of(f)[0] == 3
                acc, out = R.scan_field(np.ascontiguousarray(frames[i][1]), r.dw, r.dh, 0, f)
                r.same(d[2], r.want_buf(d, out, R.field_of(f)), "%s, size %dx%d field %d" % ((what,) + sizes[i] + (f,)))
            assert int((r.sc.debug_raster() != acc).sum()) == 0, what

        for i in range(4):
            scan([i], [541 + i], "filling the cache")
        scan([0, 4], [585, 700], "the oldest cached size beside a new one")
        scan([0, 1, 2, 3, 4, 5], [541, 542, 585, 586, 700, 701], "six sizes in one launch")
        scan([5, 0], [550, 551], "behind the launch that outgrew the cache")
        scan([2, 3, 1], [560, 561, 562], "sizes that were dropped come back")
        for f in frames:
            r.same(f[2], f[0], "source")
    finally:
        r.close()


def test_frames_host_gives_the_device_bytes(rig):
    r = rig
    for fieldno in (45, 180, 585):
        acc, out = reference(r.name, fieldno)
        s, d = r.src(), r.dst()
        hs, hd = s[0].copy(), d[0].copy()
        ls_s, ls_d = 4 * r.sw + r.pad, 4 * r.dw + r.pad
        sv = np.lib.stride_tricks.as_strided(hs[r.off:], shape=(r.sh, r.sw, 4), strides=(ls_s, 4, 1))
        dv = np.lib.stride_tricks.as_strided(hd[r.off:], shape=(r.dh, r.dw, 4), strides=(ls_d, 4, 1))
        r.sc.scan_frames_host([(dv, sv, fieldno)])
        r.sc.scan_frames([(d[3], s[3], fieldno)])
        r.sc.sync()
        assert int((hd != d[2].cpu().numpy()).sum()) == 0, fieldno
        assert int((hd != r.want_buf(d, out, R.field_of(fieldno))).sum()) == 0, fieldno
        assert int((hs != s[0]).sum()) == 0


def desc_of(dst, src, fieldno=0, **over):
    d = _capi.ScanDesc()
    d.dst_dev, d.dst_linesize = dst.data_ptr(), dst.stride(0)
    d.src_dev, d.src_linesize, d.src_width, d.src_height = src.data_ptr(), src.stride(0), src.shape[1], src.shape[0]
    d.fieldno = fieldno
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_error_codes_and_no_launch():
    import torch
    r = Rig("mono24x40")
    try:
        lib, h = r.sc._lib, r.sc.sim._h
        s, d = r.src(), r.dst()
        r.check(45, KERNELS)                                                     # a good call first: its kernels stay the last ones
        before = d[2].clone()

        def rc_of(desc):
            return lib.ntscsim_scan_frames_device(h, C.byref(desc), 1, None)

        assert rc_of(desc_of(d[3], s[3], dst_dev=None)) == _capi.E_ARG
        assert rc_of(desc_of(d[3], s[3], src_dev=None)) == _capi.E_ARG
        assert lib.ntscsim_scan_frames_device(h, None, 1, None) == _capi.E_ARG
        assert rc_of(desc_of(d[3], s[3], dst_linesize=4 * r.dw - 4)) == _capi.E_SIZE
        assert rc_of(desc_of(d[3], s[3], dst_linesize=4 * r.dw + 2)) == _capi.E_SIZE
        assert rc_of(desc_of(d[3], s[3], src_linesize=4 * r.sw - 4)) == _capi.E_SIZE
        assert rc_of(desc_of(d[3], s[3], src_linesize=4 * r.sw + 2)) == _capi.E_SIZE
        assert rc_of(desc_of(d[3], s[3], src_width=0)) == _capi.E_SIZE
        assert rc_of(desc_of(d[3], s[3], src_width=65537, src_linesize=4 * 65537)) == _capi.E_SIZE
        assert rc_of(desc_of(d[3], s[3], src_width=32768, src_height=32768, src_linesize=4 * 32768)) == _capi.E_SIZE   # 2 w h = 2^31
        # a source that overlaps the destination: the destination's own memory read as a 24 x 40 frame would need more
        # bytes than it has, so a source inside the destination buffer that fits
        inside = torch.as_strided(d[2], (4, 8, 4), (d[3].stride(0), 4, 1), r.off)
        assert rc_of(desc_of(d[3], inside)) == _capi.E_ARG
        with pytest.raises(ntscsim.NtscsimError) as e:                           # a destination of another size than the bound one
            r.sc.scan_frames([(r.frame(r.dw + 1, r.dh)[3], s[3], 0)])
        assert e.value.code == _capi.E_SIZE
        fn = C.c_uint64(0)
        sp, op = (C.c_void_p * 2)(s[3].data_ptr(), s[3].data_ptr()), (C.c_void_p * 2)(d[3].data_ptr(), d[3].data_ptr())
        assert lib.ntscsim_scan_clip_device(h, sp, s[3].stride(0), r.sw, r.sh, op, d[3].stride(0), 2, C.byref(fn), None) == _capi.E_ARG
        assert fn.value == 0                                                     # outputs that overlap each other
        assert lib.ntscsim_scan_clip_device(h, sp, s[3].stride(0), r.sw, r.sh, op, d[3].stride(0), 1, None, None) == _capi.E_ARG
        r.sc.sync()
        assert r.sc.last_kernels() == KERNELS                                    # none of them launched or cleared the list
        assert int((d[2] != before).sum().item()) == 0

        # no bind before
        fresh = ntscsim.FieldSimulator(device=0)
        try:
            assert lib.ntscsim_scan_frames_device(fresh._h, C.byref(desc_of(d[3], s[3])), 1, None) == _capi.E_ARG
            assert lib.ntscsim_scan_frames_host(fresh._h, C.byref(desc_of(d[3], s[3])), 1) == _capi.E_ARG
            assert lib.ntscsim_scan_debug_set_window_rows(fresh._h, 0) == _capi.E_ARG
            # bind limits
            for over in (dict(output_width=0), dict(output_height=0), dict(output_width=65537), dict(output_height=65537),
                         dict(output_width=65536, output_height=32768), dict(src_width=0), dict(src_height=65537),
                         dict(src_width=32768, src_height=32768)):
                p = _capi.make_scan_params([])
                for k, v in over.items():
                    setattr(p, k, v)
                assert lib.ntscsim_scan_bind(fresh._h, C.byref(p)) == _capi.E_SIZE, over
            p = _capi.make_scan_params([])
            p.struct_size = 8
            assert lib.ntscsim_scan_bind(fresh._h, C.byref(p)) == _capi.E_ARG
            assert fresh.last_kernels() == []
        finally:
            fresh.close()
    finally:
        r.close()
