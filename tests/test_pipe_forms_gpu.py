"""Every role form of the BGRA tool in double (csrc/ntsc_pipe.hip: k_field_pipe<RT,WR,SV,XA,CATV>, k_field_pipe_tv<RT,CATV>)
against the oracle, row by row of tests/_pipe_forms.py: ONE ntscsim_fields_device() launch in the latency form per row on a
fresh context, the kernel asserted by name (exactly one role kernel, or none and the one-launch decoder of the fallback), the
rand() position, and the launch's WHOLE destination buffer -- every frame with the padding behind its rows, the other
field's rows, a guard frame behind the last -- byte for byte against OracleStream (tolerance zero, nothing excluded).  Where
the exposed composite plane is the oracle's tap it is compared too: a difference there is the encoder role's, one in the
bytes alone a decoder role's.  A hand-off between two roles that timed out is reported by the NEXT call on the context
(NTSCSIM_E_HIP): every row makes one -- the same launch in the throughput form, compared as well, which also tells an
arithmetic difference (both forms) from one of the hand-offs or trip counts (the role form alone).
tests/test_pipe_forms_host.py shows on the CPU what the rows cover.  The threshold widths run again in NTSCSIM_MODE_FAST32
(role form == throughput form, which tests/test_fast32_forms_gpu.py holds to its model), and the synchronous entry point,
ntscsim_field(), runs each form below its steady threshold, at it and at 720x486, on plain and on pinned frames.
"""
import ctypes as C

import numpy as np
import pytest

import _libs as L
import _pipe_forms as T
import ntscsim
from ntscsim import _capi

pytestmark = pytest.mark.gpu

DECODERS = ("k_decode", "k_vcr_front")


def launch(torch, sim, row, c, latency):
    """the row's launch on fresh device frames: (bytes after, kernel names, rand() position, sources after, sources before,
    composite plane)"""
    w, h, n = row.w, row.h, row.n
    spw = (w + 4) // 4 * 4
    src0 = np.zeros((len(c.srcs), h, spw, 4), np.uint8)
    src0[:, :, :w] = np.stack(c.srcs)
    src = torch.from_numpy(src0).cuda()
    dst = torch.full((n + 1, h, T.row_pixels(row), 4), T.FILL, dtype=torch.uint8, device="cuda")
    sim.set_launch_form(latency)
    sim.rng_pos = 0
    sim.fields(src[:, :, :w], dst[:n, :, :w], [(si, k, field, fieldno) for k, (si, field, fieldno) in enumerate(c.jobs)])
    sim.sync()                                   # (raises with the context's error text unless NTSCSIM_OK)
    return dst.cpu().numpy(), sim.last_kernels(), sim.rng_pos, src.cpu().numpy(), src0, sim.debug_composite(n, w, h)


def differing(got, exp):
    bad = got != exp
    if not bad.any():
        return "equal"
    k, y, x, ch = (int(v) for v in np.argwhere(bad)[0])
    return "%d bytes differ, first in frame %d row %d pixel %d byte %d: %d for %d" % (int(bad.sum()), k, y, x, ch, int(got[k, y, x, ch]),
                                                                                       int(exp[k, y, x, ch]))


def plane_differing(comp, c):
    for k, tap in enumerate(c.comp):
        bad = comp[k, :tap.shape[0]] != tap
        if bad.any():
            r, x = (int(v) for v in np.argwhere(bad)[0])
            return "%d samples of field %d differ, first in row %d column %d" % (int(bad.sum()), k, r, x)
    return "equal"


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.id)
def test_role_form_equals_the_oracle(row):
    import torch
    c = T.case(row.id)
    p = T.params(row)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        if row.id in T.DEBUG:
            sim.debug_no_fast_decode(T.DEBUG[row.id])
        got, ran, pos, src, src0, comp = launch(torch, sim, row, c, True)
        # the further call on the same context: NTSCSIM_OK, or the role kernel's hand-off timed out
        got1, ran1, pos1, src1, _, comp1 = launch(torch, sim, row, c, False)
    finally:
        sim.close()
    roles = [k for k in ran if k.startswith("k_field_pipe")]
    assert roles == ([row.kernel] if row.kernel else []), ran
    dec = [k for k in ran if k.startswith(DECODERS)]
    assert dec == ([row.fallback] if row.fallback else []), ran
    one = T.launcher_name(p, row.w, row.n, aligned=row.id not in T.UNALIGNED, latency=False, debug=T.DEBUG.get(row.id, 0),
                          ghost=len(T.GHOST.get(row.id, ())))[1]
    assert not any(k.startswith("k_field_pipe") for k in ran1) and [k for k in ran1 if k.startswith(DECODERS)] == [one], ran1
    assert not any("float" in k for k in ran + ran1), (ran, ran1)
    assert pos == c.rng_pos and pos1 == c.rng_pos, (pos, pos1, c.rng_pos)
    role, wave = differing(got, c.exp), differing(got1, c.exp)
    plane = plane_differing(comp, c) if T.plane_is_the_tap(row) else "not compared"
    assert role == "equal", "%s: %s (composite plane: %s); the throughput form %s: %s" % (ran, role, plane, ran1, wave)
    assert wave == "equal", "%s: %s" % (ran1, wave)
    if T.plane_is_the_tap(row):
        assert plane == "equal", "%s: composite plane: %s" % (ran, plane)
        assert plane_differing(comp1, c) == "equal", ran1
    assert np.array_equal(src, src0) and np.array_equal(src1, src0)


def test_every_role_name_was_asked_for():
    """(the names are asserted row by row above; this is the table's side of "each of the seven runs by name")"""
    assert {r.kernel for r in T.ROWS if r.kernel} == set(T.ROLE_NAMES) == {s.kernel for s in T.SYNC}
    assert len(T.ROLE_NAMES) == 7 and all(r.fallback for r in T.ROWS if not r.kernel)


def test_frames_narrower_than_the_steady_threshold_of_the_forms_without_the_vcr_are_refused():
    """k_field_pipe_tv has a steady loop from 12 columns on; the C ABI takes frames from 16 columns: the other side of that
    condition cannot be reached, which is why the table starts those families at 16"""
    import torch
    w = T.steady_first(0, False, True) - 1
    sim = ntscsim.FieldSimulator(params=L.make_params([]))
    try:
        sim.set_launch_form(True)
        src = torch.zeros((1, 10, 16, 4), dtype=torch.uint8, device="cuda")
        dst = torch.zeros((1, 10, 16, 4), dtype=torch.uint8, device="cuda")
        with pytest.raises(ntscsim.NtscsimError) as e:
            sim.fields(src[:, :, :w], dst[:, :, :w], [(0, 0, 1, 0)])
        assert e.value.code == _capi.E_SIZE and sim.rng_pos == 0
    finally:
        sim.close()


# ------------------------------------------------------------------------------------------------ NTSCSIM_MODE_FAST32
FAST32 = [(f, w) for f in T.FAMILIES for w in T.threshold_widths(f)]


@pytest.mark.parametrize("f,w", FAST32, ids=["%s_w%d" % (f.tag, w) for f, w in FAST32])
def test_fast32_role_form_equals_its_throughput_form(f, w):
    """the float twins of the role kernels at the threshold widths: the same bytes, rand() position and composite plane as
    the one-launch forms of the mode (held to the fast32 model by tests/test_fast32_forms_gpu.py)"""
    import torch
    row = T.Row("%s_fast32_w%d" % (f.tag, w), T.fam_flags(f, w), w, 10, 2, "noise", f.kernel, None, f.hs)
    srcs = T.sources("noise", w, 10)
    c = T.Case(srcs, [(k % len(srcs), (k & 1) ^ 1, k) for k in range(2)], None, None, None, None)
    res = []
    for latency in (True, False):
        sim = ntscsim.FieldSimulator(params=L.make_params(row.flags))
        try:
            sim.set_mode(_capi.MODE_FAST32)
            res.append(launch(torch, sim, row, c, latency))
        finally:
            sim.close()
    (got, ran, pos, src, src0, comp), (got1, ran1, pos1, src1, _, comp1) = res
    assert [k for k in ran if k.startswith("k_field_pipe")] == [T.FLOAT_NAME[f.kernel]], ran
    assert not any(k.startswith("k_field_pipe") for k in ran1) and len([k for k in ran1 if k.startswith(DECODERS)]) == 1, ran1
    assert not any("double" in k for k in ran + ran1), (ran, ran1)
    assert pos == pos1 > 0
    assert differing(got, got1) == "equal", (ran, ran1, differing(got, got1))
    assert np.array_equal(comp, comp1), (ran, ran1)
    assert (got[2] == T.FILL).all() and (got[:, :, w:] == T.FILL).all() and not got[0, 1::2, :w, 3].any()
    assert np.array_equal(src, src0) and np.array_equal(src1, src0)


# ------------------------------------------------------------------------------------------------ ntscsim_field()
class HostFrame:
    """a BGRA frame inside a block of bytes that is compared whole: a numpy block with 64 bytes around a tight frame, or
    pinned memory from ntscsim_host_frame_alloc (rows of a multiple of 64 bytes, 64 spare bytes)"""

    def __init__(self, w, h, pinned):
        self.base = None
        if pinned:
            rb, rows = (C.c_int * 1)(w * 4), (C.c_int * 1)(h)
            data, ls = (C.c_void_p * 1)(), (C.c_int * 1)()
            base, nbytes = C.c_void_p(), C.c_size_t()
            rc = ntscsim.lib().ntscsim_host_frame_alloc(1, rb, rows, 64, data, ls, C.byref(base), C.byref(nbytes))
            assert rc == _capi.OK and ls[0] % 64 == 0 and ls[0] >= w * 4
            self.base = base
            self.block = np.frombuffer((C.c_uint8 * nbytes.value).from_address(base.value), np.uint8)
            off, stride = data[0] - base.value, ls[0]
        else:
            self.block = np.empty(h * w * 4 + 128, np.uint8)
            off, stride = 64, w * 4
        self.block[:] = 0xA7
        self.view = np.lib.stride_tricks.as_strided(self.block[off:], shape=(h, w, 4), strides=(stride, 4, 1))

    def expect(self, frame):
        """the block with `frame` in the frame's bytes and everything else as it was made"""
        e = np.full_like(self.block, 0xA7)
        off = self.view.ctypes.data - self.block.ctypes.data
        np.lib.stride_tricks.as_strided(e[off:], shape=self.view.shape, strides=self.view.strides)[:] = frame
        return e

    def free(self):
        if self.base is not None:
            self.view = self.block = None
            ntscsim.lib().ntscsim_host_free(self.base)
            self.base = None


@pytest.mark.parametrize("pinned", [False, True], ids=["numpy", "pinned"])
@pytest.mark.parametrize("row", T.SYNC, ids=lambda r: r.id)
def test_synchronous_call_takes_the_role_form_at_the_widths_of_its_loops(row, pinned):
    """ntscsim_field() call after call on ONE context: two calls at the row's geometry, one at 48x14, two more at the
    row's -- the setup kernel the previous call launched ahead for the next one is used, thrown away and used again -- and a
    closing call, which reports a hand-off of the call before it that timed out.  The form by name at every call; the
    destination blocks == the oracle's loop, whole; the source blocks unchanged; on pinned frames every source is read and
    every destination written in place."""
    p = L.make_params(row.flags, output_height=row.h)
    geoms = [(row.w, row.h), T.SYNC_OTHER]
    dst = [HostFrame(w, h, pinned) for w, h in geoms]
    src = [HostFrame(w, h, pinned) for w, h in geoms]
    exp = [np.full((h, w, 4), 0x5A, np.uint8) for w, h in geoms]
    for d in dst:
        d.view[:] = 0x5A
    o = L.OracleStream(p)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        for k, gi in enumerate((0, 0, 1, 0, 0, 0)):
            w, h = geoms[gi]
            field = (k & 1) ^ 1
            s = L.noise_frame(w, h, 100 + k)
            src[gi].view[:] = s
            keep = src[gi].block.copy()
            sim.field_host(dst[gi].view, src[gi].view, field, k)
            o.field(exp[gi], s, field, k)
            kern = sim.last_kernels()
            assert [x for x in kern if x.startswith("k_field_pipe")] == [row.kernel], (k, kern)
            assert np.array_equal(dst[gi].block, dst[gi].expect(exp[gi])), "call %d: %s" % (k, differing(dst[gi].view[None], exp[gi][None]))
            assert np.array_equal(src[gi].block, keep), k
            assert sim.rng_pos == o.rng_pos, k
        st = sim.debug_field_stats()
        assert st[0] == 6 and (not pinned or (st[1] == 6 and st[2] == 6)), st
    finally:
        sim.close()
        for f in dst + src:
            f.free()
