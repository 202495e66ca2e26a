"""Every role form of the YUV422P tool (csrc/ntsc422_fused.hip: k422_pipe<SPEC,DD,SVID>, k422_short_pipe) against the oracle,
row by row of tests/_pipe422_forms.py: ONE ntscsim_fields422_device() launch in the latency form per row, the kernel asserted
by name (exactly one role kernel, or none and the one-wave fallback), the rand() position, and the launch's WHOLE buffer --
every frame with its padding, the other field's rows, the guards between the frames -- byte for byte against
TocompOracleStream in MEMORY mode (tolerance zero; the only exclusion is last_row_margin_mask's, empty on padded rows).
A hand-off between two roles that timed out is reported by the NEXT call on the context (NTSCSIM_E_HIP): every row makes
one -- the same launch in the throughput form, compared as well, which also tells an arithmetic difference (both forms) from
one of the hand-offs or trip counts (the role form alone).  tests/test_pipe422_forms_host.py shows on the CPU what the rows
cover.  The synchronous entry point, ntscsim_field422(), runs each form below its steady threshold, at it and at full width.
"""
import numpy as np
import pytest

import _libs as L
import _pipe422_forms as T
import ntscsim
import test_host422 as H

pytestmark = pytest.mark.gpu

ONE_WAVE_PREFIXES = ("k422_fused", "k422_process", "k422_direct")


def planes(whole, k, row, layout):
    """frame k of a launch's device buffer: three views with the host frame's linesizes"""
    f = T.frame_at(np.empty(0, np.uint8), 0, row.w, row.h, layout)
    base = k * T.frame_bytes(row.w, row.h, layout)
    return [whole[base + f.off[i]:base + f.off[i] + f.ls[i] * row.h].view(row.h, f.ls[i]) for i in range(3)]


def launch(torch, sim, row, c, latency):
    """the row's launch on a fresh copy of its buffer: (bytes after, kernel names, rand() position, sources after)"""
    whole = torch.from_numpy(c.init.copy()).cuda()
    src = torch.from_numpy(c.srcbuf.copy()).cuda() if c.srcbuf is not None else None
    jobs = []
    for fi, si, field, fieldno, flags in c.jobs:
        j = {"dst": planes(whole, fi, row, row.layout), "field": field, "fieldno": fieldno, "flags": flags}
        if si is not None:
            j["src"], j["src_height"] = planes(src, si, row, "padded"), row.h
        jobs.append(j)
    sim.set_launch_form(latency)
    sim.rng_pos = 0
    sim.fields422(jobs, row.w, row.h)            # (raises with the context's error text unless NTSCSIM_OK)
    sim.sync()
    return whole.cpu().numpy(), sim.last_kernels(), sim.rng_pos, (src.cpu().numpy() if src is not None else None)


def differing(got, c):
    bad = (got != c.exp) & c.mask
    return "equal" if not bad.any() else "%d bytes differ, first at %d" % (int(bad.sum()), int(np.argmax(bad)))


@pytest.mark.parametrize("row", T.ROWS, ids=lambda r: r.id)
def test_role_form_equals_the_oracle(row):
    import torch
    c = T.case(row.id)
    sim = ntscsim.FieldSimulator(params=T.params(row))
    try:
        got, ran, pos, src = launch(torch, sim, row, c, True)
        # the further call on the same context: NTSCSIM_OK, or the role kernel's hand-off timed out
        got1, ran1, pos1, src1 = launch(torch, sim, row, c, False)
    finally:
        sim.close()
    roles = [k for k in ran if "pipe" in k]
    assert roles == ([row.kernel] if row.kernel else []), ran
    one = [k for k in ran if k.startswith(ONE_WAVE_PREFIXES) and "pipe" not in k]
    assert one == ([row.fallback] if row.fallback else []), ran
    assert ("k422_render" in ran) == (row.source != "inplace"), ran
    assert not any("pipe" in k for k in ran1) and sum(k.startswith(ONE_WAVE_PREFIXES) for k in ran1) == 1, ran1
    assert pos == c.rng_pos and pos1 == c.rng_pos, (pos, pos1, c.rng_pos)
    role, wave = differing(got, c), differing(got1, c)
    assert role == "equal", "%s: %s; the one-wave form %s: %s" % (ran, role, ran1, wave)
    assert wave == "equal", "%s: %s" % (ran1, wave)
    if c.srcbuf is not None:
        assert np.array_equal(src, c.srcbuf) and np.array_equal(src1, c.srcbuf)


def test_every_role_name_was_asked_for():
    """(the names are asserted row by row above; this is the table's side of "each of the eight runs by name")"""
    assert {r.kernel for r in T.ROWS if r.kernel} == set(T.ROLE_NAMES) == {s.kernel for s in T.SYNC}
    assert len(T.ROLE_NAMES) == 8 and all(r.fallback for r in T.ROWS if not r.kernel)


# ------------------------------------------------------------------------------------------------ ntscsim_field422()
def host_frame(w, h, seed):
    """a host frame with the aligned, padded rows of the table, noise in every byte that is no pixel"""
    buf = np.empty(T.frame_bytes(w, h, "padded"), np.uint8)
    f = T.frame_at(buf, 0, w, h, "padded")
    T.fill(buf, [f], seed)
    return f


@pytest.mark.parametrize("row", T.SYNC, ids=lambda r: r.id)
def test_synchronous_call_takes_the_role_form_at_the_widths_of_its_loops(row):
    """ntscsim_field422() call after call on ONE context: two iterations at the row's geometry, one at another, two more at
    the row's -- the setup the previous call ran ahead for the next one (speculate_setup) is used, thrown away and used
    again.  The form by name at every call; persistent frames and encoder frames == the oracle's loop, whole buffers."""
    p = L.make_params_tocomp(row.flags)
    geoms = [(row.w, row.h), T.SYNC_OTHER]
    frames_o = [host_frame(w, h, 11 + w) for w, h in geoms]
    frames_g = [f.copy() for f in frames_o]
    o = L.TocompOracleStream(p, oob=L.OOB_PLANE)
    ctx = H.Ctx(p)
    try:
        for vf, gi in enumerate((0, 0, 1, 0, 0)):
            w, h = geoms[gi]
            field = (vf & 1) ^ 1
            s = host_frame(w, h, 100 + vf)
            s_keep = s.buf.copy()
            eo, go = H.enc_frame(w, h, H.OUT_BOB422, fill=7), H.enc_frame(w, h, H.OUT_BOB422, fill=7)
            H.oracle_iteration(o, p, frames_o[gi], s, field, vf, 0, None, eo, H.OUT_BOB422, field)
            ctx.field(ctx.loop(frames_g[gi], s, field, vf, 0, None, go, H.OUT_BOB422, field, sh=h))
            kern = ctx.last_kernels()
            assert [k for k in kern if "pipe" in k] == [row.kernel], (vf, kern)
            H.same_frames(frames_g[gi], frames_o[gi], "frame %dx%d, iteration %d" % (w, h, vf))
            H.same_out(go, eo, h, H.OUT_BOB422, "encoder frame %d" % vf)
            assert np.array_equal(go.buf, eo.buf), vf                 # (the encoder frame's slack as well)
            assert np.array_equal(s.buf, s_keep), vf
            assert ctx.rng_pos == o.rng_pos, vf
        # a hand-off of the LAST iteration that timed out is reported by the call after it (ctx.field asserts NTSCSIM_OK):
        # one more call, which renders and processes nothing and must leave frame and rand() position as they are
        w, h = geoms[0]
        ctx.field(ctx.loop(frames_g[0], None, 1, 5, H.F_NOCOMP, None, None, H.OUT_BOB422, 1))
        H.same_frames(frames_g[0], frames_o[0], "frame %dx%d after the closing call" % (w, h))
        assert ctx.rng_pos == o.rng_pos
    finally:
        ctx.close()
