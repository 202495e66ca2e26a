"""Every sweep form of the YUV422P tool -- k422_process (csrc/ntsc422_kernels.hip), k422_fused<false,false,4>,
k422_fused<true,false,4> and k422_direct (csrc/ntsc422_fused.hip) -- against the oracle, row by row of
tests/_sweep422_forms.py: ONE ntscsim_fields422_device() launch in the throughput form per row on fresh device buffers, the
kernel asserted by name, the rand() position, and the launch's WHOLE buffer -- every frame with its padding, the other
field's rows, the bytes between the planes, the guards between and behind the frames -- byte for byte against
TocompOracleStream in MEMORY mode (tolerance zero: integer bytes, fp64 filters in the reference's order, contraction off;
the only exclusion is last_row_margin_mask's, empty unless the rows are tight).  Sources and filter frames are compared
whole as well.  Every row makes a second call on its context, which must return NTSCSIM_OK: the same launch in ANOTHER
form of the same switch set -- the dispatcher's own choice (the streamed forms, k422_direct_fast) where a debug bit reached
the row's form, the twelve sweeps otherwise -- whose buffer must equal the oracle's and so the first one's.  The rows of a
test that share a switch set share a context.  Per mixed row one
ntscsim_mixed_fields422_device() call over ten sets.  tests/test_sweep422_forms_host.py shows on the CPU what the rows cover.
"""
import numpy as np
import pytest

import _libs as L          # (puts the package on the path)
import _pipe422_forms as T
import _sweep422_forms as S
import ntscsim

pytestmark = pytest.mark.gpu

ONE_WAVE_PREFIXES = ("k422_fused", "k422_process", "k422_direct")


def planes(whole, k, w, h, layout):
    """frame k of a launch's device buffer: three views with the host frame's linesizes"""
    f = T.frame_at(np.empty(0, np.uint8), 0, w, h, layout)
    base = k * T.frame_bytes(w, h, layout)
    return [whole[base + f.off[i]:base + f.off[i] + f.ls[i] * h].view(h, f.ls[i]) for i in range(3)]


def launch(torch, sim, row, c, bits):
    """the row's launch on a fresh copy of its buffers: (bytes after, kernel names, rand() position, sources after, filter
    frames after)"""
    whole = torch.from_numpy(c.init.copy()).cuda()
    src = torch.from_numpy(c.srcbuf.copy()).cuda() if c.srcbuf is not None else None
    flt = torch.from_numpy(c.fltinit.copy()).cuda() if c.fltinit is not None else None
    jobs = []
    for fi, si, field, fieldno, flags in c.jobs:
        j = {"dst": planes(whole, fi, row.w, row.h, row.layout), "field": field, "fieldno": fieldno, "flags": flags}
        if si is not None:
            j["src"], j["src_height"] = planes(src, si, row.w, row.h, "padded"), row.h
        if flt is not None:
            j["flt"] = planes(flt, fi, row.w, row.h, "padded")
        jobs.append(j)
    sim.debug_no_fast_decode(bits)
    sim.rng_pos = 0
    sim.fields422(jobs, row.w, row.h)            # (raises with the context's error text unless NTSCSIM_OK)
    sim.sync()
    return (whole.cpu().numpy(), sim.last_kernels(), sim.rng_pos, src.cpu().numpy() if src is not None else None,
            flt.cpu().numpy() if flt is not None else None)


def differing(got, exp, mask=None):
    bad = got != exp
    if mask is not None:
        bad &= mask
    return "equal" if not bad.any() else "%d bytes differ, first at %d" % (int(bad.sum()), int(np.argmax(bad)))


def check_row(torch, sim, row):
    c = S.case(row.id)
    got, ran, pos, src, flt = launch(torch, sim, row, c, row.bits)
    other = S.companion_bits(row)
    got1, ran1, pos1, src1, flt1 = launch(torch, sim, row, c, other)
    one = [k for k in ran if k.startswith(ONE_WAVE_PREFIXES) or "pipe" in k]
    assert one == [row.kernel], (row.id, ran)
    assert ("k422_render" in ran) == (c.srcbuf is not None) and ("k422_bkey" in ran) == (c.fltinit is not None), (row.id, ran)
    one1 = [k for k in ran1 if k.startswith(ONE_WAVE_PREFIXES) or "pipe" in k]
    want1 = S.launcher_rule(S.params(row), *S.alignment(row.w, row.h, row.layout), other)
    assert one1 == [want1], (row.id, ran1)
    assert pos == c.rng_pos and pos1 == c.rng_pos, (row.id, pos, pos1, c.rng_pos)
    mine, its = differing(got, c.exp, c.mask), differing(got1, c.exp, c.mask)
    assert mine == "equal", "%s %s: %s; %s: %s" % (row.id, ran, mine, ran1, its)
    assert its == "equal", "%s %s: %s" % (row.id, ran1, its)
    # (where nothing is excluded the two forms' buffers are each other's; on tight rows the margin of the last row is
    #  defined by neither)
    assert differing(got, got1, c.mask) == "equal", row.id
    if c.srcbuf is not None:
        assert np.array_equal(src, c.srcbuf) and np.array_equal(src1, c.srcbuf), row.id
    if c.fltinit is not None:
        assert differing(flt, c.fltexp) == "equal" and differing(flt1, c.fltexp) == "equal", row.id


@pytest.mark.parametrize("group", list(S.GROUPS), ids=str)
def test_sweep_forms_equal_the_oracle(group):
    import torch
    sim, flags = None, None
    try:
        for row in S.GROUPS[group]:
            if sim is None or row.flags != flags:          # (the rows of one switch set follow each other)
                if sim is not None:
                    sim.close()
                sim, flags = ntscsim.FieldSimulator(params=S.params(row)), row.flags
                sim.set_launch_form(False)
            check_row(torch, sim, row)
    finally:
        if sim is not None:
            sim.close()


def test_every_name_was_asked_for():
    """(the names are asserted row by row above; this is the table's side of "each of the four runs by name")"""
    assert {r.kernel for r in S.ROWS} == set(S.FORMS) and len(S.FORMS) == 4
    assert sorted(r.id for rows in S.GROUPS.values() for r in rows) == sorted(r.id for r in S.ROWS)


def check_mixed(torch, m):
    c = S.mixed_case(m.id)
    whole = torch.from_numpy(c.init.copy()).cuda()
    jobs = [{"dst": planes(whole, fi, m.w, m.h, m.layout), "field": field, "fieldno": fieldno, "flags": flags}
            for fi, _, field, fieldno, flags in c.jobs]
    sim = ntscsim.FieldSimulator(params=c.sets[0])
    try:
        sim.rng_pos = 0
        sim.run_mixed_descs422(list(c.sets), sim.build_mixed_descs422(c.set_of, jobs), m.w, m.h)
        names, pos = sim.last_kernels(), sim.rng_pos
        sim.sync()
        got = whole.cpu().numpy()
        # the next call on the context: one plain launch of the first descriptor's set, which must return NTSCSIM_OK
        again = torch.from_numpy(c.init.copy()).cuda()
        sim.fields422([{"dst": planes(again, 0, m.w, m.h, m.layout), "field": c.jobs[0][2], "fieldno": 0, "flags": 0}], m.w, m.h)
        sim.sync()
    finally:
        sim.close()
    halo = 2 * ((m.h + 1) // 2) > S.WG_ROWS
    assert names == ["k_mixed_setup"] + (["k422_mixed_halo"] if halo else []) + [S.MIXED_NAME], (m.id, names)
    assert pos == c.rng_pos, (m.id, pos, c.rng_pos)
    assert differing(got, c.exp, c.mask) == "equal", m.id


@pytest.mark.parametrize("layout", S.MIXED_LAYOUTS)
def test_mixed_calls_equal_the_oracle(layout):
    """ten sets in one call (SP, LP, EP, PAL-VHS, S-Video, default, -yc-recomb 1, nocolor, after-yc-sep, input low-pass
    off), two fields each: k422_mixed_process runs process422_body per set; one call per width of the table"""
    import torch
    rows = [m for m in S.MIXED if m.layout == layout]
    assert len(rows) == len(S.MIXED_W)
    for m in rows:
        check_mixed(torch, m)
