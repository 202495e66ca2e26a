"""NTSCSIM_MODE_FAST32, every kernel form by name, against the bit-exact model of its arithmetic (flavour fast32 of
oracle/ntsc_modes_oracle.c: the exact chain with float where the kernels say RT, poles fmaf(a, s - p, p), every quantisation
kept).  tests/_fast32_forms.py is the table: per row a switch set, a geometry, how the form is reached and the names
ntscsim_debug_last_kernels() must report; tests/test_fast32_forms_host.py shows on the CPU that the table names every float
form the launcher can pick.

Tolerance: zero.  These translation units are built with contraction off and the model writes every fused operation out,
so bytes, the int32 composite plane (where the row says the exposed plane is the model's tap) and the rand() position are
EQUAL -- kernel forms of one switch set are one function.

  * batch path: one ntscsim_fields_device() call per row in MODE_FAST32;
  * the same rows in MODE_FLOAT: either the all-float kernels run (the dispatcher's rule, restated in the table, says for
    which rows: those belong to tests/test_float_model_gpu.py and end there) or names and bytes are the FAST32 row's;
  * role kernels: ntscsim_field() call after call on one rand() stream, and device-resident launches in the latency form.
"""
import functools

import numpy as np
import pytest

import _fast32_forms as F
import _modes as M
import ntscsim
from _modes_gpu import FILL, check_equal_fast32, is_fp, launch, model
from ntscsim import _capi

pytestmark = pytest.mark.gpu

CHAIN = ("k_encode", "k_ghost", "k_vcr", "k_decode")


@functools.lru_cache(maxsize=2)
def _expected(rid):
    """the model's side of a batch row, computed once for the FAST32 and the FLOAT test of the row (read only)"""
    r = F.BY_ID[rid]
    p = F.params(r.flags, r.ghost)
    srcs = M.sources(r.kind, r.w, r.h)
    jobs = M.jobs(r.n, len(srcs))
    pos, outs, frames = model("fast32", p, srcs, jobs, r.h, r.w, r.il, r.tff, taps=["composite_y"])
    return p, srcs, jobs, pos, outs, frames


def _run(r, mode):
    p, srcs, jobs, pos, outs, frames = _expected(r.id)
    sim = ntscsim.FieldSimulator(params=p)
    try:
        sim.set_mode(mode)
        if r.mode == F.GEN:
            sim.debug_force_generic(True)
        elif F.DEBUG_BITS[r.mode]:
            sim.debug_no_fast_decode(F.DEBUG_BITS[r.mode])
        got, kern, comp = launch(sim, srcs, jobs, r.h, r.w, r.il, r.tff)
        rng_pos = sim.rng_pos
    finally:
        sim.close()
    return got, kern, comp, rng_pos


def _check_row(r, got, kern, comp, rng_pos):
    p, srcs, jobs, pos, outs, frames = _expected(r.id)
    assert [k for k in kern if k.startswith(CHAIN)] == r.names, kern
    assert not any("double" in k or k.startswith("k_field_pipe") for k in kern), kern
    assert rng_pos == pos
    check_equal_fast32(got, comp if r.plane else None, outs, frames, jobs, r.id)


# (the mode varies fastest: both tests of a row are neighbours and share the row's model through the two-entry cache)
@pytest.mark.parametrize("r", F.ROWS, ids=lambda r: r.id)
@pytest.mark.parametrize("mode", ["fast32", "float"])
def test_batch_form_equals_the_model(mode, r):
    """fast32: the row's names, rand() position, bytes (the fill in the other field's rows included) and composite plane.

    float: NTSCSIM_MODE_FLOAT, "anything else runs the FAST32 forms" -- which rows the all-float kernels take is the
    dispatcher's rule (F.float_forms_take; tests/test_fast32_forms_host.py pins their number): those rows belong to
    tests/test_float_model_gpu.py, which holds them to real64, and end here; every other row reports the FAST32 row's
    names and produces its bytes."""
    if mode == "fast32":
        _check_row(r, *_run(r, _capi.MODE_FAST32))
        return
    got, kern, comp, rng_pos = _run(r, _capi.MODE_FLOAT)
    fp = is_fp(kern)
    assert bool(fp) == F.float_forms_take(r, _expected(r.id)[0]), kern
    if fp:
        assert fp[0] == "k_encode_fp" and len(fp) == 2, kern
        return
    _check_row(r, got, kern, comp, rng_pos)


# ------------------------------------------------------------------------------------------------ role kernels
def _host_calls(role, n=4):
    p = F.params(role.flags)
    srcs = M.sources("mixed", role.w, role.h)
    jobs = M.jobs(n, len(srcs))
    pos, outs, frames = model("fast32", p, srcs, jobs, role.h, role.w, 0, 0, taps=["composite_y"])
    sim = ntscsim.FieldSimulator(params=p)
    try:
        sim.set_mode(_capi.MODE_FAST32)
        got = np.full((n, role.h, role.w, 4), FILL, np.uint8)
        for k, (si, field, fieldno) in enumerate(jobs):
            sim.field_host(got[k], srcs[si], field, fieldno)
            kern = sim.last_kernels()
            assert [x for x in kern if x.startswith("k_field_pipe")] == ([role.name] if role.name else []), kern
            assert not any("double" in x for x in kern), kern
            if not role.name:
                chain = [x for x in kern if x.startswith(CHAIN)]
                assert chain and all("float" in x for x in chain if x != "k_ghost"), kern
        assert sim.rng_pos == pos
    finally:
        sim.close()
    check_equal_fast32(got, None, outs, frames, jobs, "%s ntscsim_field" % role.id)


@pytest.mark.parametrize("role", F.ROLES, ids=lambda r: r.id)
def test_fast32_role_kernel_equals_the_model(role):
    """ntscsim_field(): the chain as wavefront roles of one workgroup, each float instantiation by name"""
    _host_calls(role)


@pytest.mark.parametrize("role", F.NO_ROLE, ids=lambda r: r.id)
def test_fast32_switch_sets_outside_the_role_kernels_equal_the_model(role):
    _host_calls(role)


@pytest.mark.parametrize("n,w,h", F.LATENCY_SIZES, ids=["%dx%dx%d" % s for s in F.LATENCY_SIZES])
@pytest.mark.parametrize("flags,name", F.LATENCY, ids=[x[1] for x in F.LATENCY])
def test_fast32_latency_form_equals_the_throughput_form_and_the_model(flags, name, n, w, h):
    """ntscsim_set_launch_form(NTSCSIM_FORM_LATENCY): device-resident launches of up to 64 fields as wavefront roles"""
    p = F.params(flags)
    srcs = M.sources("mixed", w, h)
    jobs = M.jobs(n, len(srcs))
    pos, outs, frames = model("fast32", p, srcs, jobs, h, w, 0, 0, taps=["composite_y"])
    res = []
    for latency in (True, False):
        sim = ntscsim.FieldSimulator(params=p)
        try:
            sim.set_mode(_capi.MODE_FAST32)
            if latency:
                sim.set_launch_form(True)
            got, kern, comp = launch(sim, srcs, jobs, h, w, 0, 0)
            assert [x for x in kern if x.startswith("k_field_pipe")] == ([name] if latency else []), kern
            assert not any("double" in x for x in kern), kern
            assert sim.rng_pos == pos
        finally:
            sim.close()
        res.append(got)
    assert np.array_equal(res[0], res[1])
    check_equal_fast32(res[0], None, outs, frames, jobs, "%s latency form, %d fields" % (name, n))
    check_equal_fast32(res[1], None, outs, frames, jobs, "%s throughput form, %d fields" % (name, n))
