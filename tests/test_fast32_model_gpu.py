"""NTSCSIM_MODE_FAST32 against the bit-exact model of its arithmetic (oracle/ntsc_modes_oracle.c, flavour fast32: the exact
chain with float where the kernels say RT -- colour matrices, rotation, filter states with poles fmaf(a, s - p, p) -- and
every quantisation kept).  The translation units of these kernels are compiled with contraction off, so this is IEEE
arithmetic that the CPU reproduces: EQUALITY, byte for byte, and the int32 composite plane equal to the model's
composite_y tap.  Forms, each asserted by name: the hand-tuned batch kernels, the role kernels behind ntscsim_field(), and
the generic kernels that unaligned rows select.
"""
import numpy as np
import pytest

import _libs as L
import _modes as M
import ntscsim
from _modes_gpu import FILL, check_equal_fast32
from _modes_gpu import launch as _launch
from _modes_gpu import model as _model
from ntscsim import _capi

pytestmark = pytest.mark.gpu

FLAGS = {
    "default": [],
    "vhs_sp": ["-vhs"],
    "vhs_lp": ["-vhs", "-vhs-speed", "lp"],
    "vhs_ep": ["-vhs", "-vhs-speed", "ep"],
    "vhs_svideo": ["-vhs", "-vhs-svideo", "1"],
    "vhs_phase90": ["-vhs", "-comp-phase", "90"],
    "vhs_catv3": ["-vhs", "-comp-catv3"],
}
# the small widths of the FLOAT cases (both sides of the steady loops of every form) and one 256x100
SIZES = [(16, 10, 4), (28, 10, 4), (36, 10, 4), (40, 10, 4), (44, 10, 4), (68, 10, 4), (256, 100, 2)]
PRESET = ("default", "vhs_sp", "vhs_lp", "vhs_ep")


def _no_double(kern):
    sig = [k for k in kern if k.startswith(("k_encode", "k_decode", "k_vcr", "k_field_pipe"))]
    assert sig and all("float" in k for k in sig) and not any("double" in k for k in kern), kern
    return sig


@pytest.mark.parametrize("w,h,n", SIZES, ids=["%dx%d" % s[:2] for s in SIZES])
@pytest.mark.parametrize("fl", list(FLAGS))
def test_fast32_batch_equals_its_model(fl, w, h, n):
    p = L.make_params(FLAGS[fl])
    srcs = M.sources("mixed", w, h)
    jobs = M.jobs(n, len(srcs))
    sim = ntscsim.FieldSimulator(params=p)
    sim.set_mode(_capi.MODE_FAST32)
    got, kern, comp = _launch(sim, srcs, jobs, h, w, 0, 0)
    rng_pos = sim.rng_pos
    sim.close()
    _no_double(kern)
    if fl in PRESET:
        assert "k_encode_fast<float>" in kern, kern
        assert ("k_decode_fast<true,float>" if fl != "default" else "k_decode_fast<false,float>") in kern, kern
    pos, outs, frames = _model("fast32", p, srcs, jobs, h, w, 0, 0, taps=["composite_y"])
    assert rng_pos == pos
    check_equal_fast32(got, comp, outs, frames, jobs, "%s %dx%d" % (fl, w, h))


@pytest.mark.parametrize("fl", list(FLAGS))
def test_fast32_generic_forms_on_unaligned_rows_equal_the_model(fl):
    """33x17: rows of 132 bytes are not 16-byte aligned, which selects the generic kernels"""
    w, h, n = 33, 17, 4
    p = L.make_params(FLAGS[fl])
    srcs = M.sources("mixed", w, h)
    jobs = M.jobs(n, len(srcs))
    sim = ntscsim.FieldSimulator(params=p)
    sim.set_mode(_capi.MODE_FAST32)
    got, kern, comp = _launch(sim, srcs, jobs, h, w, 0, 0)
    rng_pos = sim.rng_pos
    sim.close()
    sig = _no_double(kern)
    assert any(k.startswith("k_encode<") for k in sig) and any(k.startswith("k_decode<") for k in sig), kern
    pos, outs, frames = _model("fast32", p, srcs, jobs, h, w, 0, 0, taps=["composite_y"])
    assert rng_pos == pos
    check_equal_fast32(got, comp, outs, frames, jobs, "%s 33x17" % fl)


@pytest.mark.parametrize("w,h", [s[:2] for s in SIZES], ids=["%dx%d" % s[:2] for s in SIZES])
@pytest.mark.parametrize("fl", ["vhs_sp", "vhs_lp", "vhs_ep"])
def test_fast32_host_call_role_kernels_equal_the_model(fl, w, h):
    """ntscsim_field(): the chain as wavefront roles of one workgroup, k_field_pipe<float>"""
    n = 4
    p = L.make_params(FLAGS[fl])
    srcs = M.sources("mixed", w, h)
    jobs = M.jobs(n, len(srcs))
    pos, outs, frames = _model("fast32", p, srcs, jobs, h, w, 0, 0, taps=["composite_y"])
    sim = ntscsim.FieldSimulator(params=p)
    sim.set_mode(_capi.MODE_FAST32)
    got = np.full((n, h, w, 4), FILL, np.uint8)
    for k, (si, field, fieldno) in enumerate(jobs):
        sim.field_host(got[k], srcs[si], field, fieldno)
        assert "k_field_pipe<float>" in sim.last_kernels(), sim.last_kernels()
    assert sim.rng_pos == pos
    sim.close()
    check_equal_fast32(got, None, outs, frames, jobs, "%s %dx%d ntscsim_field" % (fl, w, h))
