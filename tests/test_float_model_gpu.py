"""NTSCSIM_MODE_FLOAT against the model of its own arithmetic (oracle/ntsc_modes_oracle.c, flavour real64: the chain with
every inter-stage truncation removed, evaluated in fp64 -- DESIGN.md 3b).

tests/test_gpu_fast_mode.py compares this mode with the TRUNCATING oracle, which differs from it by design: +-1 LSB of the
output, i.e. +-256 units of the filtered signal.  Here the reference computes the same operation, so the tolerance is the
evaluation noise of fp32 alone, measured on the CPU from the model (tools/float_model_err.py, profiles/float_model_err.txt:
real32 against real64 over exactly these cases) and never from the kernels:

    DELTA_OUT  = 4 x the largest difference of a channel value in front of the final truncation  [output LSB]
    DELTA_COMP = 4 x the largest difference of a composite sample                                [1/256 of a step]

(4 x: the kernels sum the separators' boxes as pair sums and contract differently from any one CPU ordering -- other
roundings of the same size, whose signs must not be a matter of luck.)  Ceilings that are no measurements: DELTA_OUT <= 1/16
LSB, DELTA_COMP <= 0.25.

Per case: the kernel forms by name, the rand() position, the encoder's float plane against the model's composite tap on
every row of every field, and every channel of every written pixel in {q(v - DELTA_OUT), q(v + DELTA_OUT)},
q(x) = clamp(trunc(x), 0, 255); alpha 0; the other field's rows untouched.

Which decoder a case runs is decided by its number of fields: launches of up to 128 fields of the -vhs family take the
two-role workgroup k_decode_fp2 (loops vcr_steady and the TV role's), longer ones the one-wave form k_decode_fp<true>
(loop steady()); the default preset always takes k_decode_fp<false>.  The three have different entry conditions, and
tests/_modes.py (FLOAT_CASES) places widths below, at and above EACH of them and says which form every width is for.
"""
import numpy as np
import pytest

import _libs as L
import _modes as M
import ntscsim
from _modes_gpu import check_equal_fast32, check_float_fields, is_fp, launch, model
from ntscsim import _capi

pytestmark = pytest.mark.gpu

# profiles/float_model_err.txt: overall max|dv| = 0.000223 LSB, overall max|dcomp| = 0.015662 units
DELTA_OUT = 4 * 0.000223           # 0.000892 LSB = 0.23 units of the 256-scaled signal
DELTA_COMP = 4 * 0.015662          # 0.0626 units
assert DELTA_OUT <= 1.0 / 16 and DELTA_COMP <= 0.25


def _check(got, comp, outs, jobs, what):
    check_float_fields(got, comp.view(np.float32), outs, jobs, what, DELTA_OUT, DELTA_COMP)


def expected_decoder(p, n):
    """launch_decode_fp()'s rule (csrc/ntsc_float.hip)"""
    if not p.emulating_vhs:
        return "k_decode_fp<false>"
    return "k_decode_fp2" if n <= 128 else "k_decode_fp<true>"


@pytest.mark.parametrize("case", M.FLOAT_CASES, ids=[c[0] for c in M.FLOAT_CASES])
def test_float_mode_against_its_model(case):
    name, flags, w, h, n, kind, form, extra = case
    il, tff = extra.get("interlaced", 0), extra.get("tff", 0)
    p = L.make_params(flags)
    srcs = M.sources(kind, w, h)
    jobs = M.jobs(n, len(srcs))
    sim = ntscsim.FieldSimulator(params=p)
    sim.set_mode(_capi.MODE_FLOAT)
    if form == "refused":
        with pytest.raises(ntscsim.NtscsimError) as e:
            launch(sim, srcs, jobs, h, w, il, tff)
        assert e.value.code == _capi.E_SIZE and sim.rng_pos == 0, e.value
        sim.close()
        return
    got, kern, comp = launch(sim, srcs, jobs, h, w, il, tff, extra.get("pad", 0))
    rng_pos = sim.rng_pos
    sim.close()
    if form == "fp":
        dec = expected_decoder(p, n)
        assert extra.get("decoder", dec) == dec                 # (the case list says which form it is for)
        assert "k_encode_fp" in kern and dec in kern, kern
        pos, outs, _ = model("real64", p, srcs, jobs, h, w, il, tff)
        assert rng_pos == pos
        _check(got, comp, outs, jobs, name)
    else:
        # outside the float forms (geometry or switch set): the FAST32 kernels, which the fast32 flavour states bit for bit
        assert not is_fp(kern), kern
        pos, outs, frames = model("fast32", p, srcs, jobs, h, w, il, tff, taps=["composite_y"])
        assert rng_pos == pos
        check_equal_fast32(got, comp, outs, frames, jobs, name)


def test_float_saturating_cases_hit_both_clamps():
    """(a property of the test's own inputs: the saturating frames do reach both ends of the byte range in the model)"""
    for name, flags, w, h, n, kind, form, extra in [c for c in M.FLOAT_CASES if c[5] == "saturating"]:
        p = L.make_params(flags)
        srcs = M.sources(kind, w, h)
        _, outs, _ = model("real64", p, srcs, M.jobs(n, len(srcs)), h, w, 0, 0)
        v = np.concatenate([o["v"].ravel() for o in outs])
        assert v.min() < -1 and v.max() > 256, (name, v.min(), v.max())


def test_float_long_batch_one_wave_form_and_two_role_form_against_the_model():
    """130 fields of 40x18 in one launch: k_decode_fp<true> (one wave per 63 rows), checked against real64 directly; the
    same 130 jobs in launches of <= 128: k_decode_fp2, same check"""
    name, flags, w, h, n, kind = M.LONG_BATCH
    p = L.make_params(flags)
    srcs = M.sources(kind, w, h)
    jobs = M.jobs(n, len(srcs))
    pos, outs, _ = model("real64", p, srcs, jobs, h, w, 0, 0)
    sim = ntscsim.FieldSimulator(params=p)
    sim.set_mode(_capi.MODE_FLOAT)
    got, kern, comp = launch(sim, srcs, jobs, h, w, 0, 0)
    assert "k_encode_fp" in kern and "k_decode_fp<true>" in kern, kern
    assert sim.rng_pos == pos
    _check(got, comp, outs, jobs, "one launch of 130")
    sim.rng_pos = 0
    for lo in range(0, n, 65):
        part = jobs[lo:lo + 65]
        got, kern, comp = launch(sim, srcs, part, h, w, 0, 0)
        assert "k_encode_fp" in kern and "k_decode_fp2" in kern, kern
        _check(got, comp, outs[lo:lo + 65], part, "launch of fields %d.." % lo)
    assert sim.rng_pos == pos
    sim.close()
