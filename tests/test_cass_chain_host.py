"""The plan of csrc/cass_chain.hpp -- front and back cut into segments that start one warm-up early from a zero state,
the FIR between them with its zero taps left out, verify and repair for both passes -- on the host:
tests/cass_chain_check.cpp, a stand-alone program with its own main, is built plain and with the address and
undefined-behaviour sanitizers and run as the program it is.  Planned runs must equal the serial, every-tap run byte for
byte and state for state (the FIR's history included) for L in {1, 2, 63, 64, 65, 1000} and (front, back) warm-ups of
(0, 0), (1, 64), (64, 1) and the defaults, over calls of 0, 1, 777, 64 and the remaining frames -- with 57 taps the
history spans the short calls; with a warm-up of 0 on input that is not silent every segment but a call's first is
repaired.

test_convergence_stays_under_the_default_warmups measures what DESIGN.md 7m records: from 24 start points per input, the
frames a zero-state run of the front, and of the back, needs until every state is bit-identical to the true trajectory.
The back's default warm-up is derived from that measurement (csrc/cass_chain.hpp: CASS_BACK_MEASURED, the worst case,
plus a fifth, up to a multiple of 64); the test fails if a run needs longer than the recorded worst case."""
import re

import pytest

import _cass_ref as A
from ntscsim import _capi

PLANNED = ["default", "preset3", "headalign_neg", "both", "mono_both_preset1", "clip_both", "hiss_off_silence", "hiss_full", "count_3e9"]
LONG = ["long_20hz", "long_100hz"]
DEEMPHASIS = sorted(n for n, v in A.CASES.items() if "-deemphasis" in v[0])


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("name", PLANNED)
def test_planned_runs_equal_the_serial_run(name, build):
    flags, kind, _frames, _seed, count0, rng0, _block, _swap = A.CASES[name]
    cp = _capi.make_cass_params(flags)
    a = A.case_input(name)
    rc, out = A.run_checker_mode("planned", cp, a, count0, rng0, int(kind != "silence"),
                                 sines=A.recorded_sines(count0, len(a)), build=build)
    assert rc == 0 and "24 runs, 0 bad" in out, out


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_serial_run_under_the_sanitizers_equals_the_fixture(build):
    meta, _ = A.fixture()
    for name in ("count_2p31", "preset3_b1601", "preset3_b3", "mono_both_preset1"):
        m = meta[name]
        cp = _capi.make_cass_params(m["flags"])
        out, _state, pos = A.run_checker(cp, A.case_input(name), m["count0"], m["rng0"], m["block"], sines=A.recorded_sines(m["count0"], m["frames"]),
                                         build=build)
        assert A.sha(out) == m["sha256"] and pos == m["rng_after"]


@pytest.mark.parametrize("name", DEEMPHASIS)
def test_back_convergence_on_every_fixture_input_with_deemphasis(name):
    """52 frames is the worst of these (long_100hz); the short inputs are too short to measure the front on."""
    flags, _kind, _frames, _seed, count0, rng0, _block, _swap = A.CASES[name]
    _rc, out = A.run_checker_mode("converge", _capi.make_cass_params(flags), A.case_input(name), count0, rng0)
    print(out)
    m = re.search(r"back (\d+) starts, (\d+) unmet, worst (\d+) measured (\d+) default_warmup (\d+)", out)
    assert m, out
    starts, unmet, worst, measured, warmup = (int(g) for g in m.groups())
    assert starts >= 8 and unmet == 0 and worst <= measured == 52 and warmup == 64


@pytest.mark.parametrize("name", LONG)
def test_convergence_stays_under_the_default_warmups(name):
    flags, _kind, _frames, _seed, count0, rng0, _block, _swap = A.CASES[name]
    cp = _capi.make_cass_params(flags)
    assert cp.deemphasis
    rc, out = A.run_checker_mode("converge", cp, A.case_input(name), count0, rng0)
    print(out)
    m = re.search(r"converge: front (\d+) starts, (\d+) unmet, worst (\d+) default_warmup (\d+); back (\d+) starts, (\d+) unmet, worst (\d+) "
                  r"measured (\d+) default_warmup (\d+)", out)
    assert m, out
    starts, unmet, worst, warmup, bstarts, bunmet, bworst, measured, bwarmup = (int(g) for g in m.groups())
    assert rc == 0 and starts >= 8 and unmet == 0 and worst <= warmup
    assert warmup == (25280 if cp.highpass_hz == 20 else 5056)
    assert bstarts >= 20 and bunmet == 0 and bworst <= measured
    assert bwarmup == (measured + measured // 5 + 1 + 63) // 64 * 64 and bwarmup >= measured * 6 // 5
