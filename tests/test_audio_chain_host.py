"""The plan of csrc/audio_chain.hpp -- segments that start one warm-up early from a zero state, then verify and repair --
on the host: tests/audio_chain_check.cpp, a stand-alone program with its own main, is built plain and with the address and
undefined-behaviour sanitizers and run as the program it is.  Planned runs must equal the serial run byte for byte and
state for state for L in {1, 63, 64, 1000} and W in {0, 1, 64, default}, over calls of 0, 1, 777, 64 and the remaining
frames; with W = 0 on input that is not silent every segment but a call's first is repaired.

test_convergence_stays_under_the_default_warmup re-measures what DESIGN.md 7l records: from 24 start points per fixture
input, the frames a zero-state run needs until every filter state is bit-identical to the true trajectory.  It asserts
that the worst stays under the default warm-up (72 tau), which is what makes `repaired == 0` in tests/test_audio_gpu.py a
property of these inputs, and prints the worst."""
import re

import pytest

import _audio_ref as A
from ntscsim import _capi

PLANNED = ["hifi_default", "hifi_noemph_clip", "linear_sp", "linear_lp_emph", "linear_pal", "hiss_off_silence", "hiss_full", "nocomp"]
LONG = ["hifi_default_long", "hifi_noemph_long", "linear_sp_long", "linear_ep_long"]


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("name", PLANNED)
def test_planned_runs_equal_the_serial_run(name, build):
    flags, kind, _frames, _seed, count0, rng0, _block, _swap = A.CASES[name]
    ap, _ = _capi.make_audio_params(flags)
    rc, out = A.run_checker_mode("planned", ap, A.case_input(name), count0, rng0, int(kind != "silence"), build=build)
    assert rc == 0 and "16 runs, 0 bad" in out, out


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_serial_run_under_the_sanitizers_equals_the_fixture(build):
    meta, _ = A.fixture()
    for name in ("linear_sp_count_2p31", "hifi_default_b1601"):
        m = meta[name]
        ap, _ = _capi.make_audio_params(m["flags"])
        out, _state, pos = A.run_checker(ap, A.case_input(name), m["count0"], m["rng0"], m["block"], build=build)
        assert A.sha(out) == m["sha256"] and pos == m["rng_after"]


@pytest.mark.parametrize("name", LONG)
def test_convergence_stays_under_the_default_warmup(name):
    flags, _kind, _frames, _seed, count0, rng0, _block, _swap = A.CASES[name]
    ap, _ = _capi.make_audio_params(flags)
    rc, out = A.run_checker_mode("converge", ap, A.case_input(name), count0, rng0)
    print(out)
    m = re.search(r"converge: (\d+) starts, (\d+) unmet, worst (\d+) default_warmup (\d+)", out)
    assert m, out
    starts, unmet, worst, warmup = (int(g) for g in m.groups())
    assert rc == 0 and starts >= 8 and unmet == 0 and worst <= warmup
    assert warmup == (25280 if ap.highpass_hz == 20 else 5056)
