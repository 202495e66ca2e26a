"""The checker tests/_avg_ref.py against the fixtures generated from the reference's own composite_layer()
(tests/golden/make_golden_avgdelay.py; AVFrame / InputFile / delay stand-ins: unpinned).  No GPU.  Every byte of every
output frame must agree."""
import os

import numpy as np
import pytest

import _avg_ref as R

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avgdelay_golden.npz"))
CASES = sorted(k[4:-5] for k in GOLD.files if k.endswith("_geom"))


def case(name):
    w, h, delay, T, nl, field0 = (int(v) for v in GOLD["avg_%s_geom" % name])
    levels = [int(v) for v in GOLD["avg_%s_levels" % name]]
    present = GOLD["avg_%s_present" % name]
    src = GOLD["avg_%s_src" % name]
    frames = [[src[t, l] if present[t, l] else None for l in range(nl)] for t in range(T)]
    return w, h, delay, T, levels, field0, frames, GOLD["avg_%s_out" % name]


def test_the_fixture_file_has_the_cases_the_tests_rely_on():
    assert CASES == sorted(["levels", "levels_wrap", "ring_d1", "ring_d2", "ring_d3_absent", "field_big"])
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "avgdelay_golden.npz")) < 150976


@pytest.mark.parametrize("name", CASES)
def test_checker_equals_reference_fixture(name):
    w, h, delay, T, levels, field0, frames, want = case(name)
    ring = [np.zeros((h, w, 4), np.uint8) for _ in range(delay)]
    got, ri, field = R.avg_clip(ring, frames, levels, 0, field0)
    assert (ri, field) == (T % delay, field0 + T)
    assert got.shape == want.shape
    assert int((got != want).sum()) == 0
    for i in range(delay):                                                        # the ring holds the last frame of each slot
        last = max(t for t in range(T) if t % delay == i)
        assert int((ring[i] != want[last]).sum()) == 0


@pytest.mark.parametrize("name", ["levels", "levels_wrap", "field_big"])
def test_scalar_form_of_the_checker_equals_the_fixture(name):
    w, h, delay, T, levels, field0, frames, want = case(name)
    ring = [np.zeros((h, w, 4), np.uint8) for _ in range(delay)]
    for t in range(T):
        R.avg_frame(ring[t % delay], frames[t], levels, field0 + t, delay, scalar=True)
        assert int((ring[t % delay] != want[t]).sum()) == 0


def test_fixtures_show_what_they_are_there_for():
    """Levels 0 .. 256 leave the top byte 0; the wrapping levels do not; an all-absent frame repeats slot content."""
    assert int(GOLD["avg_levels_out"][:, :, :, 3].max()) == 0
    assert int(GOLD["avg_levels_wrap_out"][:, :, :, 3].max()) > 0
    out, pres = GOLD["avg_ring_d3_absent_out"], GOLD["avg_ring_d3_absent_present"]
    idle = [t for t in range(len(pres)) if not pres[t].any()]
    assert idle and all(t >= 3 for t in idle)
    for t in idle:
        assert int((out[t] != out[t - 3]).sum()) == 0 and int(out[t, :, :, 3].max()) > 0
