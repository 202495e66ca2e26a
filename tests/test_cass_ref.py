"""csrc/cass_chain.hpp against the reference's own lines.

tests/golden/cass_ref.npz was recorded once from ffmpeg_cassette's composite_audio_process() as the tool contains it: the
lines ffmpeg_cassette.cpp:55-76 (dBFS), :80-209 (the filters), :258-416 (the convolution map and the chain), its globals,
parse_argv() :418-590 and the set-up :864-880 were copied, unchanged, into a scratch program behind libc / STL headers
alone, rand() counted and sin() recorded through macros, compiled with g++ -O2 -ffp-contract=off and run on the inputs of
tests/_audio_ref.py (an integer generator: no libm in it).  No stand-in type was needed, so the runs are pinned in the
sense of DESIGN.md 4.  Only data is kept: per case the switches, the input's SHA-256, the rand() position behind the run,
the output's SHA-256, the SHA-256 of the sin() results, the full output of the one-call runs of up to 2048 frames, and the sin()
results themselves once per count range of those short runs.

The host checker (tests/cass_chain_check.cpp, the header run serially with every tap) must reproduce every recorded run
with head_tilt_final built from the RECORDED sines: that holds on any host.  Whether this host's libm gives the recorded
sines is a separate test; the two long runs have no table and run only where it does."""
import os

import numpy as np
import pytest

import _cass_ref as A
from ntscsim import _capi


def test_fixture_is_small():
    assert os.path.getsize(A.FIXTURE) < 200 * 1024


def test_fixture_holds_the_cases_of_the_helper():
    meta, arrays = A.fixture()
    assert sorted(meta) == sorted(A.CASES)
    for name, m in meta.items():
        flags, kind, frames, seed, count0, rng0, block, swap = A.CASES[name]
        assert (m["flags"], m["kind"], m["frames"], m["seed"], m["count0"], m["rng0"], m["block"], m["swap"]) == \
            (list(flags), kind, frames, seed, count0, rng0, block, swap)
        assert A.sha(A.case_input(name)) == m["input_sha256"], "the input generator changed: %s" % name
        if frames <= A.FULL_OUTPUT_FRAMES:
            if block == 0:                                                      # a run fed in blocks is kept as its hash
                assert A.sha(arrays["out_" + name]) == m["sha256"]
            assert A.sha(A.recorded_sines(count0, frames)) == m["sin_sha256"]
    for c0 in A.SINE_COUNT0:
        assert arrays["sines_%d" % c0].size == 2048


def _local_sines_match(name):
    m = A.fixture()[0][name]
    cp = _capi.make_cass_params(m["flags"])
    return A.sha(A.local_sines(cp, m["count0"], m["frames"])) == m["sin_sha256"]


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_header_equals_the_recorded_run(name):
    meta, arrays = A.fixture()
    m = meta[name]
    cp = _capi.make_cass_params(m["flags"])
    assert (cp.taps, cp.hiss_level) == (m["taps"], m["hiss_level"])
    sines = A.recorded_sines(m["count0"], m["frames"])
    if sines is None and not _local_sines_match(name):
        pytest.skip("no recorded sine table for %d frames, and this host's libm sin() differs from the recorded one" % m["frames"])
    out, _state, pos = A.run_checker(cp, A.case_input(name), m["count0"], m["rng0"], m["block"], sines=sines)
    if "out_" + name in arrays:
        want = arrays["out_" + name]
        bad = int((out != want).sum())
        assert bad == 0, "%d wrong samples, first at %d" % (bad, int(np.argmax((out != want).reshape(-1))))
    assert A.sha(out) == m["sha256"]
    assert pos == m["rng_after"]


@pytest.mark.parametrize("count0", A.SINE_COUNT0)
def test_local_libm_gives_the_recorded_sines(count0):
    """Parity with the tool is parity with the libm of the host that runs it.  glibc 2.35 on x86-64 is
    what the fixture was recorded with."""
    want = A.recorded_sines(count0, 2048)
    got = A.local_sines(_capi.make_cass_params([]), count0, 2048)
    differ = int((got.view(np.uint64) != want.view(np.uint64)).sum())
    assert differ == 0, "%d of 2048 sin() results differ from the recorded ones" % differ


def test_recording_covers_every_kind_of_case():
    meta, arrays = A.fixture()
    cp = {n: _capi.make_cass_params(m["flags"]) for n, m in meta.items()}
    kinds = {
        "default (8 taps)": any(not m["flags"] and cp[n].taps == 8 for n, m in meta.items()),
        "7 taps": any(c.taps == 7 and c.head_tilt == 0 for c in cp.values()),
        "57 taps": any(c.taps == 57 for c in cp.values()),
        "negative tilt": any(c.head_tilt < 0 for c in cp.values()),
        "no waver": any(c.head_tilt_waver == 0 for c in cp.values()),
        "pre only": any(c.preemphasis and not c.deemphasis for c in cp.values()),
        "post only": any(c.deemphasis and not c.preemphasis for c in cp.values()),
        "both": any(c.deemphasis and c.preemphasis for c in cp.values()),
        "mono": any(c.mono for c in cp.values()),
        "count above 2^31": sum(m["count0"] > 1 << 31 for m in meta.values()) >= 2,
        "rand() position not 0": any(m["rng0"] > 0 and cp[n].hiss_level for n, m in meta.items()),
        "long runs at 20 Hz and 100 Hz": any(m["frames"] == 60000 and cp[n].highpass_hz == 20 for n, m in meta.items()) and
        any(m["frames"] == 12000 and cp[n].highpass_hz == 100 for n, m in meta.items()),
        "later switches override": any(m["flags"][:2] == ["-preset", "3"] and cp[n].head_tilt == 2 and cp[n].highpass_hz == 50 for n, m in meta.items()),
    }
    for k in range(5):
        kinds["preset %d" % k] = any(m["flags"] == ["-preset", str(k)] for m in meta.values())
    for level in (0, 28, 5000):
        kinds["hiss level %d" % level] = any(c.hiss_level == level for c in cp.values())
    missing = [k for k, ok in kinds.items() if not ok]
    assert not missing, missing
    # draws: one per channel-sample with hiss, none without
    for n, m in meta.items():
        assert m["rng_after"] == m["rng0"] + (m["frames"] * 2 if cp[n].hiss_level else 0), n
    # an input that clips: each edge of its full-scale square leaves the high-passes at nearly twice full scale; the
    # limiter holds that to +-1.0 in front of the FIR, whose taps sum to a little under 1, so the output comes close to
    # the rails and never sits on them as an unlimited signal would
    out = arrays["out_clip"]
    assert int((out >= 30000).sum()) > 10 and int((out <= -30000).sum()) > 10
    assert out.max() < 32767 and out.min() > -32768
    # silence without hiss stays silence; with hiss it does not
    assert not arrays["out_hiss_off_silence"].any() and arrays["out_silence"].any()
    # fed in blocks of 1, 3 and 1601 frames with 57 taps: the one-block run
    for b in ("b1", "b3", "b1601"):
        assert meta["preset3_" + b]["block"] == int(b[1:])
        assert meta["preset3_" + b]["sha256"] == meta["preset3"]["sha256"]
    # the mono downmix is the int division of the stereo run's pair: it truncates toward zero
    st, mo = arrays["out_default"].astype(np.int64), arrays["out_mono"].astype(np.int64)
    s = st[:, 0] + st[:, 1]
    assert int(((s < 0) & (s & 1 == 1)).sum()) > 10, "no pair whose sum is odd and negative"
    want = np.where(s < 0, -((-s) // 2), s // 2)
    assert (mo[:, 0] == want).all() and (mo[:, 1] == want).all()
    # a negative tilt is the mirror image: left and right swap their delays
    a, b = arrays["out_headalign_pos"], arrays["out_headalign_neg"]
    assert int((a != b).sum()) > a.size // 4
    # the shared pre-/de-emphasis states: swapping the input channels does not just swap the outputs
    a, b = arrays["out_both"], arrays["out_both_swapped"]
    assert (A.case_input("both_swapped") == A.case_input("both")[:, ::-1]).all()
    assert int((a[:, ::-1] != b).sum()) > a.size // 4
