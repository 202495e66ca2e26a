"""csrc/audio_chain.hpp against the reference's own lines.

tests/golden/audio_ref.npz was recorded once from composite_audio_process() as the tools contain it: the lines
ffmpeg_ntsc.cpp:51-65 (dBFS), :74-203 (the filters), :889-970 (the chain), the post-parse derivation :1229-1267 and the
set-up :2031-2067 were copied, unchanged, into a scratch program behind libc / STL headers alone -- the libav includes cut
away, the globals those lines read declared with the tool's initial values, the audio switches applied as parse_argv()
:1051-1203 applies them, rand() counted through a macro -- compiled with g++ -O2 -ffp-contract=off and run on the inputs
of tests/_audio_ref.py (an integer generator: no libm in it).  No stand-in type was needed, so the runs are pinned in the
sense of DESIGN.md 4.  Only data is kept: per case the switches, the input's SHA-256, the rand() position behind the
run, the output's SHA-256, and the full output of the runs of 2048 frames.  The sibling tool's text
(ffmpeg_to_composite.cpp:558-627) is the same line for line and was not recorded a second time.

Here the host checker (tests/audio_chain_check.cpp, the header run serially) must reproduce every recorded run."""
import os

import numpy as np
import pytest

import _audio_ref as A
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
            assert A.sha(arrays["out_" + name]) == m["sha256"]


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_header_equals_the_recorded_run(name):
    meta, arrays = A.fixture()
    m = meta[name]
    ap, _ = _capi.make_audio_params(m["flags"])
    assert ap.channels == m["channels"]
    out, _state, pos = A.run_checker(ap, A.case_input(name), m["count0"], m["rng0"], m["block"])
    if "out_" + name in arrays:
        want = arrays["out_" + name]
        bad = int((out != want).sum())
        assert bad == 0, "%d wrong samples, first at %d" % (bad, int(np.argmax((out != want).reshape(-1))))
    assert A.sha(out) == m["sha256"]
    assert pos == m["rng_after"]


def test_recording_covers_every_kind_of_case():
    meta, arrays = A.fixture()
    ap = {n: _capi.make_audio_params(m["flags"])[0] for n, m in meta.items()}
    kinds = {
        "hifi stereo with emphasis": any(a.hifi and a.channels == 2 and a.preemphasis and a.deemphasis for a in ap.values()),
        "hifi stereo without emphasis": any(a.hifi and a.channels == 2 and not a.preemphasis and not a.deemphasis for a in ap.values()),
        "linear emphasis": any(not a.hifi and a.preemphasis and a.emphasis_hz == 8000 for a in ap.values()),
        "pal": any(a.vsync_lines == 625 and not a.hifi for a in ap.values()),
        "nocomp": any(not a.enabled for a in ap.values()),
        "count above 2^31": any(m["count0"] > 1 << 31 and not ap[n].hifi for n, m in meta.items()),
        "rand() position not 0": any(m["rng0"] > 0 and ap[n].hiss_level for n, m in meta.items()),
        "long runs": sum(m["frames"] >= 12000 for m in meta.values()) >= 4,
    }
    for lp in (10000, 7000, 4000):
        kinds["linear mono %d Hz with buzz and boost" % lp] = any(
            not a.hifi and a.channels == 1 and a.lowpass_hz == lp and a.highpass_hz == 100 and a.buzz > 1e-9 and a.boost_gain > 0 for a in ap.values())
    for level in (0, 1, 39, 5000):
        kinds["hiss level %d" % level] = any(a.hiss_level == level and a.enabled for a in ap.values())
    missing = [k for k, ok in kinds.items() if not ok]
    assert not missing, missing
    # draws: one per channel-sample with hiss, none without, none with -nocomp
    for n, m in meta.items():
        draws = m["frames"] * m["channels"] if ap[n].enabled and ap[n].hiss_level else 0
        assert m["rng_after"] == m["rng0"] + draws, n
    # an input that clips: the limiter's +-1.0 reaches the output as the rails
    out = arrays["out_hifi_noemph_clip"]
    assert int((out == 32767).sum()) > 10 and int((out == -32768).sum()) > 10
    # fed in blocks of 1, 1024 and 1601 frames: the one-block run
    for b in ("b1", "b1024", "b1601"):
        assert meta["hifi_default_" + b]["block"] == int(b[1:])
        assert meta["hifi_default_" + b]["sha256"] == meta["hifi_default"]["sha256"]
    # -nocomp copies
    assert (arrays["out_nocomp"] == A.case_input("nocomp")).all()
    # the shared pre-/de-emphasis states: swapping the input channels does not just swap the outputs
    a, b = arrays["out_hifi_default"], arrays["out_hifi_default_swapped"]
    assert (A.case_input("hifi_default_swapped") == A.case_input("hifi_default")[:, ::-1]).all()
    assert int((a[:, ::-1] != b).sum()) > a.size // 4
