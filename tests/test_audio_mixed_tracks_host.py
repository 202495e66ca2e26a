"""The mixed-track plan of csrc/audio_chain.hpp on the host: audio_mixed_layout() (plane, segments, the channel-sample
offsets of the tracks that draw, a warm-up per track) and audio_run_mixed_tracks_planned(), which states what
k_audio_mixed_segments and k_audio_mixed_verify do.

tests/audio_mixed_tracks_check.cpp, a stand-alone program with its own main, is built plain and with the address and
undefined-behaviour sanitizers and run as the program it is.  For the track sets of tests/test_audio_mixed_tracks_gpu.py
it asserts that the planned tracks equal audio_run_serial run per track with that track's cfg -- bytes, states bitwise,
counts, the rand() position -- and that segment and repair counts are those of the single-stream plan on that track alone.

test_default_plan_sets_need_no_repair is the CPU half of the GPU test's `repaired == 0`, on the same generator inputs."""
import re

import pytest

import _audio_mixed as M
import _audio_tracks as T

BUILDS = ["plain", "sanitized"]


def run(names, set_of, frames, plan, states=None, kinds="music", rng_pos=0, build="plain", seed=40):
    sets = M.sets_of(names)
    tracks = M.make_tracks(frames, sets, set_of, kinds, seed)
    rc, out = M.run_mixed_check(sets, set_of, tracks, plan, states, rng_pos, build)
    m = re.search(r"mixed: (\d+) checks, (\d+) bad", out)
    assert rc == 0 and m and int(m.group(1)) > 0 and int(m.group(2)) == 0, out
    stats = [tuple(int(x) for x in s.split("/")) for s in re.search(r"^stats(.*)$", out, re.M).group(1).split()]
    pos = int(re.search(r"^pos (\d+)$", out, re.M).group(1))
    return stats, pos, sets


@pytest.mark.parametrize("build", BUILDS)
def test_three_sets_in_one_wavefront(build):
    set_of = [t % len(M.CYCLE) for t in range(len(T.STRADDLE))]
    stats, pos, sets = run(M.CYCLE, set_of, T.STRADDLE, (64, 20), build=build, rng_pos=11)
    on = [sets[s].enabled for s in set_of]
    assert [s[0] for s in stats] == [(f + 63) // 64 if e else 0 for f, e in zip(T.STRADDLE, on)]
    assert pos == 11 + sum(f * sets[s].channels for f, s in zip(T.STRADDLE, set_of) if sets[s].enabled and sets[s].hiss_level)
    for plan in ((1, 0), (65, 64)):
        stats, _, _ = run(M.CYCLE, set_of[:4], T.STRADDLE[:4], plan, build=build)
        assert [s[0] for s in stats] == [(f + plan[0] - 1) // plan[0] for f in T.STRADDLE[:4]]


@pytest.mark.parametrize("build", BUILDS)
def test_default_plan_sets_need_no_repair(build):
    """three stereo_hifi tracks of 60000 frames and three stereo_linear tracks of 12000, interleaved, each at its own
    default warm-up (25,280 and 5,056 frames)"""
    frames = [60000, 12000] * 3
    stats, _, sets = run(["stereo_hifi", "stereo_linear"], [0, 1] * 3, frames, (4096, -1), build=build, rng_pos=1000)
    assert stats == [((f + 4095) // 4096, 0) for f in frames], stats
    assert sets[0].highpass_hz == 20 and sets[1].highpass_hz == 100


@pytest.mark.parametrize("build", BUILDS)
def test_the_feature_tracks(build):
    stats, pos, _ = run(["stereo_hifi", "mono_lp"], [0, 1], [4096, 4096], (4096, -1), build=build)
    assert stats == [(1, 0), (1, 0)] and pos == 3 * 4096


@pytest.mark.parametrize("build", BUILDS)
def test_states_counts_and_copies(build):
    """a NULL state, counts of hours on an NTSC and a PAL track (the buzz phase follows them), a copied track with a
    state, tracks without frames"""
    names = ["stereo_linear", "pal_linear", "nocomp", "loud_hiss"]
    stats, _, _ = run(names, [0, 1, 2, 3, 1, 0], [3000, 3000, 500, 0, 700, 0], (256, 64),
                      states=["n", "3000000000", "77", "z", str((1 << 31) + 5), "9"], build=build, rng_pos=5)
    assert [s[0] for s in stats] == [12, 12, 0, 0, 3, 0]


def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """ntscsim_audio_mixed_track, as a strict C99 program sees it, against ntscsim/_capi.py"""
    import ctypes as C
    import os
    import shutil
    import subprocess
    import _libs as L
    from ntscsim import _capi
    assert shutil.which("gcc") is not None, "gcc is needed to read the header's layout"
    cname, mirror = "ntscsim_audio_mixed_track", _capi.AudioMixedTrack
    lines = ['#include "ntscsim.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {", 'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for fname, _ in mirror._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(L.ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out[cname]) == C.sizeof(mirror) == 24
    for fname, _ in mirror._fields_:
        assert int(out["%s.%s" % (cname, fname)]) == getattr(mirror, fname).offset, fname
    assert _capi.AudioMixedTrack.set.offset == 12
    for sym in ("ntscsim_audio_mixed_tracks_device", "ntscsim_audio_mixed_tracks_host"):
        assert sym in _capi.EXPORTS and hasattr(_capi.lib(), sym)
