"""The multi-track plan of csrc/audio_chain.hpp on the host: the track table, the segment-to-track lookup and
audio_run_tracks_planned(), which states what k_audio_track_segments and k_audio_track_verify do.

tests/audio_tracks_check.cpp, a stand-alone program with its own main, is built plain and with the address and
undefined-behaviour sanitizers and run as the program it is.  For every track set of tests/test_audio_tracks_gpu.py it
asserts that the planned tracks equal audio_run_serial run per track from that track's state -- output bytes, the 30 state
values bitwise, the counts -- that the per-track segment and repair counts are those of the single-track plan on that
track alone, and that audio_track_of maps every call-wide segment index to the (track, local segment) a linear walk
finds, tracks without frames included.

test_default_plan_sets_need_no_repair is the CPU half of the GPU test's `repaired == 0`: on the generator inputs that
test uses, every speculative segment of every track meets the true state within the default warm-up."""
import re

import pytest

import _audio_tracks as T

BUILDS = ["plain", "sanitized"]


def run(preset, frames, plan, states=None, kinds="music", split=False, rng_pos=0, build="plain", seed=40):
    ap = T.PRESETS[preset]()
    a = T.make_tracks(frames, ap.channels, kinds, seed)
    rc, out = T.run_tracks_check(ap, a, plan, list(zip(frames, states or ["z"] * len(frames))), split, rng_pos, build)
    m = re.search(r"tracks: (\d+) checks, (\d+) bad", out)
    assert rc == 0 and m and int(m.group(1)) > 0 and int(m.group(2)) == 0, out
    stats = [tuple(int(x) for x in s.split("/")) for s in re.search(r"^stats(.*)$", out, re.M).group(1).split()]
    pos = int(re.search(r"^pos (\d+)$", out, re.M).group(1))
    return stats, pos, ap


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("preset", ["mono_lp", "stereo_hifi", "stereo_linear"])
def test_groups_straddle_tracks(preset, build):
    stats, pos, ap = run(preset, T.STRADDLE, (64, 20), build=build, rng_pos=11)
    assert [s[0] for s in stats] == [(f + 63) // 64 for f in T.STRADDLE] and sum(s[0] for s in stats) == 17
    assert pos == 11 + sum(T.STRADDLE) * ap.channels
    for plan in ((1, 0), (65, 64)):
        stats, _, _ = run(preset, T.STRADDLE[:4], plan, build=build)
        assert [s[0] for s in stats] == [(f + plan[0] - 1) // plan[0] for f in T.STRADDLE[:4]]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("preset,frames", [("stereo_hifi", 60000), ("stereo_linear", 12000)])
def test_default_plan_sets_need_no_repair(preset, frames, build):
    stats, _, _ = run(preset, [frames] * 3, (4096, -1), build=build)
    assert stats == [((frames + 4095) // 4096, 0)] * 3, stats


@pytest.mark.parametrize("build", BUILDS)
def test_repair_in_some_tracks_only(build):
    stats, pos, _ = run("no_hiss", [3000, 3000], (256, 0), kinds=["music", "silence"], build=build)
    assert stats == [(12, 11), (12, 0)] and pos == 0


@pytest.mark.parametrize("build", BUILDS)
def test_states_counts_and_two_calls(build):
    """a NULL state, a state at a count of hours, a zero state; a prefix call and then the rest on the same states"""
    run("stereo_linear", [3000, 3000, 3000, 0], (256, 64), states=["n", "3000000000", "z", "7"], split=True, build=build)
    run("mono_lp", [100] * 200, (4096, -1), states=[str(1000 * t) for t in range(200)], build=build)


def test_struct_layouts_match_the_ctypes_mirrors(tmp_path):
    """ntscsim_audio_track and what it points to, as a strict C99 program sees them, against ntscsim/_capi.py"""
    import ctypes as C
    import os
    import shutil
    import subprocess
    import _libs as L
    from ntscsim import _capi
    assert shutil.which("gcc") is not None, "gcc is needed to read the header's layout"
    structs = {"ntscsim_audio_track": _capi.AudioTrack, "ntscsim_audio_desc": _capi.AudioDesc, "ntscsim_audio_state": _capi.AudioState,
               "ntscsim_audio_stats": _capi.AudioStats}
    lines = ['#include "ntscsim.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {"]
    for cname, mirror in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(L.ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, mirror in structs.items():
        assert int(out[cname]) == C.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert int(out["%s.%s" % (cname, fname)]) == getattr(mirror, fname).offset, (cname, fname)
    assert C.sizeof(_capi.AudioState) == 248
    for sym in ("ntscsim_audio_tracks_device", "ntscsim_audio_debug_track_stats"):
        assert sym in _capi.EXPORTS and hasattr(_capi.lib(), sym)


@pytest.mark.parametrize("build", BUILDS)
def test_nocomp_copies(build):
    stats, pos, _ = run("nocomp", [100, 0, 300], (64, 20), build=build, rng_pos=9)
    assert stats == [(0, 0)] * 3 and pos == 9
