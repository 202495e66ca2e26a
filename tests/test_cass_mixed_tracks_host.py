"""The mixed tracks plan of csrc/cass_chain.hpp on the host (parameters per track): cass_mixed_set_table(),
cass_mixed_layout() (a section of the x plane of every track's OWN taps, a warm-up per track), cass_sine_layout() (the
table holds sines, one union of counts per distinct rate) and cass_run_mixed_tracks_planned(), which states what the
k_cass_mixed_* kernels do.

tests/cass_mixed_tracks_check.cpp, a stand-alone program with its own main, is built plain and with the address and
undefined-behaviour sanitizers and run as the program it is.  For the track sets of tests/test_cass_mixed_tracks_gpu.py it
asserts that the planned tracks equal cass_run_serial (every tap) run per track with that track's cfg -- bytes, states
bitwise with the whole history array, counts, taps, the rand() position -- and that segment and repair counts are those
of the single-stream plan on that track alone with its own warm-up.  Every `check` here runs with SPLIT, so the second
call starts from a carried history of every track's own length."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import _cass_mixed as M
import _cass_ref as A
import _cass_tracks as T
import _libs as L
from ntscsim import _capi

BUILDS = ["plain", "sanitized"]


def hiss_draws(sets, set_of, frames):
    return sum(2 * f for f, s in zip(frames, set_of) if sets[s].hiss_level != 0)


@pytest.mark.parametrize("build", BUILDS)
def test_six_decks_in_one_wavefront(build):
    sets = M.decks()
    assert [s.taps for s in sets] == [57, 57, 8, 8, 8, 8] and [s.deemphasis for s in sets] == [0, 1, 1, 0, 0, 0]
    assert sets[2].hiss_level == 0 and sets[0].hiss_level > sets[5].hiss_level > 0 and sets[3].mono and sets[3].highpass_hz == 100
    for plan, frames in T.STRADDLE_PLANS:
        set_of, counts = M.cycle(len(frames)), [0] * len(frames)
        a = T.make_tracks(frames)
        stats, pos, tilt = M.run_check(sets, set_of, a, frames, counts, plan, split=True, rng_pos=3, build=build)
        assert [s[0] for s in stats] == [(f - f // 3 + plan[0] - 1) // plan[0] for f in frames], plan
        assert pos == 3 + hiss_draws(sets, set_of, frames)
        assert all(s[2] == 0 for s, k in zip(stats, set_of) if not sets[k].deemphasis)
        _, _, tilt = M.run_check(sets, set_of, a, frames, counts, plan, rng_pos=3, build=build)
        assert tilt == max(frames)                                              # one rate, all from count 0: one tape's sines


@pytest.mark.parametrize("build", BUILDS)
def test_tiles_with_alternating_taps(build):
    """the halo of a 57-tap track's first tile stands behind an 8-tap track's section"""
    sets = [T.params([]), T.params(A.BAD_DECK)]
    set_of, counts = [0, 1, 0, 1, 0], [0, 1000, 5, 77, 100000]
    a = T.make_tracks(T.TILES)
    stats, _, _ = M.run_check(sets, set_of, a, T.TILES, counts, (64, 20, 16), split=True, rng_pos=9, build=build)
    assert [s[0] for s in stats] == [(f - f // 3 + 63) // 64 for f in T.TILES]


@pytest.mark.parametrize("build", BUILDS)
def test_deemphasis_on_none_and_on_all(build):
    frames, counts = [130, 70, 200], [0, 9, 44100]
    a = T.make_tracks(frames)
    for flag_sets in (([], A.BAD_DECK, ["-mono"]), (["-deemphasis", "1"], A.BAD_DECK + T.BOTH, T.NO_HISS_DEEMPH)):
        sets = M.decks(flag_sets)
        M.run_check(sets, [0, 1, 2], a, frames, counts, (64, 20, 16), null=(1,), split=True, build=build)


@pytest.mark.parametrize("build", BUILDS)
def test_repairs_in_one_track_only(build):
    sets = [T.params(T.NO_HISS_DEEMPH), T.params(["-audio-hiss", "-200"])]
    frames, counts = [3000, 3000, 3000], [0, 0, 0]
    a = T.make_tracks(frames, ["music", "silence", "music"])
    stats, pos, _ = M.run_check(sets, [0, 0, 1], a, frames, counts, (256, 0, 0), build=build)
    assert stats[1] == (12, 0, 0) and stats[0][1] == 11 and stats[0][2] > 0 and stats[2][1] == 11 and stats[2][2] == 0
    assert pos == 0


@pytest.mark.parametrize("build", BUILDS)
def test_default_plan_warms_up_per_track(build):
    """three tracks of 60000 frames at 20 Hz (25,280 frames of warm-up) interleaved with three of 12000 at -high 100
    (5,056): no repair with every track at its own warm-up"""
    sets = [T.params([]), T.params(["-high", "100"])]
    frames = [60000, 12000] * 3
    a = T.make_tracks(frames)
    stats, pos, tilt = M.run_check(sets, [0, 1] * 3, a, frames, [0] * 6, (4096, -1, -1), rng_pos=1000, build=build)
    assert stats == [((f + 4095) // 4096, 0, 0) for f in frames], stats
    assert pos == 1000 + 2 * sum(frames) and tilt == 60000


def test_the_sine_union():
    tilts = [T.params(["-headalign", str(h), "-headalignwaver", str(w)]) for h, w in ((0, 0), (1, 2), (-3, 1), (10, 3))]
    assert len({(s.head_tilt, s.head_tilt_waver) for s in tilts}) == 4 and len({s.taps for s in tilts}) > 1
    frames = [300, 200, 250, 100]
    assert M.sines(tilts, [0, 1, 2, 3], frames, [0] * 4) == (300, 1)             # same counts, different tilt and waver
    same_rate = M.decks()
    assert M.sines(same_rate, M.cycle(4), frames, [0] * 4) == (300, 1)           # same counts, one rate
    two = [T.params([]), M.params([], rate=48000)]
    assert two[1].rate == 48000 and two[1].alpha_lowpass != two[0].alpha_lowpass
    assert M.sines(two, [0, 1, 0, 1], frames, [0] * 4) == (300 + 200, 2)         # two rates at the same counts: the sum
    three = M.decks(([], A.BAD_DECK, ["-mono"]))
    assert M.sines(three, [0, 1, 2, 0, 1], T.UNION_FRAMES, T.UNION_COUNTS) == (750, 2)   # [0, 450) and 300 far away
    assert M.sines([three[0], two[1], three[2]], [0, 1, 2, 0, 1], T.UNION_FRAMES, T.UNION_COUNTS) == (450 + 300 + 300, 3)


def test_expect_mode_on_one_set_is_the_tracks_checker():
    """the `expect` mode that the GPU tests rely on, pinned to tests/cass_tracks_check.cpp's"""
    cp = T.params(A.BAD_DECK + T.BOTH)
    frames, counts = [300, 0, 40, 700], [0, 5, 1 << 40, 77]
    a = T.make_tracks(frames)
    lead, lead_states, _ = T.expect(cp, a, frames, counts)
    want = T.expect(cp, a, frames, counts, states_in=lead_states, null=(2,), rng_pos=7)
    got = M.expect([T.params([]), cp], [1] * 4, a, frames, counts, states_in=lead_states, null=(2,), rng_pos=7)
    assert all((g == w).all() for g, w in zip(got[0], want[0])) and got[1] == want[1] and got[2] == want[2]


def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """ntscsim_cass_mixed_track, as a strict C99 program sees it, against ntscsim/_capi.py"""
    assert shutil.which("gcc") is not None, "gcc is needed to read the header's layout"
    cname, mirror = "ntscsim_cass_mixed_track", _capi.CassMixedTrack
    lines = ['#include "ntscsim.h"', "#include <stdio.h>", "#include <stddef.h>", "int main(void) {", 'printf("%s %%zu\\n", sizeof(%s));' % (cname, cname)]
    for fname, _ in mirror._fields_:
        lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(L.ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split() for ln in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out[cname]) == C.sizeof(mirror) == 32
    for fname, _ in mirror._fields_:
        assert int(out["%s.%s" % (cname, fname)]) == getattr(mirror, fname).offset, fname
    assert mirror.set.offset == 12 and mirror.count.offset == 16 and mirror.state.offset == 24
    for sym in ("ntscsim_cass_mixed_tracks_device", "ntscsim_cass_mixed_tracks_host"):
        assert sym in _capi.EXPORTS and hasattr(_capi.lib(), sym)


def test_mixed_kernels_use_no_scratch_memory():
    """Code-object metadata of csrc/ntsc_cass.o through tools/kres.sh: the five k_cass_mixed_* kernels are there by
    name, without a private segment and without spills."""
    obj = os.path.join(L.PKG, "csrc", "ntsc_cass.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("device object or llvm tools not present")
    out = subprocess.run(["sh", os.path.join(L.ROOT, "tools", "kres.sh"), obj], cwd=L.ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr
    rows = {ln.split("(")[0].split("::")[-1]: ln for ln in out.stdout.splitlines() if "\t" in ln and "k_cass_mixed_" in ln}
    assert sorted(rows) == ["k_cass_mixed_back", "k_cass_mixed_back_verify", "k_cass_mixed_conv", "k_cass_mixed_front", "k_cass_mixed_front_verify"]
    bad = [ln for ln in rows.values() if " scratch 0 " not in ln + " " or not ln.rstrip().endswith("spill 0")]
    assert not bad, "\n".join(bad)
