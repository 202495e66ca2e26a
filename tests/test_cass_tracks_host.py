"""The multi-track plan of csrc/cass_chain.hpp on the host: the track table, the segment-to-track and tile-to-track
lookups, the tilt union and cass_run_tracks_planned(), which states what the k_cass_track_* kernels do.

tests/cass_tracks_check.cpp, a stand-alone program with its own main, is built plain and with the address and
undefined-behaviour sanitizers and run as the program it is.  For every track set of tests/test_cass_tracks_gpu.py it
asserts that the planned tracks equal cass_run_serial (every tap) run per track from that track's state and count --
output bytes, the 28 filter values and the taps - 1 history frames bitwise, count and taps -- that the per-track segment
and repair counts are those of cass_run_planned on that track alone, that both lookups map every call-wide index to the
(track, local index) a linear walk finds, tracks without frames included, that cass_tilt_layout's union length and
offsets agree with a brute-force set of the counts, and that an overflowing count + frames is reported."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _cass_ref as A
import _cass_tracks as T
import _libs as L
from ntscsim import _capi

BUILDS = ["plain", "sanitized"]


def segs(frames, seg_len):
    return [(f + seg_len - 1) // seg_len for f in frames]


@pytest.mark.parametrize("build", BUILDS)
def test_the_feature_set(build):
    cp = T.params([])
    stats, pos, tilt = T.run_check(cp, T.make_tracks([4096, 4096], seed=21), [4096, 4096], [0, 0], (4096, -1, -1), build=build)
    assert stats == [(1, 0, 0)] * 2 and pos == 4 * 4096 and tilt == 4096


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("flags", T.STRADDLE_FLAGS, ids=lambda f: " ".join(f) or "default")
def test_groups_straddle_tracks(flags, build):
    cp = T.params(flags)
    assert cp.taps == (57 if "-preset" in flags else 8)
    for plan, frames in T.STRADDLE_PLANS:
        stats, pos, tilt = T.run_check(cp, T.make_tracks(frames), frames, [0] * len(frames), plan, rng_pos=11, build=build)
        assert [s[0] for s in stats] == segs(frames, plan[0]), plan
        assert pos == 11 + 2 * sum(frames) and tilt == max(frames)
    assert sum(segs(T.STRADDLE, 64)) == 17
    # two calls on the same states: the history of the 1- and 2-frame tracks is partly the call's before
    T.run_check(cp, T.make_tracks(T.STRADDLE), T.STRADDLE, [7 * t for t in range(8)], (64, 20, 16), split=True, build=build)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("flags", [A.BAD_DECK, A.BAD_DECK + ["-deemphasis", "1"]], ids=" ".join)
def test_tiles(flags, build):
    cp = T.params(flags)
    counts = [0, 1000, 5, 77, 100000]
    stats, _, tilt = T.run_check(cp, T.make_tracks(T.TILES), T.TILES, counts, (4096, -1, -1), split=True, build=build)
    assert [s[0] for s in stats] == [1, 1, 1, 0, 1]


@pytest.mark.parametrize("build", BUILDS)
def test_counts_and_the_tilt_union(build):
    cp = T.params([])
    _, _, tilt = T.run_check(cp, T.make_tracks([300] * 16), [300] * 16, [0] * 16, (4096, -1, -1), build=build)
    assert tilt == 300                                                          # not 4800
    _, _, tilt = T.run_check(cp, T.make_tracks(T.UNION_FRAMES), T.UNION_FRAMES, T.UNION_COUNTS, (4096, -1, -1), null=(2,), build=build)
    assert tilt == 450 + 300
    frames, counts = [100, 200, 50], [0, 100, 1000]                             # disjoint (two of them touch): the sum
    _, _, tilt = T.run_check(cp, T.make_tracks(frames), frames, counts, (64, 20, 16), build=build)
    assert tilt == 350


@pytest.mark.parametrize("build", BUILDS)
def test_repairs_in_some_tracks_only(build):
    cp = T.params(T.NO_HISS_DEEMPH)
    assert cp.hiss_level == 0
    a = T.make_tracks([3000, 3000], ["music", "silence"])
    stats, pos, _ = T.run_check(cp, a, [3000, 3000], [0, 0], (256, 0, 0), build=build)
    assert stats[1] == (12, 0, 0) and pos == 0                                  # silence without hiss: a zero state IS the true state
    assert stats[0][0] == 12 and stats[0][1] == 11 and stats[0][2] >= 11 - cp.taps
    assert stats[0] == A.plan_stats(cp, a[:3000], 256, 0, 0)


@pytest.mark.parametrize("build", BUILDS)
def test_default_plan_needs_no_repair(build):
    """the CPU half of the GPU test's zero repairs: on these inputs both passes of every track converge in time"""
    cp = T.params(T.HIGH100)
    stats, _, tilt = T.run_check(cp, T.make_tracks([12000] * 3), [12000] * 3, [0] * 3, (4096, -1, -1), rng_pos=1000, build=build)
    assert stats == [(3, 0, 0)] * 3 and tilt == 12000


@pytest.mark.parametrize("build", BUILDS)
def test_many_short_tracks(build):
    cp = T.params(["-deemphasis", "1"])
    frames, counts = [8] * T.MANY, [1000 * t for t in range(T.MANY)]
    stats, pos, tilt = T.run_check(cp, T.make_tracks(frames, seed=5), frames, counts, (4096, -1, -1), rng_pos=7, build=build)
    assert stats == [(1, 0, 0)] * T.MANY and pos == 7 + 16 * T.MANY and tilt == 8 * T.MANY


def test_expect_mode_is_the_serial_chain():
    """the mode the GPU tests take their expectation from equals tests/cass_chain_check.cpp's serial run per track"""
    cp = T.params(A.BAD_DECK + ["-deemphasis", "1"])
    frames, counts = [300, 0, 40], [5, 9, 3000000000]
    a = T.make_tracks(frames)
    outs, states, pos = T.expect(cp, a, frames, counts, rng_pos=3)
    at = 3
    for t in (0, 2):
        want, (vals, count, hist), at = A.run_checker(cp, T.cut(a, frames)[t], count0=counts[t], rng_pos=at)
        assert (outs[t] == want).all()
        s = _capi.CassState.from_buffer_copy(states[t * T.STATE_BYTES:(t + 1) * T.STATE_BYTES])
        assert s.count == count == counts[t] + frames[t] and s.taps == 57
        got = [x for c in s.bandpass for x in c] + list(s.pre) + list(s.post)
        assert (np.array(got).view(np.uint64) == vals).all()
        assert (np.array([list(s.history[k]) for k in range(56)]).view(np.uint64) == hist).all()
    assert pos == at and not any(states[T.STATE_BYTES:2 * T.STATE_BYTES])
    # the second call from those states equals one call over both
    outs2, states2, pos2 = T.expect(cp, a, frames, [c + f for c, f in zip(counts, frames)], states_in=states, rng_pos=pos)
    both = np.concatenate([T.cut(a, frames)[0], T.cut(a, frames)[0]])
    want, _, _ = A.run_checker(cp, both, count0=5, rng_pos=3, block="blocks=300:3,300:%d" % pos)
    assert (np.concatenate([outs[0], outs2[0]]) == want).all()


def test_struct_layouts_match_the_ctypes_mirrors(tmp_path):
    """ntscsim_cass_track and what it points to, as a strict C99 program sees them, against ntscsim/_capi.py"""
    assert shutil.which("gcc") is not None, "gcc is needed to read the header's layout"
    structs = {"ntscsim_cass_track": _capi.CassTrack, "ntscsim_cass_desc": _capi.CassDesc, "ntscsim_cass_state": _capi.CassState,
               "ntscsim_cass_stats": _capi.CassStats}
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
    assert C.sizeof(_capi.CassTrack) == 32 and C.sizeof(_capi.CassState) == 8416 == T.STATE_BYTES
    for sym in ("ntscsim_cass_tracks_device", "ntscsim_cass_debug_track_stats", "ntscsim_cass_debug_tilt_frames"):
        assert sym in _capi.EXPORTS and hasattr(_capi.lib(), sym)


def test_track_kernels_use_no_scratch_memory():
    """Code-object metadata of csrc/ntsc_cass.o, read as tests/test_params_capi.py reads the other device objects':
    no cassette kernel, the five k_cass_track_* among them, has a private segment."""
    obj = os.path.join(L.PKG, "csrc", "ntsc_cass.o")
    if not os.path.exists(obj) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("c++filt") is None:
        pytest.skip("device object or llvm tools not present")
    out = subprocess.run(["sh", os.path.join(L.ROOT, "tools", "kres.sh"), obj], cwd=L.ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stderr
    rows = [ln for ln in out.stdout.splitlines() if "\t" in ln and "k_cass_" in ln]
    names = [ln.split("(")[0].split("::")[-1] for ln in rows]
    for k in ("k_cass_track_front", "k_cass_track_front_verify", "k_cass_track_conv", "k_cass_track_back", "k_cass_track_back_verify"):
        assert k in names, names
    bad = [ln for ln in rows if " scratch 0 " not in ln + " " or not ln.rstrip().endswith("spill 0")]
    assert not bad, "\n".join(bad)
