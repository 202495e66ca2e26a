"""What the mixed-track cassette tests share: the decks (switch sets that differ in everything a track may now own), and
the host program tests/cass_mixed_tracks_check.cpp over csrc/cass_chain.hpp, built once per session.  The track sets and
the inputs are tests/_cass_tracks.py's."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

import _cass_ref as A
import _cass_tracks as T
import _libs as L

HERE = os.path.dirname(os.path.abspath(__file__))
STATE_BYTES = T.STATE_BYTES

# six decks in one wavefront: 57 and 8 taps, pre-emphasis on and off, hiss and none, -high 100 next to 20 Hz, mono,
# de-emphasis on some only.  Decks 0 and 1 have 57 taps: with the tracks of T.STRADDLE = (64, 1, 0, 193, 128, 385, 2, 63)
# cycling through the decks, the 1-frame track (index 1) and the 2-frame track (index 6) are shorter than their history.
DECKS = (A.BAD_DECK + ["-audio-hiss", "-30"], A.BAD_DECK + T.BOTH, ["-audio-hiss", "-200", "-deemphasis", "1"], ["-mono", "-high", "100"],
         ["-preemphasis", "1"], [])


def cycle(n, n_sets=len(DECKS)):
    return [t % n_sets for t in range(n)]


def params(flags, rate=None):
    """ntscsim_cass_params of the switches; rate: set in the struct, then derived (the tool has no switch for it)."""
    import ctypes as C
    from ntscsim import _capi
    cp = T.params(flags)
    if rate is not None:
        cp.rate = int(rate)
        assert _capi.lib().ntscsim_cass_params_derive(C.byref(cp)) == _capi.OK
    return cp


def decks(flag_sets=DECKS):
    return [params(f) for f in flag_sets]


@functools.lru_cache(maxsize=None)
def checker(build="plain"):
    """Path of tests/cass_mixed_tracks_check.cpp built with g++ as tests/cass_tracks_check.cpp is, once per session."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/cass_mixed_tracks_check.cpp"
    d = os.path.dirname(A.checker(build))                                       # the session's directory, cleaned up with it
    exe = os.path.join(d, "cass_mixed_tracks_check_" + build)
    csrc = os.path.join(L.PKG, "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + A._FLAGS[build] +
                          ["-I", csrc, "-I", os.path.join(L.ROOT, "include"), os.path.join(HERE, "cass_mixed_tracks_check.cpp"),
                           os.path.join(csrc, "glibc_rand.cpp"), "-o", exe])
    return exe


def spec(frames, counts, set_of, null=()):
    return ",".join("%d:%d:%d%s" % (f, c, s, ":n" if t in null else "") for t, (f, c, s) in enumerate(zip(frames, counts, set_of)))


def _cfgs(d, sets):
    paths = []
    for i, cp in enumerate(sets):
        paths.append(os.path.join(d, "cfg%d" % i))
        A.write_cfg(paths[-1], cp)
    return [str(len(sets))] + paths


def _ok(r):
    m = re.search(r"mixed: (\d+) checks, (\d+) bad", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) > 0 and int(m.group(2)) == 0, r.stdout


def run_check(sets, set_of, audio, frames, counts, plan, null=(), split=False, rng_pos=0, build="plain"):
    """`check` over a track set: ([(segments, repaired front, repaired back)] of the last call, rand() position behind
    it, sines evaluated).  plan: (L, WF, WB), WF -1: every track's own default.  Fails unless every assertion held."""
    with tempfile.TemporaryDirectory(prefix="cass_mixed_") as d:
        inp = os.path.join(d, "in")
        np.ascontiguousarray(audio).tofile(inp)
        r = subprocess.run([checker(build), "check"] + _cfgs(d, sets) + [inp] + [str(int(x)) for x in plan] +
                           [str(int(split)), str(rng_pos), spec(frames, counts, set_of, null)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    _ok(r)
    out = r.stdout
    stats = [tuple(int(x) for x in s.split("/")) for s in re.search(r"^stats(.*)$", out, re.M).group(1).split()]
    return stats, int(re.search(r"^pos (\d+)$", out, re.M).group(1)), int(re.search(r"^tilt (\d+)$", out, re.M).group(1))


def sines(sets, set_of, frames, counts, build="plain"):
    """(entries, runs) of the table of sines of a track set, its layout checked against brute force."""
    with tempfile.TemporaryDirectory(prefix="cass_mixed_") as d:
        r = subprocess.run([checker(build), "sines"] + _cfgs(d, sets) + [spec(frames, counts, set_of)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True)
    _ok(r)
    return int(re.search(r"^tilt (\d+)$", r.stdout, re.M).group(1)), int(re.search(r"^runs (\d+)$", r.stdout, re.M).group(1))


def expect(sets, set_of, audio, frames, counts, states_in=None, null=(), rng_pos=0):
    """The serial chain per track with that track's parameters, every tap, in one process: (outputs cut per track, end
    states as bytes [n * STATE_BYTES] as the mixed call must leave them, rand() position)."""
    n = len(frames)
    with tempfile.TemporaryDirectory(prefix="cass_mixed_") as d:
        inp, outp, sout, sin = (os.path.join(d, x) for x in ("in", "out", "sout", "sin"))
        np.ascontiguousarray(audio).tofile(inp)
        if states_in is not None:
            assert len(states_in) == n * STATE_BYTES
            with open(sin, "wb") as f:
                f.write(states_in)
        r = subprocess.run([checker(), "expect"] + _cfgs(d, sets) + [inp, outp, sout, sin if states_in is not None else "-", str(rng_pos),
                                                                     spec(frames, counts, set_of, null)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        out = np.fromfile(outp, np.int16).reshape(-1, 2)
        with open(sout, "rb") as f:
            states = f.read()
    assert len(states) == n * STATE_BYTES
    return T.cut(out, frames), states, int(re.search(r"^pos (\d+)$", r.stdout, re.M).group(1))
