"""What the multi-track cassette tests share: the switch sets, the track sets (the smallest at which the indexing of a
tracks call can go wrong) and the host program tests/cass_tracks_check.cpp over csrc/cass_chain.hpp, built once per
session.  The inputs are tests/_audio_ref.py's integer generator."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

import _audio_ref as AU
import _cass_ref as A
import _libs as L
from ntscsim import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
STATE_BYTES = C.sizeof(_capi.CassState)

BOTH = ["-preemphasis", "1", "-deemphasis", "1"]
# default tilt: 8 taps; -preset 3: 57 taps, so that tracks of 1 and 2 frames are shorter than the history
STRADDLE_FLAGS = [[], A.BAD_DECK, BOTH, A.BAD_DECK + BOTH, ["-mono"]]
# 1, 1, 0, 4, 2, 7, 1 and 1 segments of 64: 17 in six wavefronts of three groups, the last with two live groups
STRADDLE = (64, 1, 0, 193, 128, 385, 2, 63)
STRADDLE_PLANS = (((64, 20, 16), STRADDLE), ((1, 0, 0), STRADDLE[:4]), ((65, 64, 64), STRADDLE[:4]))
# the tile edges of the FIR (256 frames), a one-frame last tile, three tiles in one track, a track without frames
TILES = (256, 257, 255, 0, 513)
UNION_COUNTS, UNION_FRAMES = (0, 100, 100, 50, 3000000000), (300, 300, 50, 400, 300)   # [0, 450) and 300 more: 750 sines
NO_HISS_DEEMPH = ["-audio-hiss", "-200", "-deemphasis", "1"]
HIGH100 = ["-high", "100", "-deemphasis", "1"]                                   # front warm-up 5056 frames
MANY = 1100                                                                      # more than 1024 tracks, 8 frames each


def params(flags):
    return _capi.make_cass_params(list(flags))


def make_tracks(frames, kinds="music", seed=40):
    """One int16 [sum(frames), 2] buffer, the tracks back to back with different content in each, so that a warm-up, a
    halo or a tile that crossed a boundary would change bits."""
    if isinstance(kinds, str):
        kinds = [kinds] * len(frames)
    parts = [AU.make_input(k, f, 2, seed + 3 * t) for t, (f, k) in enumerate(zip(frames, kinds))]
    return np.concatenate(parts) if parts else np.zeros((0, 2), np.int16)


def cut(buf, frames):
    """views of the tracks in `buf` (numpy or torch, [frames, 2])"""
    out, at = [], 0
    for f in frames:
        out.append(buf[at:at + f])
        at += f
    return out


@functools.lru_cache(maxsize=None)
def checker(build="plain"):
    """Path of tests/cass_tracks_check.cpp built with g++ as tests/cass_chain_check.cpp is, once per session."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/cass_tracks_check.cpp"
    d = os.path.dirname(A.checker(build))                                       # the session's directory, cleaned up with it
    exe = os.path.join(d, "cass_tracks_check_" + build)
    csrc = os.path.join(L.PKG, "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + A._FLAGS[build] +
                          ["-I", csrc, "-I", os.path.join(L.ROOT, "include"), os.path.join(HERE, "cass_tracks_check.cpp"), os.path.join(csrc, "glibc_rand.cpp"), "-o", exe])
    return exe


def spec(frames, counts, null=()):
    return ",".join("%d:%d%s" % (f, c, ":n" if t in null else "") for t, (f, c) in enumerate(zip(frames, counts)))


def run_check(cp, audio, frames, counts, plan, null=(), split=False, rng_pos=0, build="plain"):
    """`check` over a track set: ([(segments, repaired front, repaired back)] of the last call, rand() position behind
    it, sines evaluated).  Fails unless every assertion of the program held."""
    with tempfile.TemporaryDirectory(prefix="cass_tracks_") as d:
        cfg, inp = os.path.join(d, "cfg"), os.path.join(d, "in")
        A.write_cfg(cfg, cp)
        np.ascontiguousarray(audio).tofile(inp)
        r = subprocess.run([checker(build), "check", cfg, inp] + [str(int(x)) for x in plan] + [str(int(split)), str(rng_pos), spec(frames, counts, null)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = r.stdout
    m = re.search(r"tracks: (\d+) checks, (\d+) bad", out)
    assert r.returncode == 0 and m and int(m.group(1)) > 0 and int(m.group(2)) == 0, out
    stats = [tuple(int(x) for x in s.split("/")) for s in re.search(r"^stats(.*)$", out, re.M).group(1).split()]
    return stats, int(re.search(r"^pos (\d+)$", out, re.M).group(1)), int(re.search(r"^tilt (\d+)$", out, re.M).group(1))


def expect(cp, audio, frames, counts, states_in=None, null=(), rng_pos=0):
    """The serial chain per track, every tap, in one process: (outputs cut per track, end states as bytes
    [n * STATE_BYTES] as the tracks call must leave them, rand() position).  states_in: bytes of the states the tracks
    start from (None: zeros); their count and taps fields are not read."""
    n = len(frames)
    with tempfile.TemporaryDirectory(prefix="cass_tracks_") as d:
        cfg, inp, outp, sout, sin = (os.path.join(d, x) for x in ("cfg", "in", "out", "sout", "sin"))
        A.write_cfg(cfg, cp)
        np.ascontiguousarray(audio).tofile(inp)
        if states_in is not None:
            assert len(states_in) == n * STATE_BYTES
            with open(sin, "wb") as f:
                f.write(states_in)
        r = subprocess.run([checker(), "expect", cfg, inp, outp, sout, sin if states_in is not None else "-", str(rng_pos), spec(frames, counts, null)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
        out = np.fromfile(outp, np.int16).reshape(-1, 2)
        with open(sout, "rb") as f:
            states = f.read()
    assert len(states) == n * STATE_BYTES
    return cut(out, frames), states, int(re.search(r"^pos (\d+)$", r.stdout, re.M).group(1))
