"""What the multi-track audio tests share: the presets, the track sets (the smallest at which the indexing of a tracks
call can go wrong) and the host program tests/audio_tracks_check.cpp over csrc/audio_chain.hpp, built once per session."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import _audio_ref as A
import _libs as L
from ntscsim import _capi

HERE = os.path.dirname(os.path.abspath(__file__))


def params(flags, **edit):
    ap, _ = _capi.make_audio_params(list(flags))
    for k, v in edit.items():
        setattr(ap, k, v)
    return ap


PRESETS = {
    "mono_lp": lambda: params(["-vhs-hifi", "0", "-vhs-speed", "lp"]),       # mono linear LP
    "stereo_hifi": lambda: params([]),
    "stereo_linear": lambda: params(["-vhs", "-vhs-hifi", "0"], channels=2),  # buzz and per-channel boost on two channels
    "no_hiss": lambda: params(["-audio-hiss", "-200"]),
    "nocomp": lambda: params(["-nocomp"]),
}

# 1, 1, 0, 4, 2, 7, 1 and 1 segments of 64: 17 in six wavefronts of three groups, the last with two live groups
STRADDLE = (64, 1, 0, 193, 128, 385, 2, 63)


def make_tracks(frames, channels, kinds="music", seed=40):
    """One int16 [sum(frames), channels] buffer, the tracks back to back with different content in each, so that a
    warm-up that crossed a boundary would change bits."""
    if isinstance(kinds, str):
        kinds = [kinds] * len(frames)
    parts = [A.make_input(k, f, channels, seed + 3 * t) for t, (f, k) in enumerate(zip(frames, kinds))]
    return np.concatenate(parts) if parts else np.zeros((0, channels), np.int16)


def cut(buf, frames):
    """views of the tracks in `buf` (numpy or torch, [frames, channels])"""
    out, at = [], 0
    for f in frames:
        out.append(buf[at:at + f])
        at += f
    return out


@functools.lru_cache(maxsize=None)
def checker(build="plain"):
    """Path of tests/audio_tracks_check.cpp built with g++ as tests/audio_chain_check.cpp is, once per session."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/audio_tracks_check.cpp"
    d = os.path.dirname(A.checker(build))                                       # the session's directory, cleaned up with it
    exe = os.path.join(d, "audio_tracks_check_" + build)
    csrc = os.path.join(L.PKG, "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + A._FLAGS[build] +
                          ["-I", csrc, "-I", os.path.join(L.ROOT, "include"), os.path.join(HERE, "audio_tracks_check.cpp"), os.path.join(csrc, "glibc_rand.cpp"), "-o", exe])
    return exe


def run_tracks_check(ap, audio, plan, states, split=False, rng_pos=0, build="plain"):
    """audio_tracks_check over the tracks (frames, state) of `states`: (return code, output)."""
    with tempfile.TemporaryDirectory(prefix="audio_tracks_") as d:
        cfg, inp = os.path.join(d, "cfg"), os.path.join(d, "in")
        A.write_cfg(cfg, ap)
        np.ascontiguousarray(audio).tofile(inp)
        spec = ",".join("%d:%s" % (f, s) for f, s in states)
        r = subprocess.run([checker(build), cfg, inp, str(plan[0]), str(plan[1]), str(int(split)), str(rng_pos), spec], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout
