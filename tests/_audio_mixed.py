"""What the mixed-track audio tests share: the presets (those of _audio_tracks plus a PAL twin of stereo_linear and a
louder hiss), the expectation -- the serial checker per track with that track's parameters, the rand() position chained
through -- and the host program tests/audio_mixed_tracks_check.cpp over csrc/audio_chain.hpp, built once per session."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import _audio_ref as A
import _audio_tracks as T
import _libs as L

HERE = os.path.dirname(os.path.abspath(__file__))

PRESETS = dict(T.PRESETS)
PRESETS["pal_linear"] = lambda: T.params(["-tvstd", "pal", "-vhs", "-vhs-hifi", "0"], channels=2)   # stereo_linear's PAL twin
PRESETS["loud_hiss"] = lambda: T.params(["-audio-hiss", "-30"])                                      # stereo_hifi, another level

# the cycle of test 2: mono and stereo, NTSC buzz, PAL buzz and none, hiss and none, a copied track
CYCLE = ("mono_lp", "stereo_hifi", "stereo_linear", "no_hiss", "nocomp", "pal_linear")


def sets_of(names):
    return [PRESETS[n]() for n in names]


def make_tracks(frames, sets, set_of, kinds="music", seed=40):
    """One int16 array [frames[t], channels of track t's set] per track, with different content in each."""
    if isinstance(kinds, str):
        kinds = [kinds] * len(frames)
    return [A.make_input(k, f, sets[s].channels, seed + 3 * t) for t, (f, k, s) in enumerate(zip(frames, kinds, set_of))]


def expect(sets, set_of, tracks, counts=None, pos=0, blocks=None):
    """A.run_checker per track with that track's parameters, in order, the rand() position running through:
    ([(output, (values, count))], position).  A copied track (enabled == 0) draws nothing, sets no position and keeps
    its state."""
    out = []
    for t, a in enumerate(tracks):
        ap = sets[set_of[t]]
        cut = blocks[t] if blocks is not None and blocks[t] is not None else None
        count0 = counts[t] if counts else 0
        if not ap.enabled:
            out.append((a, None))
            continue
        if len(a) == 0:
            out.append((a, (tuple([0.0] * 30), count0)))
            for _n, p in (cut or []):
                pos = pos if p is None else p                                   # a block without samples still sets the position
            continue
        want, st, pos = A.run_checker(ap, a, count0=count0, rng_pos=pos, block=("blocks=" + A.block_spec(cut)) if cut else 0)
        out.append((want, st))
    return out, pos


@functools.lru_cache(maxsize=None)
def checker(build="plain"):
    """Path of tests/audio_mixed_tracks_check.cpp built with g++ as tests/audio_tracks_check.cpp is, once per session."""
    assert shutil.which("g++") is not None, "g++ is needed to build tests/audio_mixed_tracks_check.cpp"
    d = os.path.dirname(A.checker(build))                                       # the session's directory, cleaned up with it
    exe = os.path.join(d, "audio_mixed_tracks_check_" + build)
    csrc = os.path.join(L.PKG, "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + A._FLAGS[build] +
                          ["-I", csrc, "-I", os.path.join(L.ROOT, "include"), os.path.join(HERE, "audio_mixed_tracks_check.cpp"),
                           os.path.join(csrc, "glibc_rand.cpp"), "-o", exe])
    return exe


def run_mixed_check(sets, set_of, tracks, plan, states=None, rng_pos=0, build="plain"):
    """audio_mixed_tracks_check over the tracks: (return code, output)."""
    with tempfile.TemporaryDirectory(prefix="audio_mixed_") as d:
        cfgs = []
        for i, ap in enumerate(sets):
            cfgs.append(os.path.join(d, "cfg%d" % i))
            A.write_cfg(cfgs[-1], ap)
        inp = os.path.join(d, "in")
        np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in tracks] + [np.zeros(0, np.int16)]).tofile(inp)
        spec = ",".join("%d:%d:%s" % (len(a), s, st) for a, s, st in zip(tracks, set_of, states or ["z"] * len(tracks)))
        r = subprocess.run([checker(build), inp, str(plan[0]), str(plan[1]), str(rng_pos), spec] + cfgs, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout
