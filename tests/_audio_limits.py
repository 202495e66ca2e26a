"""What tests/test_audio_limits_gpu.py and tests/test_audio_limits_host.py share: the block layouts that cross the launch
thresholds of the audio stages, and the plans whose repairs are MIXED -- found by search_mixed() on the host plan alone
(audio_run_planned / cass_run_planned through the checkers' `plan` modes), never from what the device gives."""
import numpy as np

import _audio_ref as A
import _audio_tracks as T
import _cass_ref as CR
from ntscsim import _capi

# ------------------------------------------------------------------------------------------------ calls in flight
def frames_of(calls):
    return sum(b[0] for c in calls for b in c)


def packet_calls():
    """The tool's packets with edges mixed in: 15 calls that take a record slot (each of the four at least three
    times) and one without frames.  The 12,000-frame call follows small ones (hiss / pulses / recs grow under them), the
    64-block call follows 1-block calls (its slot must be re-made: 176 B a block with hiss).  Three blocks carry a
    position, one of them backwards.  22,903 frames."""
    many = [(1 + i % 3, (1 << 33) + 9 if i == 40 else None) for i in range(64)]
    return [[(1152, None)], [(1, None)], [(1024, 500000)], [(0, None)], [(37, None)], [(1152, 100)], [(4097, None)], [(300, None)], [(12000, None)],
            [(5, None)], [(2, None)], many, [(1152, None)], [(700, None)], [(2, 77)], [(1152, None)]]


def tape_calls():
    """Runs of calls shorter than taps - 1 (1, 2, 3, 1 for 8 taps; 5 .. 3 for 57), so that the history a call reads is
    written by calls that have not run when it is enqueued; 3 frames and then 12,000, so that the tilt staging, tf, xs
    and rs are re-made with an upload pending."""
    return [[(1152, None)], [(1, None)], [(2, None)], [(3, None)], [(1, 900)], [(1024, None)], [(0, None)], [(5, None)], [(7, None)], [(10, 50)],
            [(20, None)], [(15, None)], [(3, None)], [(12000, None)], [(37, None)], [(1, None), (1, None), (2, 1 << 33)], [(1, None)], [(1152, None)]]


# ------------------------------------------------------------------------------------------------ B1: > 1024 blocks
HISS_GRID_Y = 1024                                                               # audio_hiss_launch: blocks of gridDim.y


def many_blocks(base=70000):
    """[(frames, rand() position or None)]: 1500 blocks of 1..5 frames and five without frames; every 100th block that
    has frames carries a position -- forwards, backwards, 2^33 away in turn -- and so does one block without frames."""
    blocks, k = [], 0
    for i in range(1500):
        n = 1 + (i * 7 + i // 3) % 5
        pos = None
        if i % 100 == 50:
            pos = (base + ((k // 3 + 1) << 33) + 17 * k, 1000 + k, base + 12345 * k)[k % 3]   # far, back, near
            k += 1
        blocks.append((n, pos))
        if i in (0, 299, 300, 1023, 1499):
            blocks.append((0, (1 << 34) + 5 if i == 1023 else None))             # block 1024 with frames starts where this one says
    return blocks


def first_draws(blocks, channels, pos, hiss=True):
    """the rand() position of every block's first draw, as the stages count them"""
    out = []
    for n, p in blocks:
        pos = pos if p is None else p
        out.append(pos)
        if hiss:
            pos += n * channels
    return out, pos


def spread(blocks, tracks):
    """the blocks dealt to `tracks` tracks in order, in runs of unequal length"""
    cuts = [len(blocks) * t // tracks + (3 if 0 < t < tracks and t % 2 else 0) for t in range(tracks + 1)]
    return [blocks[cuts[t]:cuts[t + 1]] for t in range(tracks)]


# ------------------------------------------------------------------------------------------------ B3: step or jump
HISS_STEP_MAX = 65536                                                            # audio_hiss_window steps up to this many draws, jumps beyond


def boundary_blocks():
    """Mono.  [(frames, position or None)] whose first draws lie 0, 1, 65535, 65536, 65537 draws apart and 1 draw back,
    then NTSCSIM_RNG_AUTO behind a block of exactly 65536 and of exactly 65537 draws; 140,000 frames."""
    p = 1000
    blocks = [(300, p)]
    for gap in (0, 1, 65535, 65536, 65537, -1):
        p += gap
        blocks.append((300, p))
    blocks += [(65536, None), (700, None), (65537, None), (700, None)]
    blocks.append((140000 - sum(n for n, _ in blocks), None))
    return blocks


# ------------------------------------------------------------------------------------------------ B6: mixed repairs
def alternating(frames, channels, seed, stretch):
    """`loud` and `quiet` stretches in turn: the loud ones leave the slow poles far from where a zero state gets in a
    marginal warm-up, the quiet ones let them meet"""
    parts, at, k = [], 0, 0
    while at < frames:
        n = min(stretch, frames - at)
        parts.append(A.make_input("loud" if k % 2 == 0 else "quiet", n, channels, seed + k))
        at += n
        k += 1
    return np.concatenate(parts)


MIXED_SEG = 256
MIXED_FRAMES = 8192                                                              # 32 segments
# the audio chain, 100 Hz high-pass (default warm-up 5056): W found by search_mixed("audio") in 1000 .. 6000
MIXED_AUDIO = {"preset": "stereo_linear", "seed": 3, "stretch": 2500, "warmup": 3750, "rng_pos": 5}
# the cassette, 100 Hz high-pass, 37 taps: the front's W and the back's found by search_mixed("cass"); the back's plan does
# not depend on the front's (the front's repairs leave the true x behind)
MIXED_CASS = {"flags": ["-preset", "1", "-mono", "-preemphasis", "1", "-deemphasis", "1"], "seed": 3, "stretch": 1500, "front": 3750, "back": 46,
              "rng_pos": 5}
# a tracks call: the middle track is MIXED_AUDIO's input; its neighbours are no longer than W + L, so that every one of
# their segments starts at the track's first frame from the carried state and none can need a repair
# (search_mixed("tracks") finds W for the middle track at the position the first track leaves the stream at)
MIXED_TRACKS = {"neighbours": (3000, 2900), "kinds": ("music", "loud"), "seed": 50, "warmup": 3750, "rng_pos": 5}


def mixed_audio_case():
    ap = T.PRESETS[MIXED_AUDIO["preset"]]()
    return ap, alternating(MIXED_FRAMES, ap.channels, MIXED_AUDIO["seed"], MIXED_AUDIO["stretch"])


def mixed_cass_case():
    cp = _capi.make_cass_params(MIXED_CASS["flags"])
    return cp, alternating(MIXED_FRAMES, 2, MIXED_CASS["seed"], MIXED_CASS["stretch"])


def mixed_tracks_case():
    """(params, [tracks], [rand() position of each track's first draw])"""
    ap, mid = mixed_audio_case()
    n0, n1 = MIXED_TRACKS["neighbours"]
    k0, k1 = MIXED_TRACKS["kinds"]
    tracks = [A.make_input(k0, n0, ap.channels, MIXED_TRACKS["seed"]), mid, A.make_input(k1, n1, ap.channels, MIXED_TRACKS["seed"] + 1)]
    pos, at = [], MIXED_TRACKS["rng_pos"]
    for a in tracks:
        pos.append(at)
        at += len(a) * ap.channels if ap.hiss_level else 0
    return ap, tracks, pos


def search_mixed(which, warmups=range(1000, 6001, 250), backs=range(1, 64, 3)):
    """How the plans above were found: every warm-up whose host plan meets A.mixed_repairs, with the repaired segments."""
    found = []
    if which == "audio":
        ap, a = mixed_audio_case()
        for w in warmups:
            (segs, _), rep = A.plan(ap, a, MIXED_SEG, w, rng_pos=MIXED_AUDIO["rng_pos"])
            if A.mixed_repairs(segs, rep):
                found.append((w, rep))
    elif which == "tracks":
        ap, tracks, pos = mixed_tracks_case()
        for w in warmups:
            (segs, _), rep = A.plan(ap, tracks[1], MIXED_SEG, w, rng_pos=pos[1])
            if A.mixed_repairs(segs, rep):
                found.append((w, rep))
    else:
        cp, a = mixed_cass_case()
        for w in warmups:
            st, front, _ = CR.plan(cp, a, MIXED_SEG, w, 64, rng_pos=MIXED_CASS["rng_pos"])
            if A.mixed_repairs(st[0], front):
                found.append(("front", w, front))
        for w in backs:
            st, _, back = CR.plan(cp, a, MIXED_SEG, max(warmups), w, rng_pos=MIXED_CASS["rng_pos"])
            if A.mixed_repairs(st[0], back):
                found.append(("back", w, back))
    return found
