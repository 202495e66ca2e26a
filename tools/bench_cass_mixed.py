#!/usr/bin/env python3
"""Speed of many independent cassette tracks WITH PARAMETERS PER TRACK in one call (ntscsim_cass_mixed_tracks_device).

Inputs, resident in HBM: 64 stereo tracks of 10 s (441,000 frames each) over 4 sets -- the default deck (8 taps), -preset 3
(57 taps), both emphasis filters, mono at -high 100 -- 16 tracks each, the tracks of a set next to each other so that leg
(a) draws at the same rand() positions, cut back to back from one buffer made like tools/bench_audio.py's, all starting
at sample count 0 -- so the table of sines of the mixed call is ONE track long.

In the same run:
  mixed    one mixed call over the 64 tracks, each with its own state (device events, median of --reps after --warmup; the
           host's sin() fill runs inside it; the states zeroed and the rand() position reset in front of every run, outside
           its events)
  (a)      the same tracks as one ntscsim_cass_bind + ntscsim_cass_tracks_device per set, which is what a caller had to do
           before: wall clock, because bind's wait for the device is the point
  (b)      64 tracks all on ONE set (the default deck) through the mixed call, and the same through
           ntscsim_cass_tracks_device: the mixed kernels against the uniform ones on a uniform call
and the kernels' own times from ntscsim_cass_debug_kernel_ms in a further run, the host fill's time with the sines it
evaluated (ntscsim_cass_debug_tilt_frames), segments and repaired segments from the stats tap.

Verified before a number is printed: the buffers hold --tracks tracks of the full length; the mixed call's output and end
states equal (a)'s, and (b)'s two forms equal each other, track by track.

    python tools/bench_cass_mixed.py [--tracks 64] [--seconds 10] [--reps 5] [--warmup 2] [--out profiles/cass_mixed_tracks.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "composite-video-simulator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_audio import RATE, make_track  # noqa: E402

SETS = (("default", []), ("preset3", ["-preset", "3"]), ("emphasis", ["-deemphasis", "1", "-preemphasis", "1"]), ("mono_high100", ["-mono", "-high", "100"]))
SLOTS = ("host_sin_fill", "sines_upload", "k_audio_hiss", "front", "front_verify", "conv", "back", "back_verify")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    import ntscsim
    from ntscsim import _capi
    if not torch.cuda.is_available():
        sys.exit("bench_cass_mixed.py needs a GPU")
    stream = torch.cuda.Stream()
    n, frames = a.tracks, int(a.seconds * RATE)
    assert n % len(SETS) == 0
    per = n // len(SETS)
    sets = [_capi.make_cass_params(flags) for _name, flags in SETS]
    set_of = [t // per for t in range(n)]
    counts = [0] * n
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rate": RATE, "tracks": n, "frames_per_track": frames,
              "sets": [s[0] for s in SETS], "taps": [int(s.taps) for s in sets], "seconds_of_audio": n * frames / RATE}

    def events(fn, before):
        ms = []
        for i in range(a.warmup + a.reps):
            before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    def wall(fn, before):
        ms = []
        for i in range(a.warmup + a.reps):
            before()
            stream.synchronize()
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    sim = ntscsim.FieldSimulator(device=0)
    chain = ntscsim.Cassette(sets[0], sim=sim)
    with torch.cuda.stream(stream):
        src = make_track(torch, n * frames, 2, 7)
        dst = torch.zeros_like(src)
        dst_a = torch.zeros_like(src)
        states = chain.zero_states(n)
        states_a = chain.zero_states(n)
    stream.synchronize()
    srcs = [src[t * frames:(t + 1) * frames] for t in range(n)]
    dsts = [dst[t * frames:(t + 1) * frames] for t in range(n)]
    dsts_a = [dst_a[t * frames:(t + 1) * frames] for t in range(n)]
    if src.numel() != n * frames * 2 or len(srcs) != n or any(x.numel() != frames * 2 for x in srcs + dsts + dsts_a):
        sys.exit("the buffers do not hold %d tracks of %d frames" % (n, frames))
    result["buffer_tracks"] = src.numel() // (frames * 2)

    def reset():
        with torch.cuda.stream(stream):
            states.zero_()
            states_a.zero_()
        sim.rng_pos = 0

    def run_mixed():
        chain.process_mixed_tracks(sets, set_of, srcs, dsts, counts, states, stream=stream.cuda_stream)

    def run_per_set():                                                          # (a)
        for s in range(len(sets)):
            c = ntscsim.Cassette(sets[s], sim=sim)                              # ntscsim_cass_bind
            lo, hi = s * per, (s + 1) * per
            c.process_tracks(srcs[lo:hi], dsts_a[lo:hi], counts[lo:hi], states_a[lo * c.STATE_BYTES:hi * c.STATE_BYTES], stream=stream.cuda_stream)

    def kernels(fn, prefix):
        chain.debug_time_kernels(True)
        reset()
        fn()
        stream.synchronize()
        k = chain.kernel_ms()
        chain.debug_time_kernels(False)
        return {(name if i < 3 else prefix + name): v for i, (name, v) in enumerate(zip(SLOTS, k))}

    def totals(case):
        stats = chain.track_stats(n)
        case.update({"tilt_frames": chain.tilt_frames(), "segments": sum(s[0] for s in stats), "repaired_front": sum(s[1] for s in stats),
                     "repaired_back": sum(s[2] for s in stats)})

    case = events(run_mixed, reset)
    case["kernel_ms"] = kernels(run_mixed, "k_cass_mixed_")
    totals(case)
    end_states = states.clone()                                                 # reset() zeroes the tensor in front of (a)
    result["mixed_call"] = case
    result["a_one_bind_and_tracks_call_per_set"] = wall(run_per_set, reset)
    if not torch.equal(dst, dst_a) or not torch.equal(end_states, states_a):
        sys.exit("the mixed call differs from one tracks call per set (%d samples, end states %s)" % (
            int((dst != dst_a).sum()), "equal" if torch.equal(end_states, states_a) else "differ"))
    result["verified"] = "mixed call == one bind + tracks call per set, bytes and end states, every track"
    result["a_over_mixed"] = result["a_one_bind_and_tracks_call_per_set"]["ms"] / case["ms"]
    result["times_real_time"] = n * frames / RATE / (case["ms"] * 1e-3)
    print("mixed", json.dumps(result), flush=True)

    # (b): a uniform call through both kernel families
    chain = ntscsim.Cassette(sets[0], sim=sim)

    def run_uniform_mixed():
        chain.process_mixed_tracks([sets[0]], [0] * n, srcs, dsts, counts, states, stream=stream.cuda_stream)

    def run_uniform_tracks():
        chain.process_tracks(srcs, dsts_a, counts, states_a, stream=stream.cuda_stream)

    b = {"set": SETS[0][0], "tracks": len(srcs)}
    b["mixed_call"] = events(run_uniform_mixed, reset)
    b["mixed_call"]["kernel_ms"] = kernels(run_uniform_mixed, "k_cass_mixed_")
    totals(b["mixed_call"])
    end_states = states.clone()
    b["tracks_call"] = events(run_uniform_tracks, reset)
    b["tracks_call"]["kernel_ms"] = kernels(run_uniform_tracks, "k_cass_track_")
    totals(b["tracks_call"])
    if not torch.equal(dst, dst_a) or not torch.equal(end_states, states_a):
        sys.exit("(b): the mixed call on one set differs from the tracks call")
    b["verified"] = "mixed call on one set == tracks call, bytes and end states"
    b["mixed_over_tracks"] = b["mixed_call"]["ms"] / b["tracks_call"]["ms"]
    result["b_all_tracks_on_one_set"] = b
    sim.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
