#!/usr/bin/env python3
"""Speed of many independent cassette tracks in one call (ntscsim_cass_tracks_device) on the GPU.

Inputs, resident in HBM: 64 stereo tracks of 10 s (441,000 frames each), cut back to back from one buffer made like
tools/bench_audio.py's, all starting at sample count 0 -- so the tilt table of the tracks call is ONE track long.  Four
cases: the default tilt (8 taps) and -preset 3 (57 taps), de-emphasis off and on.

Per case, in the same run:
  tracks   one tracks call over the 64 tracks, each with its own state (device events around the call, median of --reps
           after --warmup; the host's sin() fill runs inside it; the states zeroed and the rand() position reset in front
           of every run, outside its events)
  (a)      the same tracks as 64 ntscsim_cass_device calls with ntscsim_cass_set_state / ntscsim_cass_get_state between
           them, which is what a caller had to do before: wall clock, because the waits of set / get for the device are
           the point
  (b)      one ntscsim_cass_device call over a single track of the same total length (device events)
and the kernels' own times of the tracks call and of (b) from ntscsim_cass_debug_kernel_ms in a further run, the host
fill's time with the sines it evaluated (ntscsim_cass_debug_tilt_frames), segments and repaired segments.

Verified before a number is printed: the tracks call's output and end states equal (a)'s, track by track.

    python tools/bench_cass_tracks.py [--tracks 64] [--seconds 10] [--reps 5] [--warmup 2] [--out profiles/cass_tracks.json]"""
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

SINGLE = ("host_sin_fill", "tilt_upload", "k_audio_hiss", "k_cass_front", "k_cass_front_verify", "k_cass_conv", "k_cass_back", "k_cass_back_verify")
TRACKS = ("host_sin_fill", "tilt_upload", "k_audio_hiss", "k_cass_track_front", "k_cass_track_front_verify", "k_cass_track_conv", "k_cass_track_back",
          "k_cass_track_back_verify")
CASES = (("taps8", []), ("taps8_deemph", ["-deemphasis", "1"]), ("taps57", ["-preset", "3"]), ("taps57_deemph", ["-preset", "3", "-deemphasis", "1"]))


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
    if not torch.cuda.is_available():
        sys.exit("bench_cass_tracks.py needs a GPU")
    stream = torch.cuda.Stream()
    n, frames = a.tracks, int(a.seconds * RATE)
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rate": RATE, "tracks": n, "frames_per_track": frames,
              "cases": {}}

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
    with torch.cuda.stream(stream):
        src = make_track(torch, n * frames, 2, 7)
        dst = torch.zeros_like(src)
        dst_a = torch.zeros_like(src)
    stream.synchronize()
    srcs = [src[t * frames:(t + 1) * frames] for t in range(n)]
    dsts = [dst[t * frames:(t + 1) * frames] for t in range(n)]
    dsts_a = [dst_a[t * frames:(t + 1) * frames] for t in range(n)]
    counts = [0] * n
    for name, flags in CASES:
        chain = ntscsim.Cassette(flags=flags, sim=sim)
        with torch.cuda.stream(stream):
            states = chain.zero_states(n)
        zero = (tuple([0.0] * 28), 0, tuple([(0.0, 0.0)] * (chain.taps - 1)))
        saved = [zero] * n

        def reset():
            with torch.cuda.stream(stream):
                states.zero_()
            chain.reset()
            sim.rng_pos = 0
            saved[:] = [zero] * n

        def run_tracks():
            chain.process_tracks(srcs, dsts, counts, states, stream=stream.cuda_stream)

        def run_calls():                                                        # (a)
            for t in range(n):
                chain.state = saved[t]
                chain.process(srcs[t], dsts_a[t], stream=stream.cuda_stream)
                saved[t] = chain.state

        def run_single():                                                       # (b)
            chain.process(src, dst_a, stream=stream.cuda_stream)

        def kernels(fn, names):
            chain.debug_time_kernels(True)
            reset()
            fn()
            stream.synchronize()
            k = chain.kernel_ms()
            chain.debug_time_kernels(False)
            return dict(zip(names, k))

        case = {"flags": flags, "taps": chain.taps, "seconds_of_audio": n * frames / RATE}
        case["tracks_call"] = events(run_tracks, reset)
        case["tracks_call"]["kernel_ms"] = kernels(run_tracks, TRACKS)
        case["tracks_call"]["tilt_frames"] = chain.tilt_frames()
        stats = chain.track_stats(n)
        end_states = [chain.track_state(states, t) for t in range(n)]           # reset() zeroes the tensor in front of (a)
        case["tracks_call"].update({"segments": sum(s[0] for s in stats), "repaired_front": sum(s[1] for s in stats),
                                    "repaired_back": sum(s[2] for s in stats)})
        case["a_one_call_per_track"] = wall(run_calls, reset)
        for t in range(n):                                                      # the last run of each stands in dst / dst_a
            if not torch.equal(dsts[t], dsts_a[t]) or end_states[t] != saved[t]:
                sys.exit("%s: track %d of the tracks call differs from its own ntscsim_cass_device call (%d samples, end state %s)" % (
                    name, t, int((dsts[t] != dsts_a[t]).sum()), "equal" if end_states[t] == saved[t] else "differs"))
        case["verified"] = "tracks call == one call per track, bytes and end states, every track"
        case["b_single_track_of_the_total_length"] = events(run_single, reset)
        case["b_single_track_of_the_total_length"]["kernel_ms"] = kernels(run_single, SINGLE)
        case["b_single_track_of_the_total_length"]["tilt_frames"] = chain.tilt_frames()
        seg, rf, rb = chain.stats()
        case["b_single_track_of_the_total_length"].update({"segments": seg, "repaired_front": rf, "repaired_back": rb})
        t_ms = case["tracks_call"]["ms"]
        case["a_over_tracks"] = case["a_one_call_per_track"]["ms"] / t_ms
        case["tracks_over_b"] = t_ms / case["b_single_track_of_the_total_length"]["ms"]
        case["times_real_time"] = n * frames / RATE / (t_ms * 1e-3)
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)
    sim.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
