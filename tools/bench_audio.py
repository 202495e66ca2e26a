#!/usr/bin/env python3
"""Speed of the audio stage (ntscsim_audio_device) on the GPU.

Inputs, resident in HBM: 10 s (441,000 frames) and 10 min of stereo Hi-Fi at the default preset, 10 s of linear mono SP
(-vhs -vhs-hifi 0: buzz, boost, hiss level 39).  Sine sums with noise, loud enough to be music, not loud enough to clip.

Per input the call is timed with device events (median of --reps runs after --warmup runs, the state reset in front of
every run, outside its events) at the default plan and -- for the 10 s inputs -- at the serial plan (one segment:
seg_len >= the call's frames) of the same kernel in the same run; their ratio is what the speculation is worth.  The
10 s Hi-Fi input also runs at segment lengths 1,024 .. 32,768 with the default warm-up: the default length is chosen
from that.  The kernels' own times come from ntscsim_audio_debug_kernel_ms in a further timed run; segments and
repaired segments from ntscsim_audio_debug_stats.

Verified before a number is printed: the default plan's output and final state equal the serial plan's (10 s inputs),
and the 10 s outputs equal the header's serial loop on the host (vhsaudio_cli --host), whose wall time -- one core of
the GPU host, reading and writing the file included -- is recorded beside them.

Next to the audio: 600 -vhs fields of 720x486 through ntscsim_fields_device in the same run, the video that goes with
10 s of audio.

    python tools/bench_audio.py [--reps 5] [--warmup 2] [--minutes 10] [--ref-cpu-s X] [--out profiles/audio.json]

--ref-cpu-s records the reference's own loop (ffmpeg_ntsc.cpp:901-970) on the 10 s stereo input as measured elsewhere:
one core of the build machine's CPU -- a different host, labelled as such."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "composite-video-simulator_amd")
sys.path.insert(0, PKG)

RATE = 44100


def make_track(torch, frames, channels, seed):
    """int16 [frames, channels] on the GPU"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = torch.empty((frames, channels), dtype=torch.int16, device="cuda")
    step = 1 << 22
    for at in range(0, frames, step):
        n = min(step, frames - at)
        t = torch.arange(at, at + n, device="cuda", dtype=torch.float64) / RATE
        for c in range(channels):
            s = 6000 * torch.sin(6.283185307179586 * (220.0 + 13 * c) * t) + 3500 * torch.sin(6.283185307179586 * (1318.5 + 7 * c) * t)
            s += 1800 * torch.sin(6.283185307179586 * (6271.9 - 11 * c) * t) + 200 * (torch.rand(n, device="cuda", generator=g, dtype=torch.float64) - 0.5)
            out[at:at + n, c] = s.to(torch.int16)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--ref-cpu-s", type=float, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    import ntscsim
    from ntscsim import _capi
    if not torch.cuda.is_available():
        sys.exit("bench_audio.py needs a GPU")
    stream = torch.cuda.Stream()
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "rate": RATE, "cases": {}}

    def timed(fn, before=None, reps=None):
        ms = []
        for i in range(a.warmup + (reps or a.reps)):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    sim = ntscsim.FieldSimulator(params=_capi.make_params(["-vhs"]), device=0)
    inputs = (("hifi_10s", [], 10 * RATE, True, True), ("linear_sp_10s", ["-vhs", "-vhs-hifi", "0"], 10 * RATE, True, False),
              ("hifi_%gmin" % a.minutes, [], int(a.minutes * 60 * RATE), False, False))
    for name, flags, frames, serial_too, sweep in inputs:
        chain = ntscsim.AudioChain(flags=flags, sim=sim)
        ch = chain.channels
        with torch.cuda.stream(stream):
            src = make_track(torch, frames, ch, 7)
            dst = torch.zeros_like(src)
        stream.synchronize()

        def reset():
            chain.reset()
            sim.rng_pos = 0

        def run():
            chain.process(src, dst, stream=stream.cuda_stream)

        def plan(seg_len, warmup):
            chain.set_plan(seg_len, warmup)
            t = timed(run, before=reset)
            chain.debug_time_kernels(True)
            reset()
            run()
            stream.synchronize()
            k = chain.kernel_ms()
            chain.debug_time_kernels(False)
            seg, rep = chain.stats()
            t.update({"kernel_ms": {"draws_and_pulses": k[0], "k_audio_segments": k[1], "k_audio_verify_repair": k[2]}, "segments": seg,
                      "repaired": rep, "seg_len": seg_len or 4096, "warmup": warmup or chain.default_warmup(),
                      "frames_per_s": frames / (t["ms"] * 1e-3), "times_real_time": frames / RATE / (t["ms"] * 1e-3)})
            return t

        case = {"flags": flags, "frames": frames, "channels": ch, "seconds_of_audio": frames / RATE, "default_plan": plan(0, 0)}
        want, want_state = dst.clone(), chain.state
        if sweep:
            case["segment_length_sweep"] = {}
            for seg_len in (1024, 2048, 4096, 8192, 16384, 32768):
                case["segment_length_sweep"][str(seg_len)] = plan(seg_len, chain.default_warmup())
                if not torch.equal(dst, want) or chain.state != want_state:
                    sys.exit("%s: segment length %d changes the result" % (name, seg_len))
        if serial_too:
            a_reps, a.reps = a.reps, 1
            a_warm, a.warmup = a.warmup, 0
            case["serial_plan"] = plan(frames, 0)
            a.reps, a.warmup = a_reps, a_warm
            if not torch.equal(dst, want) or chain.state != want_state:
                sys.exit("%s: the serial plan and the default plan differ" % name)
            case["speculation_speedup"] = case["serial_plan"]["ms"] / case["default_plan"]["ms"]
            case["serial_plan_ns_per_channel_sample"] = case["serial_plan"]["kernel_ms"]["k_audio_segments"] * 1e6 / (frames * ch)
            # the header's serial loop on the host, through the command line tool
            with tempfile.TemporaryDirectory(prefix="bench_audio_") as d:
                inp, outp = os.path.join(d, "in.s16"), os.path.join(d, "out.s16")
                src.cpu().numpy().tofile(inp)
                t0 = time.time()
                subprocess.check_call([os.path.join(PKG, "vhsaudio_cli"), "--host"] + flags + ["-i", inp, "-o", outp], stderr=subprocess.DEVNULL)
                case["host_serial_loop_s"] = time.time() - t0
                host = np.fromfile(outp, np.int16).reshape(frames, ch)
            if not (host == want.cpu().numpy()).all():
                sys.exit("%s: the device and the host loop differ" % name)
            case["verified"] = "default plan == serial plan == host loop, bytes and state"
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        del src, dst, want
        torch.cuda.empty_cache()

    # the video that goes with 10 s of audio: 600 -vhs fields
    w, h, n = 720, 486, 600
    with torch.cuda.stream(stream):
        vsrc = torch.randint(0, 256, (2, h, w, 4), dtype=torch.uint8, device="cuda")
        vdst = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
    stream.synchronize()
    jobs = [(k & 1, k, (k & 1) ^ 1, k) for k in range(n)]
    sim.fields(vsrc, vdst, jobs)
    sim.sync()
    t0 = time.time()
    for _ in range(a.reps):
        sim.fields(vsrc, vdst, jobs)
    sim.sync()
    video_ms = (time.time() - t0) * 1e3 / a.reps
    audio_ms = result["cases"]["hifi_10s"]["default_plan"]["ms"]
    result["video_600_vhs_fields_720x486_ms"] = video_ms
    result["audio_10s_over_video_600_fields"] = audio_ms / video_ms
    result["longer_of_the_two"] = "audio" if audio_ms > video_ms else "video"
    if a.ref_cpu_s is not None:
        result["reference_cpu"] = {"what": "the reference's own loop (ffmpeg_ntsc.cpp:901-970), one core, 10 s of stereo Hi-Fi at the default preset",
                                   "host": "the build machine's CPU, not the GPU host: a different machine", "seconds": a.ref_cpu_s}
    sim.close()
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
