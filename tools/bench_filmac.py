#!/usr/bin/env python3
"""Speed of the filmac stage (ntscsim_filmac_frames_device) on the GPU, beside its yardsticks: device-to-device
hipMemcpyAsync of the same memory traffic, same process, same buffers, same run.

Workload: N frames (default 600) resident in HBM, every frame a buffer of its own, at 720x486 and at 1920x1080, with
-gamma ntsc and without: noise whose band of values drifts from frame to frame, so that the levels move and the
recurrence takes all of its branches.  The clip goes through ONE call: five launches (k_filmac_stats, k_filmac_frame_levels,
k_filmac_levels, k_filmac_tables, k_filmac_apply) over all frames, the level state on the device throughout.

Per case the call is timed with device events (median of --reps runs after --warmup runs; the descriptor array is built
once, so a run is the C call alone).  Then the same call is timed again with events between its kernels
(ntscsim_filmac_debug_time_kernels): the time of each of the five kernels, the serial walk of k_filmac_levels among
them.  Two copies are the yardsticks: 8*W*H bytes of traffic per frame (a frame read once and written once: what the
stage would move if the map's read of the frame came from cache) and 12*W*H (the statistics pass reads the frame, the
map reads it again from memory).  The statistics pass reads only the blocks, columns width*15/100 to about width*90/100,
so `traffic_bytes` is smaller than 12*W*H; it is computed from the block grid and reported too.  Copies run first and
last, the stage between them.

Before a case's numbers are printed the last timed run is verified (tools/bench_verify.py; --no-verify skips it): the
state is reset in front of that run, outside its events; output frames 0, 1, the middle one and the last are compared
with the checker's map of the levels the device reports, those frames' own minv / maxv with the checker's, and the
recurrence of ALL frames is walked in Python on the reported minv / maxv and compared with the reported final levels
and with the state behind the clip.

    python tools/bench_filmac.py [--frames 600] [--reps 10] [--warmup 3] [--ref-cpu-fps X --ref-cpu-fps-gamma Y] [--out profiles/filmac.json]

--ref-cpu-fps / --ref-cpu-fps-gamma record the reference's own loop (filmac.cpp:857-1006) as measured elsewhere: one
thread, 720x486, on the build machine's CPU -- a different host, labelled as such."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "composite-video-simulator_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_verify as V  # noqa: E402
from bench_led import HBM_BYTES_PER_S, hip_runtime  # noqa: E402


def make_clip(torch, n, w, h, seed):
    """[n, h, w, 4] uint8 on the GPU: frame k is noise in [lo_k, lo_k + span_k)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    clip = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    step = max(1, (256 << 20) // (w * h * 4))
    for i in range(0, n, step):
        m = min(step, n - i)
        lo = torch.randint(0, 100, (m, 1, 1, 1), device="cuda", generator=g)
        span = torch.randint(40, 156, (m, 1, 1, 1), device="cuda", generator=g)
        noise = torch.rand((m, h, w, 4), device="cuda", generator=g)
        clip[i:i + m] = (lo + noise * span).to(torch.uint8)
    return clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-cpu-fps", type=float, default=None)
    ap.add_argument("--ref-cpu-fps-gamma", type=float, default=None)
    ap.add_argument("--out", default=None)
    V.add_argument(ap)
    a = ap.parse_args()

    import numpy as np
    import torch
    import ntscsim
    import _filmac_ref as RF
    if not torch.cuda.is_available():
        sys.exit("bench_filmac.py needs a GPU")
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3
    stream = torch.cuda.Stream()
    result = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "reps": a.reps, "warmup": a.warmup,
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "cases": {}}

    def timed(fn, before_last=None, each=None):
        ms = []
        for i in range(a.warmup + a.reps):
            if before_last is not None and i == a.warmup + a.reps - 1:
                before_last()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
                if each is not None:
                    each()
        return statistics.median(ms), min(ms), max(ms)

    for w, h in ((720, 486), (1920, 1080)):
        with torch.cuda.stream(stream):
            src = make_clip(torch, a.frames, w, h, 2000 + w)
            out = torch.zeros((a.frames, h, w, 4), dtype=torch.uint8, device="cuda")
        stream.synchronize()
        xs, ys = RF.block_origins(w, h)
        measured = (min(w, xs[-1] + RF.BLOCK) - xs[0]) * h                         # pixels the statistics pass reads
        frame_px = w * h
        sh = C.c_void_p(stream.cuda_stream)
        jobs = [(out[k], src[k]) for k in range(a.frames)]

        def copy(nbytes):
            def run():
                left = nbytes
                while left > 0:                                                    # 6*W*H*N bytes: the clip, then half of it again
                    m = min(left, 4 * frame_px * a.frames)
                    if hip.hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), m, D2D, sh) != 0:
                        raise RuntimeError("hipMemcpyAsync failed")
                    left -= m
            return run

        copy8, copy12 = copy(4 * frame_px * a.frames), copy(6 * frame_px * a.frames)
        for tag, flags in (("plain", []), ("gamma", ["-gamma", "ntsc"])):
            ac = ntscsim.AutoContrast(flags=flags, width=w, height=h)
            arr = ac._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))

            def run():
                rc = ac._lib.ntscsim_filmac_frames_device(ac.sim._h, arr, len(jobs), sh)
                if rc != 0:
                    raise RuntimeError("ntscsim_filmac_frames_device: %d" % rc)

            name = "%dx%d_%s" % (w, h, tag)
            c8a, c12a = timed(copy8), timed(copy12)
            with torch.cuda.stream(stream):
                out.zero_()
            k0 = timed(run)
            kernels = ac.last_kernels()
            per_kernel = []
            ac.debug_time_kernels(True)
            kt = timed(run, each=lambda: per_kernel.append(ac.kernel_ms()))
            ac.debug_time_kernels(False)
            k1 = timed(run, before_last=ac.reset)
            verified = {}
            if not a.no_verify:
                t0 = time.time()
                stream.synchronize()
                lv = [ac.levels(k) for k in range(a.frames)]
                s = RF.Stream(2.2 if flags else -1.0)
                for k in range(a.frames):
                    if s.step(lv[k][0], lv[k][1]) != (lv[k][2], lv[k][3]):
                        V.mismatch("%s: the recurrence at frame %d" % (name, k))
                    if k in V.sample_frames(a.frames):
                        f = src[k].cpu().numpy()
                        if s.frame_levels(f) != (lv[k][0], lv[k][1]):
                            V.mismatch("%s: minv / maxv of frame %d" % (name, k))
                        want = np.empty_like(f)
                        want[:, :, :3] = s.table()[f[:, :, :3]]
                        want[:, :, 3] = 0xFF
                        V.same(want, out[k].cpu().numpy(), "%s, output frame %d" % (name, k))
                if ac.state != (True, s.fmin, s.fmax):
                    V.mismatch("%s: the state behind the clip" % name)
                verified = {"frames_verified": V.sample_frames(a.frames), "recurrence_verified_frames": a.frames,
                            "branches": s.branches, "verify_s": time.time() - t0}
            c8b, c12b = timed(copy8), timed(copy12)
            ms, c8, c12 = 0.5 * (k0[0] + k1[0]), 0.5 * (c8a[0] + c8b[0]), 0.5 * (c12a[0] + c12b[0])
            kms = [statistics.median(p[i] for p in per_kernel) for i in range(5)]
            traffic = (8 * frame_px + 4 * measured) * a.frames
            case = {
                "width": w, "height": h, "gamma": bool(flags), "kernels": kernels,
                "blocks_per_frame": len(xs) * len(ys), "measured_fraction_of_frame": measured / frame_px,
                "filmac_ms": ms, "filmac_ms_runs": [k0[0], k1[0]], "filmac_ms_min_max": [min(k0[1], k1[1]), max(k0[2], k1[2])],
                "frames_per_s": a.frames / (ms * 1e-3),
                "kernel_ms": {"k_filmac_stats": kms[0], "k_filmac_frame_levels": kms[1], "k_filmac_levels": kms[2], "k_filmac_tables": kms[3], "k_filmac_apply": kms[4]},
                "kernel_ms_call_with_events": kt[0],
                "traffic_bytes": traffic, "frac_hbm": traffic / (ms * 1e-3) / HBM_BYTES_PER_S,
                "copy_8wh_ms": c8, "copy_8wh_ms_runs": [c8a[0], c8b[0]], "copy_8wh_ms_min_max": [min(c8a[1], c8b[1]), max(c8a[2], c8b[2])],
                "copy_12wh_ms": c12, "copy_12wh_ms_runs": [c12a[0], c12b[0]], "copy_12wh_ms_min_max": [min(c12a[1], c12b[1]), max(c12a[2], c12b[2])],
                "copy_frac_hbm": 8 * frame_px * a.frames / (c8 * 1e-3) / HBM_BYTES_PER_S,
                "filmac_over_copy_8wh": ms / c8, "filmac_over_copy_12wh": ms / c12,
                "apply_over_copy_8wh": kms[4] / c8,
            }
            case.update(verified)
            result["cases"][name] = case
            print(name, json.dumps(case), flush=True)
            ac.close()
        del src, out, jobs
        torch.cuda.empty_cache()
    if a.ref_cpu_fps is not None:
        result["reference_cpu"] = {
            "what": "the reference's own loop (filmac.cpp:857-1006), one thread, 720x486, noise frames",
            "host": "the build machine's CPU, not the GPU host: a different machine",
            "frames_per_s": a.ref_cpu_fps, "frames_per_s_gamma": a.ref_cpu_fps_gamma,
        }
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
