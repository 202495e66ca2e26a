#!/usr/bin/env python3
"""Speed of the frameblend stage (ntscsim_blend_frames_device) on the GPU, beside its yardstick: a device-to-device
hipMemcpyAsync of the same number of bytes, same process, same buffers, same run.

Workload: N output frames (default 600) from a 24000/1001 clip resident in HBM to 60000/1001 -- the 2-tap fast form
(four periods in five fall inside one source frame and have a single tap: the plan is the tool's).  Cases:
720x486 with -gamma ntsc, 1920x1080 with -gamma ntsc, 720x486 without gamma.

Per case: the launch is timed with device events (median of --reps runs after --warmup runs; the descriptor array is
built once, so a run is the C call alone: record upload + one kernel).  Algorithmic bytes per output frame are
4*W*H*(taps + 1); frac_hbm = bytes / time / 8 TB/s, as roofline.frac elsewhere in this repository.  The copy moves
that many bytes from the source clip into the output buffer (hipMemcpyAsync, device to device, in pieces no larger
than either buffer), and `copy_half` half of them -- a copy of n bytes reads n and writes n, so the half-size copy is
the one with the kernel's memory traffic.

Before a case's numbers are printed, output frames 0, 1, the middle one and the last are compared with the checker
(tools/bench_verify.py; --no-verify skips it) as the last timed call left them, before the second copy overwrites them;
`frames_verified` and `verify_s` say what was compared.

    python tools/bench_blend.py [--frames 600] [--reps 20] [--warmup 5] [--ref-cpu-fps X] [--out profiles/blend.json]

--ref-cpu-fps records the reference's own pixel loop as measured elsewhere (tests/golden/make_golden_frameblend.py
--bench on the build machine's CPU: one thread, 720x486, 2 taps, gamma): a different host, labelled as such."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "composite-video-simulator_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_verify as V  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def hip_runtime():
    """The HIP runtime torch has loaded (one runtime per process: ntscsim/_capi.py, lib())."""
    try:
        return C.CDLL("libamdhip64.so")
    except OSError:
        for line in open("/proc/self/maps"):
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
        raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ref-cpu-fps", type=float, default=None)
    ap.add_argument("--out", default=None)
    V.add_argument(ap)
    a = ap.parse_args()

    import torch
    import ntscsim
    if not torch.cuda.is_available():
        sys.exit("bench_blend.py needs a GPU")
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3
    stream = torch.cuda.Stream()
    result = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "reps": a.reps, "warmup": a.warmup,
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "cases": {}}

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    for name, (w, h, flags) in {"720x486_gamma": (720, 486, ("-gamma", "ntsc")),
                                "1920x1080_gamma": (1920, 1080, ("-gamma", "ntsc")),
                                "720x486_plain": (720, 486, ())}.items():
        fb = ntscsim.FrameBlender(flags)
        nsrc = (a.frames * 2 + 4) // 5 + 2
        times = fb.frame_times(nsrc, 24000, 1001)
        plan = fb.plan(times, 0, a.frames)
        with torch.cuda.stream(stream):
            src = torch.randint(0, 256, (nsrc, h, w, 4), dtype=torch.uint8, device="cuda")
            out = torch.zeros((a.frames, h, w, 4), dtype=torch.uint8, device="cuda")
        stream.synchronize()
        jobs = [(out[k], [(src[i], wt) for i, wt in zip(ids, w16)]) for k, (ids, w16) in enumerate(plan)]
        arr, keep = fb._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))
        taps = sum(len(ids) for ids, _ in plan)
        nbytes = 4 * w * h * (taps + a.frames)
        sh = C.c_void_p(stream.cuda_stream)

        def run_blend():
            rc = fb._lib.ntscsim_blend_frames_device(fb.sim._h, arr, len(jobs), sh)
            if rc != 0:
                raise RuntimeError("ntscsim_blend_frames_device: %d" % rc)

        def copier(total):
            piece = min(src.numel(), out.numel())

            def run():
                left = total
                while left > 0:
                    n = min(left, piece)
                    if hip.hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), n, D2D, sh) != 0:
                        raise RuntimeError("hipMemcpyAsync failed")
                    left -= n
            return run

        # the copies first and last, the kernel between them: drift of the clock shows as a difference of the two
        c0 = timed(copier(nbytes))
        k = timed(run_blend)
        kernels = fb.last_kernels()
        verified = {}
        if not a.no_verify:                                                       # what the timed calls left, before the copy overwrites it
            import _blend_ref as RB
            verified = V.verify_frames(a.frames, lambda k: RB.blend_frame((h, w), [src[i].cpu().numpy() for i in plan[k][0]], plan[k][1],
                                                                          2.2 if flags else None),
                                       lambda k: out[k].cpu().numpy(), name)
        c1 = timed(copier(nbytes))
        ch = timed(copier(nbytes // 2))
        copy_ms = 0.5 * (c0[0] + c1[0])
        case = {
            "width": w, "height": h, "gamma": bool(flags), "kernels": kernels, "taps_total": taps,
            "algorithmic_bytes": nbytes,
            "blend_ms": k[0], "blend_ms_min_max": [k[1], k[2]],
            "frames_per_s": a.frames / (k[0] * 1e-3),
            "bytes_per_s": nbytes / (k[0] * 1e-3),
            "frac_hbm": nbytes / (k[0] * 1e-3) / HBM_BYTES_PER_S,
            "copy_same_bytes_ms": copy_ms, "copy_same_bytes_ms_runs": [c0[0], c1[0]],
            "copy_frac_hbm": nbytes / (copy_ms * 1e-3) / HBM_BYTES_PER_S,
            "copy_half_ms": ch[0],
            "blend_over_copy": k[0] / copy_ms,
            "blend_over_copy_half": k[0] / ch[0],
        }
        case.update(verified)
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        fb.close()
        del src, out, jobs, arr, keep
        torch.cuda.empty_cache()
    if a.ref_cpu_fps is not None:
        result["reference_cpu"] = {
            "what": "the reference's own pixel loop (frameblend.cpp:1032-1056), one thread, 720x486, 2 taps, gamma 2.2",
            "host": "the build machine's CPU, not the GPU host: a different machine",
            "frames_per_s": a.ref_cpu_fps,
        }
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
