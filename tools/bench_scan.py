#!/usr/bin/env python3
"""Speed of the scanimate stage on the GPU.

Workload: a clip of N source frames (default 600) resident in HBM, one output field per frame through
ntscsim_scan_clip_device, field numbers from 0 -- so 180 fields each of the trapezoid, rotate and stretch effects and the
rest of the sine effect.  Configurations: the tool's 600x800 source to 720x480, the -inntsc 480x480 source to 720x480 and
to 1920x1080.  Sources hold uniform random bytes.

Per configuration: the whole clip in one call, and each effect's run of fields in a call of its own, timed with device
events (median of --reps runs after --warmup runs; the pointer arrays are built once).  Behind every call the splat
kernel's counters are read: workgroups that drew a dot, and the share of them that added to the accumulator plane
directly (spilled) instead of through the on-chip window.  For the first configuration the whole clip is also run with
the window switched off (ntscsim_scan_debug_set_window_rows(0): every add goes to the plane): the A/B the window has
to justify itself with.

Before a configuration's numbers are printed, output fields 0, 1, the middle one and the last are compared with the
checker (tools/bench_verify.py; --no-verify skips it) as the timed calls left them: behind the whole-clip and per-effect
runs, which all use the window, and -- first configuration -- once more behind the all-spill run, before the window is
switched back on.  `frames_verified` and `verify_s` of the case and of its `all_spill` entry say what was compared.

    python tools/bench_scan.py [--frames 600] [--reps 3] [--warmup 1] [--ref-cpu-fps X] [--out profiles/scan.json]

--ref-cpu-fps records the reference's own loop as measured elsewhere (ffmpeg_scanimate.cpp:817-974 compiled -O2, one
core, 600x800 -> 720x480): a different host unless measured on this one, and labelled by --ref-cpu-host."""
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

CONFIGS = [("600x800_to_720x480", [], 720, 480), ("inntsc_480x480_to_720x480", ["-inntsc"], 720, 480),
           ("inntsc_480x480_to_1920x1080", ["-inntsc", "-tvstd", "1080p60"], 1920, 1080)]
EFFECTS = ["trapezoid", "rotate", "stretch", "sine"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--configs", default=",".join(c[0] for c in CONFIGS))
    ap.add_argument("--ref-cpu-fps", type=float, default=None)
    ap.add_argument("--ref-cpu-host", default="the build machine's CPU, not the GPU host: a different machine")
    ap.add_argument("--out", default=None)
    V.add_argument(ap)
    a = ap.parse_args()

    import torch
    import ntscsim
    if not torch.cuda.is_available():
        sys.exit("bench_scan.py needs a GPU")
    stream = torch.cuda.Stream()
    T = a.frames
    result = {"device": torch.cuda.get_device_name(0), "frames": T, "reps": a.reps, "warmup": a.warmup, "cases": {}}

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

    sim = ntscsim.FieldSimulator(device=0)
    for name, flags, w, h in CONFIGS:
        if name not in a.configs.split(","):
            continue
        sc = ntscsim.Scanimator(flags, sim=sim)
        assert (int(sc.params.output_width), int(sc.params.output_height)) == (w, h)
        sw, sh = int(sc.params.src_width), int(sc.params.src_height)
        with torch.cuda.stream(stream):
            src = torch.randint(0, 256, (T, sh, sw, 4), dtype=torch.uint8, device="cuda")
            out = torch.zeros((T, h, w, 4), dtype=torch.uint8, device="cuda")
        stream.synchronize()
        shd = C.c_void_p(stream.cuda_stream)
        lib, hctx = sc._lib, sc.sim._h

        def clip(first, last):
            n = last - first
            sp = (C.c_void_p * n)(*[src[t].data_ptr() for t in range(first, last)])
            op = (C.c_void_p * n)(*[out[t].data_ptr() for t in range(first, last)])

            def run():
                fn = C.c_uint64(first)
                rc = lib.ntscsim_scan_clip_device(hctx, sp, 4 * sw, sw, sh, op, 4 * w, n, C.byref(fn), shd)
                if rc != 0:
                    raise RuntimeError("ntscsim_scan_clip_device: %d" % rc)
            return run

        def measure(first, last):
            k = timed(clip(first, last))
            wgs, spilled = sc.debug_spill()
            return {"fields": last - first, "ms": k[0], "ms_min_max": [k[1], k[2]], "fields_per_s": (last - first) / (k[0] * 1e-3),
                    "workgroups": wgs, "spilled_share": (spilled / wgs) if wgs else 0.0}

        wanted = {}

        def want(k, w=w, h=h, flags=flags):
            if k not in wanted:
                import _scan_ref as RS
                f = RS.scan_field(src[k].cpu().numpy(), w, h, 1 if "-inntsc" in flags else 0, k)[1]
                f[:RS.field_of(k)] = 0                                            # the clip form zeroes row 0 of a field == 1 output
                wanted[k] = f
            return wanted[k]

        def verify(what):
            """the output buffer as the timed calls before this point left it; cleared behind the compare, so that a
            later compare cannot pass on these bytes"""
            stream.synchronize()
            v = V.verify_frames(T, want, lambda k: out[k].cpu().numpy(), what)
            with torch.cuda.stream(stream):
                out.zero_()
            stream.synchronize()
            return v

        case = {"flags": flags, "src": [sw, sh], "dst": [w, h], "overall": measure(0, T), "kernels": sc.last_kernels()[:2],
                "effects": {}}
        for e, ename in enumerate(EFFECTS):
            first, last = min(T, 180 * e), min(T, 180 * (e + 1))
            if last > first:
                case["effects"][ename] = measure(first, last)
        if not a.no_verify:
            case.update(verify(name))                                             # every run so far used the window
        if name == CONFIGS[0][0]:
            sc.debug_set_window_rows(0)
            case["all_spill"] = measure(0, T)
            case["all_spill"]["kernels"] = sc.last_kernels()[:2]
            if not a.no_verify:
                case["all_spill"].update(verify(name + ", all-spill form"))
            sc.debug_set_window_rows(-1)
            case["window_over_all_spill"] = case["all_spill"]["ms"] / case["overall"]["ms"]
        result["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        del src, out
        torch.cuda.empty_cache()
    sim.close()
    if a.ref_cpu_fps is not None:
        result["reference_cpu"] = {
            "what": "the reference's own loop (ffmpeg_scanimate.cpp:817-974, -O2), one core, 600x800 -> 720x480",
            "host": a.ref_cpu_host, "fields_per_s": a.ref_cpu_fps,
        }
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
