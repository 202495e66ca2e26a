#!/usr/bin/env python3
"""Speed of the average_delay stage on the GPU, beside its yardstick: a device-to-device hipMemcpyAsync with the same
memory traffic, same process, same run.

Workload: a clip of N output frames (default 600) of one or two layers resident in HBM, averaged by
ntscsim_avg_clip_device onto a ring of `delay` frames.  Cases: 720x486 and 1920x1080, delay 1 and 8, one layer (-n 128)
and two layers (-n 128, -n 64).

Per case: the call is timed with device events (median of --reps runs after --warmup runs; the pointer arrays are
built once, so a run is the C call alone: record upload, the launch).  Algorithmic bytes per output frame are
4*W*H*(layers + 1): every layer read once, the output written once; the ring is read and written once per clip, which
600 frames make negligible.  frac_hbm = bytes / time / 8 TB/s.  `copy_half` is a device-to-device copy of half that
many bytes -- a copy of n bytes reads n and writes n, so the half-size copy is the one with the kernel's traffic;
`copy_same_bytes` moves all of them (the yardstick of profiles/blend.json).  `frames_form` is the same clip through
ntscsim_avg_frames_device, one frame per call (reads the destination at every frame).

Before a size's numbers are printed every case of it is verified against the checker (tools/bench_verify.py;
--no-verify skips it).  The ring is zeroed in front of the last timed clip call, outside its two events, and what that
call left is compared: the first 2 * delay + 3 output frames -- the whole clip and the ring where the checker's pace
allows -- and the ring index and field number behind it.  `frames_verified` and `verify_s` say what was compared.

    python tools/bench_avg.py [--frames 600] [--reps 10] [--warmup 3] [--ref-cpu-fps X --ref-cpu-fps-2 Y] [--out profiles/avg.json]

--ref-cpu-fps* record the reference's own loop as measured elsewhere (tests/golden/make_golden_avgdelay.py --bench on
the build machine's CPU: one thread, 720x486, one / two layers): a different host, labelled as such."""
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
LEVELS = (128, 64)


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="720x486,1920x1080")
    ap.add_argument("--ref-cpu-fps", type=float, default=None)
    ap.add_argument("--ref-cpu-fps-2", type=float, default=None)
    ap.add_argument("--out", default=None)
    V.add_argument(ap)
    a = ap.parse_args()

    import torch
    import ntscsim
    if not torch.cuda.is_available():
        sys.exit("bench_avg.py needs a GPU")
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3
    stream = torch.cuda.Stream()
    T = a.frames
    result = {"device": torch.cuda.get_device_name(0), "frames": T, "reps": a.reps, "warmup": a.warmup,
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "cases": {}}

    def timed(fn, before_last=None):
        """before_last: enqueued in front of the last run, outside its two events"""
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
        return statistics.median(ms), min(ms), max(ms)

    if not a.no_verify:
        import _avg_ref as RA
    sim = ntscsim.FieldSimulator(device=0)
    for size in a.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        with torch.cuda.stream(stream):
            src = torch.randint(0, 256, (2, T, h, w, 4), dtype=torch.uint8, device="cuda")
            out = torch.zeros((T, h, w, 4), dtype=torch.uint8, device="cuda")
        stream.synchronize()
        sh = C.c_void_p(stream.cuda_stream)

        def copier(total):
            flat_src, flat_out = src.view(-1), out.view(-1)
            piece = min(flat_src.numel(), flat_out.numel())

            def run():
                left = total
                while left > 0:
                    n = min(left, piece)
                    if hip.hipMemcpyAsync(C.c_void_p(flat_out.data_ptr()), C.c_void_p(flat_src.data_ptr()), n, D2D, sh) != 0:
                        raise RuntimeError("hipMemcpyAsync failed")
                    left -= n
            return run

        copies = {}
        for nl in (1, 2):
            nbytes = 4 * w * h * (nl + 1) * T
            copies[nl] = [timed(copier(nbytes))]
        for nl in (1, 2):
            nbytes = 4 * w * h * (nl + 1) * T
            for delay in (1, 8):
                argv = ["-d", str(delay)]
                for l in range(nl):
                    argv += ["-i", "layer%d" % l, "-n", str(LEVELS[l])]
                av = ntscsim.FrameAverager(argv, width=w, height=h, sim=sim)
                with torch.cuda.stream(stream):
                    ring = torch.zeros((delay, h, w, 4), dtype=torch.uint8, device="cuda")
                stream.synchronize()
                rp = (C.c_void_p * delay)(*[ring[i].data_ptr() for i in range(delay)])
                sp = (C.c_void_p * (nl * T))(*[src[l, t].data_ptr() for l in range(nl) for t in range(T)])
                ls = (C.c_int32 * nl)(*([4 * w] * nl))
                op = (C.c_void_p * T)(*[out[t].data_ptr() for t in range(T)])
                lib, hctx = av._lib, av.sim._h

                behind = {}

                def run_clip():
                    ri, field = C.c_int32(0), C.c_uint64(0)
                    rc = lib.ntscsim_avg_clip_device(hctx, rp, 4 * w, C.byref(ri), sp, ls, op, 4 * w, T, C.byref(field), sh)
                    if rc != 0:
                        raise RuntimeError("ntscsim_avg_clip_device: %d" % rc)
                    behind["ri"], behind["field"] = ri.value, field.value

                def zero_ring():
                    with torch.cuda.stream(stream):
                        ring.zero_()

                descs = [av._descs([(ring[t % delay], [src[l, t] for l in range(nl)], t)], lambda x: x.data_ptr(), lambda x: x.stride(0))
                         for t in range(T)]

                def run_frames():
                    for arr, _ in descs:
                        rc = lib.ntscsim_avg_frames_device(hctx, arr, 1, sh)
                        if rc != 0:
                            raise RuntimeError("ntscsim_avg_frames_device: %d" % rc)

                name = "%dx%d_d%d_l%d" % (w, h, delay, nl)
                k = timed(run_clip, None if a.no_verify else zero_ring)
                kernels = av.last_kernels()
                verified = {}
                if not a.no_verify:                                               # what the last timed call left, before the frames form writes the ring
                    if behind["ri"] != T % delay or behind["field"] != T:
                        V.mismatch("%s: ring index %d, field %d behind the clip (want %d, %d)"
                                   % (name, behind["ri"], behind["field"], T % delay, T))

                    def step(dst, t, nl=nl, delay=delay):
                        RA.avg_frame(dst, [src[l, t].cpu().numpy() for l in range(nl)], LEVELS[:nl], t, delay)

                    verified = V.verify_clip(T, delay, (h, w, 4), step, lambda t: out[t].cpu().numpy(),
                                             lambda i: ring[i].cpu().numpy(), name)
                f = timed(run_frames)
                result["cases"][name] = {
                    "width": w, "height": h, "delay": delay, "layers": nl, "newlevels": list(LEVELS[:nl]), "kernels": kernels,
                    "algorithmic_bytes": nbytes,
                    "clip_ms": k[0], "clip_ms_min_max": [k[1], k[2]],
                    "frames_per_s": T / (k[0] * 1e-3),
                    "frac_hbm": nbytes / (k[0] * 1e-3) / HBM_BYTES_PER_S,
                    "frames_form_ms": f[0], "frames_form_over_clip": f[0] / k[0],
                }
                result["cases"][name].update(verified)
                del ring, descs
        for nl in (1, 2):
            nbytes = 4 * w * h * (nl + 1) * T
            copies[nl].append(timed(copier(nbytes)))
            ch = timed(copier(nbytes // 2))
            copy_ms = 0.5 * (copies[nl][0][0] + copies[nl][1][0])
            for name, case in result["cases"].items():
                if name.startswith("%dx%d_" % (w, h)) and case["layers"] == nl:
                    case.update({"copy_same_bytes_ms": copy_ms, "copy_same_bytes_ms_runs": [copies[nl][0][0], copies[nl][1][0]],
                                 "copy_frac_hbm": nbytes / (copy_ms * 1e-3) / HBM_BYTES_PER_S, "copy_half_ms": ch[0],
                                 "copy_over_clip": copy_ms / case["clip_ms"], "copy_half_over_clip": ch[0] / case["clip_ms"]})
                    print(name, json.dumps(case), flush=True)
        del src, out
        torch.cuda.empty_cache()
    sim.close()
    if a.ref_cpu_fps is not None:
        result["reference_cpu"] = {
            "what": "the reference's own loop (ffmpeg_average_delay.cpp:800-837 per layer, ring of 1), one thread, 720x486",
            "host": "the build machine's CPU, not the GPU host: a different machine",
            "frames_per_s_1_layer": a.ref_cpu_fps, "frames_per_s_2_layers": a.ref_cpu_fps_2,
        }
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
