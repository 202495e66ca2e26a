#!/usr/bin/env python3
"""Speed of the colorkey stage on the GPU, beside its yardstick: a device-to-device hipMemcpyAsync with the same
memory traffic, same process, same run.

Workload: a clip of N output frames (default 600) of two layers resident in HBM, keyed by ntscsim_key_clip_device onto
a ring of `delay` frames.  Cases: 720x486 and 1920x1080, delay 1 and 8, without noise and with -noise 500 on the top
layer.  Layer settings: -color 0x20C040 -threshhold 96 -f 8 on the bottom layer, -xd 3 on the top one.

Per case: the call is timed with device events (median of --reps runs after --warmup runs; the pointer arrays are
built once, so a run is the C call alone: record upload, the launches).  Algorithmic bytes per output frame are
4*W*H*(layers + 1): every present layer read once, the output written once, no destination read after a chain's
first step.  frac_hbm = bytes / time / 8 TB/s.  `copy_half` is a device-to-device copy of half that many bytes -- a
copy of n bytes reads n and writes n, so the half-size copy is the one with the kernel's traffic; `copy_same_bytes`
moves all of them (the yardstick of profiles/blend.json).  `frames_form` is the same clip through
ntscsim_key_frames_device, one frame per call (reads the destination at every frame).  `noise_overhead_share` of a
noisy case is 1 - plain / noisy of the event times: everything noise adds, k_key_draw and the pixel kernel's bit reads.
Before a size's numbers are printed every case of it is verified against the checker (tools/bench_verify.py;
--no-verify skips it).  The ring is zeroed in front of the last timed clip call, outside its two events, and what that
call left is compared: the first 2 * delay + 3 output frames -- the whole clip and the ring where the checker's pace
allows -- and the ring index and rand() position behind it.  `frames_verified` and `verify_s` say what was compared.
`draw_kernel_share` is the share of a noisy run spent in k_key_draw itself, by the kernels' own durations: it comes from
a kernel trace of this tool, taken in a run of its own and folded into the result afterwards:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o ks -- python tools/bench_key.py --reps 5 --warmup 2
    python tools/bench_key.py --fold-trace DIR/.../ks_kernel_trace.csv --out profiles/key.json

    python tools/bench_key.py [--frames 600] [--reps 10] [--warmup 3] [--ref-cpu-fps X --ref-cpu-fps-noise Y] [--out profiles/key.json]

--ref-cpu-fps* record the reference's own loop as measured elsewhere (tests/golden/make_golden_colorkey.py --bench on
the build machine's CPU: one thread, 720x486, 2 layers): a different host, labelled as such."""
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


def fold_trace(csv_path, json_path):
    """draw_kernel_share and the kernels' own durations per noisy case, from a rocprofv3 kernel trace of this tool."""
    import csv
    with open(json_path) as f:
        result = json.load(f)
    rows = [r for r in csv.DictReader(open(csv_path)) if "k_key" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    acc = {}
    pending = 0.0
    for r in rows:
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        name = r["Kernel_Name"]
        if "k_key_draw" in name:
            pending += us
        elif "k_key_clip" in name:
            key = (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), "<true" in name)
            a = acc.setdefault(key, [0.0, 0.0, 0])
            a[0] += pending
            a[1] += us
            a[2] += 1
            pending = 0.0
        else:
            pending = 0.0                                                         # the frames form: not folded
    for name, case in result["cases"].items():
        slices = ((case["width"] + 3) // 4 * case["height"] + 255) // 256
        a = acc.get((slices * 256, min(case["delay"], result["frames"]), bool(case["noisekey"])))
        if not a:
            continue
        case["trace_clip_kernel_us_total"] = a[1]
        case["trace_launches"] = a[2]
        if case["noisekey"]:
            case["trace_draw_kernel_us_total"] = a[0]
            case["draw_kernel_share"] = a[0] / (a[0] + a[1])
    with open(json_path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, case in sorted(result["cases"].items()):
        print(name, case.get("draw_kernel_share"), case.get("trace_clip_kernel_us_total"), case.get("trace_launches"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold-trace", default=None)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="720x486,1920x1080")
    ap.add_argument("--ref-cpu-fps", type=float, default=None)
    ap.add_argument("--ref-cpu-fps-noise", type=float, default=None)
    ap.add_argument("--out", default=None)
    V.add_argument(ap)
    a = ap.parse_args()
    if a.fold_trace:
        if not a.out:
            sys.exit("--fold-trace needs --out, the result file to fold into")
        return fold_trace(a.fold_trace, a.out)

    import torch
    import ntscsim
    if not torch.cuda.is_available():
        sys.exit("bench_key.py needs a GPU")
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3
    stream = torch.cuda.Stream()
    T = a.frames
    result = {"device": torch.cuda.get_device_name(0), "frames": T, "layers": 2, "reps": a.reps, "warmup": a.warmup,
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
        import _key_ref as RK
        RK.RAND = V.block_rand(RK.GlibcRand)                                      # the same stream, cheap at these positions
    sim = ntscsim.FieldSimulator(device=0)
    for size in a.sizes.split(","):
        w, h = (int(x) for x in size.split("x"))
        with torch.cuda.stream(stream):
            src = torch.randint(0, 256, (2, T, h, w, 4), dtype=torch.uint8, device="cuda")
            src[:, :, :, : w // 2, 1] = 0xC0                                      # half of the pixels near the key colour
            out = torch.zeros((T, h, w, 4), dtype=torch.uint8, device="cuda")
        stream.synchronize()
        sh = C.c_void_p(stream.cuda_stream)
        nbytes = 4 * w * h * 3 * T

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

        c0 = timed(copier(nbytes))
        plain_ms = {}
        for delay in (1, 8):
            for noise in (0, 500):
                argv = ["-d", str(delay), "-i", "bottom", "-color", "0x20C040", "-threshhold", "96", "-f", "8",
                        "-i", "top", "-f", "0", "-xd", "3", "-noise", str(noise)]
                ck = ntscsim.ColorKeyer(argv, width=w, height=h, sim=sim)
                with torch.cuda.stream(stream):
                    ring = torch.zeros((delay, h, w, 4), dtype=torch.uint8, device="cuda")
                stream.synchronize()
                rp = (C.c_void_p * delay)(*[ring[i].data_ptr() for i in range(delay)])
                sp = (C.c_void_p * (2 * T))(*[src[l, t].data_ptr() for l in range(2) for t in range(T)])
                ls = (C.c_int32 * 2)(4 * w, 4 * w)
                op = (C.c_void_p * T)(*[out[t].data_ptr() for t in range(T)])
                lib, hctx = ck._lib, ck.sim._h

                behind = {}

                def run_clip():
                    ri, pos = C.c_int32(0), C.c_uint64(0)
                    rc = lib.ntscsim_key_clip_device(hctx, rp, 4 * w, C.byref(ri), sp, ls, op, 4 * w, T, C.byref(pos), sh)
                    if rc != 0:
                        raise RuntimeError("ntscsim_key_clip_device: %d" % rc)
                    behind["ri"], behind["pos"] = ri.value, pos.value

                def zero_ring():
                    with torch.cuda.stream(stream):
                        ring.zero_()

                descs = []
                pos = 0
                for t in range(T):
                    arr, keep = ck._descs([(ring[t % delay], [src[0, t], src[1, t]], pos)], lambda x: x.data_ptr(), lambda x: x.stride(0))
                    descs.append((arr, keep))
                    pos = ck.rand_advance(pos)

                def run_frames():
                    for arr, _ in descs:
                        rc = lib.ntscsim_key_frames_device(hctx, arr, 1, sh)
                        if rc != 0:
                            raise RuntimeError("ntscsim_key_frames_device: %d" % rc)

                name = "%dx%d_d%d_%s" % (w, h, delay, "noise" if noise else "plain")
                k = timed(run_clip, None if a.no_verify else zero_ring)
                kernels = ck.last_kernels()
                verified = {}
                if not a.no_verify:                                               # what the last timed call left, before the frames form writes the ring
                    layers = [RK.layer(color=L.color, threshhold=L.threshhold, fade=L.fade, xdivr=L.xdivr, invert=L.invert,
                                       noisekey=L.noisekey) for L in ck.params.layers[:ck.n_layers]]   # as the switches were parsed
                    if behind["ri"] != T % delay or behind["pos"] != pos:
                        V.mismatch("%s: ring index %d, position %d behind the clip (want %d, %d)"
                                   % (name, behind["ri"], behind["pos"], T % delay, pos))
                    at = [0]

                    def step(dst, t):
                        at[0] = RK.key_frame(dst, [src[0, t].cpu().numpy(), src[1, t].cpu().numpy()], layers, at[0])

                    verified = V.verify_clip(T, delay, (h, w, 4), step, lambda t: out[t].cpu().numpy(),
                                             lambda i: ring[i].cpu().numpy(), name)
                f = timed(run_frames)
                case = {
                    "width": w, "height": h, "delay": delay, "noisekey": noise, "kernels": kernels,
                    "algorithmic_bytes": nbytes,
                    "clip_ms": k[0], "clip_ms_min_max": [k[1], k[2]],
                    "frames_per_s": T / (k[0] * 1e-3),
                    "frac_hbm": nbytes / (k[0] * 1e-3) / HBM_BYTES_PER_S,
                    "frames_form_ms": f[0], "frames_form_over_clip": f[0] / k[0],
                }
                case.update(verified)
                if noise:
                    case["noise_overhead_share"] = 1.0 - plain_ms[delay] / k[0]
                else:
                    plain_ms[delay] = k[0]
                result["cases"][name] = case
                del ring, descs
        c1 = timed(copier(nbytes))
        ch = timed(copier(nbytes // 2))
        copy_ms = 0.5 * (c0[0] + c1[0])
        for name, case in result["cases"].items():
            if name.startswith("%dx%d_" % (w, h)):
                case.update({"copy_same_bytes_ms": copy_ms, "copy_same_bytes_ms_runs": [c0[0], c1[0]],
                             "copy_frac_hbm": nbytes / (copy_ms * 1e-3) / HBM_BYTES_PER_S, "copy_half_ms": ch[0],
                             "copy_over_clip": copy_ms / case["clip_ms"], "copy_half_over_clip": ch[0] / case["clip_ms"]})
                print(name, json.dumps(case), flush=True)
        del src, out
        torch.cuda.empty_cache()
    sim.close()
    if a.ref_cpu_fps is not None:
        result["reference_cpu"] = {
            "what": "the reference's own loop (ffmpeg_colorkey.cpp:832-886 per layer, ring of 1), one thread, 720x486, 2 layers",
            "host": "the build machine's CPU, not the GPU host: a different machine",
            "frames_per_s": a.ref_cpu_fps, "frames_per_s_noise_500": a.ref_cpu_fps_noise,
        }
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
