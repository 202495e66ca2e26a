#!/usr/bin/env python3
"""Speed of the vhsled stage (ntscsim_led_frames_device) on the GPU, beside its yardstick: a device-to-device
hipMemcpyAsync of the same memory traffic, same process, same buffers, same run.

Workload: N frames (default 600) resident in HBM, every frame a buffer of its own, at 720x486 and at 1920x1080:
  capture   random picture content behind a dark left border whose length jitters per row, 8 .. 40 pixels: every
            row's edge lies inside the scan's first probe
  all_dark  no row has an edge: every scan reads its whole row, the worst case of the scan

Per case the call is timed with device events (median of --reps runs after --warmup runs; the descriptor array is built
once, so a run is the C call alone: record upload + one kernel).  Floor traffic per frame is 8*W*H bytes, one read and
one write; frac_hbm = 8*W*H*N / time / 8 TB/s.  The copy moves 4*W*H*N bytes from the source clip into the output
clip -- a copy of n bytes reads n and writes n, so that is the stage's floor traffic.  The kernel is timed in both
forms of its source loads (16-byte loads from dword-aligned addresses, the default; four dword loads,
NTSCSIM_LED_SRC_DWORDS=1), alternating, between two runs of the copy.

Before a case's numbers are printed, output frames 0, 1, the middle one and the last are compared with the checker
(tools/bench_verify.py; --no-verify skips it) as the first timed runs of each form of the source loads left them; the
output is cleared between the two.  `frames_verified` and `verify_s` of the case are the default form's, those of its
`src_dwords` entry the dword form's.

    python tools/bench_led.py [--frames 600] [--reps 10] [--warmup 3] [--ref-cpu-fps X] [--out profiles/led.json]

--ref-cpu-fps records the reference's own loop (ffmpeg_vhsled.cpp:866-931) as measured elsewhere: one thread, 720x486,
the capture clip, on the build machine's CPU -- a different host, labelled as such."""
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


def make_clip(torch, n, w, h, dark, seed):
    """[n, h, w, 4] uint8 on the GPU.  Every row's first pixel has blue 4; a border pixel stays below 16 in every
    channel (blackish), a picture pixel has green >= 32 (not blackish)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    clip = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
    step = max(1, (256 << 20) // (w * h * 4))
    x = torch.arange(w, device="cuda").view(1, 1, w, 1)
    for i in range(0, n, step):
        m = min(step, n - i)
        pic = torch.randint(0, 256, (m, h, w, 4), dtype=torch.uint8, device="cuda", generator=g)
        if dark:
            pic[..., :3] //= 16
        else:
            pic[..., 1] |= 32
            border = torch.randint(8, 41, (m, h, 1, 1), device="cuda", generator=g)
            low = pic // 16
            low[..., 3] = pic[..., 3]
            pic = torch.where(x < border, low, pic)
        pic[:, :, 0, 0] = 4
        clip[i:i + m] = pic
    return clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-cpu-fps", type=float, default=None)
    ap.add_argument("--out", default=None)
    V.add_argument(ap)
    a = ap.parse_args()

    import torch
    import ntscsim
    if not torch.cuda.is_available():
        sys.exit("bench_led.py needs a GPU")
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

    for w, h in ((720, 486), (1920, 1080)):
        # one context per form of the source loads: the switch is read when a context first binds the stage
        os.environ.pop("NTSCSIM_LED_SRC_DWORDS", None)
        wide = ntscsim.EdgeAligner(width=w, height=h)
        os.environ["NTSCSIM_LED_SRC_DWORDS"] = "1"
        narrow = ntscsim.EdgeAligner(width=w, height=h)
        os.environ.pop("NTSCSIM_LED_SRC_DWORDS", None)
        for kind in ("capture", "all_dark"):
            with torch.cuda.stream(stream):
                src = make_clip(torch, a.frames, w, h, kind == "all_dark", 1000 + w)
                out = torch.zeros((a.frames, h, w, 4), dtype=torch.uint8, device="cuda")
            stream.synchronize()
            jobs = [(out[k], src[k]) for k in range(a.frames)]
            arr = wide._descs(jobs, lambda t: t.data_ptr(), lambda t: t.stride(0))
            nbytes = 8 * w * h * a.frames
            sh = C.c_void_p(stream.cuda_stream)

            def runner(led):
                def run():
                    rc = led._lib.ntscsim_led_frames_device(led.sim._h, arr, len(jobs), sh)
                    if rc != 0:
                        raise RuntimeError("ntscsim_led_frames_device: %d" % rc)
                return run

            def copy():
                if hip.hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), nbytes // 2, D2D, sh) != 0:
                    raise RuntimeError("hipMemcpyAsync failed")

            # the copies first and last, the kernels between them: drift of the clock shows as a difference of the two
            c0 = timed(copy)
            name = "%dx%d_%s" % (w, h, kind)

            def verify(what):
                """the output as the timed runs before this point left it; cleared behind the compare"""
                if a.no_verify:
                    return {}
                import _led_ref as RL
                stream.synchronize()
                v = V.verify_frames(a.frames, lambda k: RL.align_frame(src[k].cpu().numpy())[0], lambda k: out[k].cpu().numpy(), what)
                with torch.cuda.stream(stream):
                    out.zero_()
                stream.synchronize()
                return v

            k0 = timed(runner(wide))
            kernels = wide.last_kernels()
            verified = verify(name + ", 16-byte loads")
            n0 = timed(runner(narrow))
            kernels_narrow = narrow.last_kernels()
            verified_narrow = verify(name + ", dword loads")
            k1 = timed(runner(wide))
            n1 = timed(runner(narrow))
            c1 = timed(copy)
            # what the clip looks like to the stage: the shifts of its first frame
            wide.debug_keep_edges(True)
            wide.align_frames([(out[0], src[0])], stream=stream.cuda_stream)
            e, x = wide.edges(0)
            wide.debug_keep_edges(False)
            led_ms, narrow_ms, copy_ms = 0.5 * (k0[0] + k1[0]), 0.5 * (n0[0] + n1[0]), 0.5 * (c0[0] + c1[0])
            case = {
                "width": w, "height": h, "kind": kind, "kernels": kernels, "floor_bytes": nbytes,
                "edge_min_max_first_frame": [int(e.min()), int(e.max())], "shift_min_max_first_frame": [int(x.min()), int(x.max())],
                "led_ms": led_ms, "led_ms_runs": [k0[0], k1[0]], "led_ms_min_max": [min(k0[1], k1[1]), max(k0[2], k1[2])],
                "frames_per_s": a.frames / (led_ms * 1e-3),
                "frac_hbm": nbytes / (led_ms * 1e-3) / HBM_BYTES_PER_S,
                "copy_same_traffic_ms": copy_ms, "copy_same_traffic_ms_runs": [c0[0], c1[0]],
                "copy_frac_hbm": nbytes / (copy_ms * 1e-3) / HBM_BYTES_PER_S,
                "led_over_copy": led_ms / copy_ms,
                "src_dwords": {"kernels": kernels_narrow, "led_ms": narrow_ms, "led_ms_runs": [n0[0], n1[0]],
                               "frames_per_s": a.frames / (narrow_ms * 1e-3), "over_default": narrow_ms / led_ms},
            }
            case.update(verified)
            case["src_dwords"].update(verified_narrow)
            result["cases"][name] = case
            print(name, json.dumps(case), flush=True)
            del src, out, jobs, arr
            torch.cuda.empty_cache()
        wide.close()
        narrow.close()
    if a.ref_cpu_fps is not None:
        result["reference_cpu"] = {
            "what": "the reference's own loop (ffmpeg_vhsled.cpp:866-931), one thread, 720x486, the capture clip",
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
