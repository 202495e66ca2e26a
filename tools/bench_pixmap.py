#!/usr/bin/env python3
"""Speed of the posterize and colormap stages (ntscsim_post_frames_device, ntscsim_cmap_frames_device) on the GPU, beside
their yardstick: a device-to-device hipMemcpyAsync of the same memory traffic, same process, same buffers, same run.

Workload: N frames (default 600) resident in HBM, every frame a buffer of its own, one call, at 720x486 and 1920x1080:
  sources   gradient      smooth ramps: neighbouring pixels have neighbouring greens, the table reads of a wavefront
                          fall on few entries (what pictures do)
            random_green  every byte uniform noise: the table reads of a 32-lane group spread over all banks
  stages    post          k_post_frames, threshhold 3: a copy with one AND per dword, the floor for the gather
            cmap_map      k_cmap_frames with a map in every descriptor (the table filled from the map's middle row),
                          then k_cmap_take
            cmap_nomap    k_cmap_frames with no map at all (the table filled from the ctx's table)

Per case the call is timed with device events (median of --reps runs after --warmup runs; the descriptor array is built
once, so a run is the C call alone: record upload + the kernels).  Floor traffic per frame is 8*W*H bytes, one read and
one write; frac_hbm = 8*W*H*N / time / 8 TB/s.  The copy moves 4*W*H*N bytes from the source clip into the output clip
-- a copy of n bytes reads n and writes n.  The copies are taken first and last, the stages between them in two rounds,
so drift shows as a difference of the two series; `spread` of a size is the largest relative difference between two
series of one thing in that run, the measure `cmap_over_post` is read against.

Before a case's numbers are printed, output frames 0, 1, the middle one and the last are compared with the checker
(tools/bench_verify.py; --no-verify skips it) as the first timed runs left them.

    python tools/bench_pixmap.py [--frames 600] [--reps 10] [--warmup 3] [--ref-cpu-fps-post X --ref-cpu-fps-cmap Y]
                                 [--out profiles/pixmap.json]

--ref-cpu-fps-* record the reference's own loops (ffmpeg_posterize.cpp:789-813; ffmpeg_colormap.cpp:785-822, take and
apply) as measured elsewhere: one thread, 720x486, on the build machine's CPU -- a different host, labelled as such."""
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
from bench_led import HBM_BYTES_PER_S, hip_runtime  # noqa: E402


def make_clip(torch, n, w, h, kind, seed):
    """[n, h, w, 4] uint8 on the GPU"""
    if kind == "random_green":
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        clip = torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda")
        step = max(1, (256 << 20) // (w * h * 4))
        for i in range(0, n, step):
            m = min(step, n - i)
            clip[i:i + m] = torch.randint(0, 256, (m, h, w, 4), dtype=torch.uint8, device="cuda", generator=g)
        return clip
    x = torch.arange(w, device="cuda").view(1, 1, w)
    y = torch.arange(h, device="cuda").view(1, h, 1)
    k = torch.arange(n, device="cuda").view(n, 1, 1)
    chans = [(x * 255) // max(1, w - 1) + 0 * y + 0 * k, ((x + 2 * y + 3 * k) // 4) % 256, (y * 255) // max(1, h - 1) + 0 * x + 0 * k,
             255 + 0 * (x + y + k)]
    return torch.stack([c.to(torch.uint8) for c in chans], dim=3).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-cpu-fps-post", type=float, default=None)
    ap.add_argument("--ref-cpu-fps-cmap", type=float, default=None)
    ap.add_argument("--out", default=None)
    V.add_argument(ap)
    a = ap.parse_args()

    import torch
    import ntscsim
    if not torch.cuda.is_available():
        sys.exit("bench_pixmap.py needs a GPU")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _pixmap_ref as R
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    D2D = 3
    stream = torch.cuda.Stream()
    sh = C.c_void_p(stream.cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "reps": a.reps, "warmup": a.warmup,
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "cases": {}, "spread": {}}

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
        post = ntscsim.Posterizer(["-i", "in"], width=w, height=h)                 # threshhold 3, the tool's default
        cm = ntscsim.ColorMapper(width=w, height=h)
        nbytes = 8 * w * h * a.frames
        spread = 0.0
        for kind in ("gradient", "random_green"):
            with torch.cuda.stream(stream):
                src = make_clip(torch, a.frames, w, h, kind, 2000 + w)
                maps = make_clip(torch, a.frames, w, h, "random_green", 3000 + w)
                out = torch.zeros((a.frames, h, w, 4), dtype=torch.uint8, device="cuda")
            stream.synchronize()
            entry = (R.identity_table() ^ 0x00FF00FF).astype("uint32")
            stages = {
                "post": (post, post._descs([(out[k], src[k]) for k in range(a.frames)], lambda t: t.data_ptr(), lambda t: t.stride(0)),
                         lambda k, s: R.posterize(s, 3)),
                "cmap_map": (cm, cm._descs([(out[k], src[k], maps[k]) for k in range(a.frames)], lambda t: t.data_ptr(), lambda t: t.stride(0)),
                             lambda k, s: R.apply(s, R.take(maps[k].cpu().numpy()))),
                "cmap_nomap": (cm, cm._descs([(out[k], src[k], None) for k in range(a.frames)], lambda t: t.data_ptr(), lambda t: t.stride(0)),
                               lambda k, s: R.apply(s, entry)),
            }

            def runner(name):
                stage, arr, _ = stages[name]
                call = getattr(stage._lib, "ntscsim_%s_frames_device" % stage._STAGE)

                def run():
                    rc = call(stage.sim._h, arr, a.frames, sh)
                    if rc != 0:
                        raise RuntimeError("ntscsim_%s_frames_device: %d" % (stage._STAGE, rc))
                return run

            def copy():
                if hip.hipMemcpyAsync(C.c_void_p(out.data_ptr()), C.c_void_p(src.data_ptr()), nbytes // 2, D2D, sh) != 0:
                    raise RuntimeError("hipMemcpyAsync failed")

            def verify(name):
                """the output as the timed runs before this point left it; cleared behind the compare"""
                if a.no_verify:
                    return {}
                stream.synchronize()
                want = stages[name][2]
                v = V.verify_frames(a.frames, lambda k: want(k, src[k].cpu().numpy()), lambda k: out[k].cpu().numpy(),
                                    "%dx%d %s %s" % (w, h, kind, name))
                with torch.cuda.stream(stream):
                    out.zero_()
                stream.synchronize()
                return v

            series = {"copy": [timed(copy)]}
            kernels, verified = {}, {}
            for rnd in range(2):
                for name in stages:
                    if name == "cmap_nomap":
                        stream.synchronize()
                        cm.table = entry                                           # the maps of cmap_map left theirs
                    series.setdefault(name, []).append(timed(runner(name)))
                    if rnd == 0:
                        kernels[name] = stages[name][0].last_kernels()
                        verified[name] = verify(name)
            series["copy"].append(timed(copy))
            med = {name: 0.5 * (s[0][0] + s[1][0]) for name, s in series.items()}
            for s in series.values():
                spread = max(spread, abs(s[0][0] - s[1][0]) / min(s[0][0], s[1][0]))
            for name in stages:
                case = {
                    "width": w, "height": h, "source": kind, "stage": name, "kernels": kernels[name], "floor_bytes": nbytes,
                    "ms": med[name], "ms_runs": [s[0] for s in series[name]],
                    "ms_min_max": [min(s[1] for s in series[name]), max(s[2] for s in series[name])],
                    "frames_per_s": a.frames / (med[name] * 1e-3),
                    "frac_hbm": nbytes / (med[name] * 1e-3) / HBM_BYTES_PER_S,
                    "copy_same_traffic_ms": med["copy"], "copy_same_traffic_ms_runs": [s[0] for s in series["copy"]],
                    "over_copy": med[name] / med["copy"], "over_post": med[name] / med["post"],
                }
                case.update(verified[name])
                key = "%dx%d_%s_%s" % (w, h, kind, name)
                result["cases"][key] = case
                print(key, json.dumps(case), flush=True)
            del src, maps, out, stages
            torch.cuda.empty_cache()
        result["spread"]["%dx%d" % (w, h)] = spread
        post.close()
        cm.close()
    if a.ref_cpu_fps_post is not None and a.ref_cpu_fps_cmap is not None:
        result["reference_cpu"] = {
            "what": "the reference's own loops (ffmpeg_posterize.cpp:789-813; ffmpeg_colormap.cpp:785-822, take and apply), one thread, 720x486",
            "host": "the build machine's CPU, not the GPU host: a different machine",
            "frames_per_s_post": a.ref_cpu_fps_post, "frames_per_s_cmap": a.ref_cpu_fps_cmap,
        }
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
