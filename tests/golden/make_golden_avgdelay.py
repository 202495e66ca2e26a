"""Generates tests/golden/avgdelay_golden.npz from the reference's own ffmpeg_average_delay.cpp (run once, where the
reference tree exists: NTSC_REFERENCE_DIR, default /root/reference).  Only DATA is written into this repository.

Line range :800-837 of ffmpeg_average_delay.cpp -- composite_layer() whole -- is streamed into g++'s stdin together
with a driver of ours (the pattern of make_golden_colorkey.py) and built in a temporary directory.  The function
dereferences two AVFrames (data[0], linesize[0], width, height), an InputFile (newlevel) and the global
output_avstream_video_frame_delay: structs and a variable of ours with those names stand in for libavutil's and the
tool's, so by this project's rule every fixture here is reported UNPINNED.

The driver is ours: it is the tool's frame loop (:948-970 the ring zeroed once, :1069-1122 every layer of frame
`current` onto ring slot index with field = current, index wraps at delay) with the frames read from a file instead
of decoded, and a first frame number other than 0 where a case asks for it.

parse_argv() :623-708 does not extract without libav; tests/test_avg_params.py derives its expected values by hand
from the cited lines.

--bench times the reference's loop (one thread, 720x486, one and two layers, delay 1) on this machine's CPU and
prints frames per second: the CPU figure quoted beside the GPU figures (profiles/avg.json).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _avg_ref as R  # noqa: E402

REF = os.path.join(os.environ.get("NTSC_REFERENCE_DIR", "/root/reference"), "ffmpeg_average_delay.cpp")

PRE = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <vector>
using namespace std;

/* stand-ins (ours) for what composite_layer() dereferences */
struct AVFrame { uint8_t *data[1]; int linesize[1]; int width, height; };
struct InputFile { int newlevel; };
size_t output_avstream_video_frame_delay = 1;
"""

DRIVER = r"""
/* driver (ours): run|bench <W> <H> <delay> <T> <nl> <first field> <src file> <out file> <present: T*nl chars 0/1>
 * then newlevel per layer */
int main(int argc, char **argv) {
    if (argc < 11) return 2;
    const bool bench = !strcmp(argv[1], "bench");
    const int W = atoi(argv[2]), H = atoi(argv[3]), delay = atoi(argv[4]), T = atoi(argv[5]), nl = atoi(argv[6]);
    unsigned long long current = strtoull(argv[7], NULL, 0);
    const char *present = argv[10];
    if (argc != 11 + nl || (int)strlen(present) != T * nl) return 2;
    output_avstream_video_frame_delay = (size_t)delay;
    std::vector<InputFile> in(nl);
    for (int l = 0; l < nl; l++) in[l].newlevel = (int)strtoul(argv[11 + l], NULL, 0);
    const size_t fb = (size_t)W * H * 4;
    std::vector<uint8_t> src((size_t)T * nl * fb);
    FILE *f = fopen(argv[8], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size()) return 3;
    fclose(f);
    std::vector<AVFrame> ring(delay);
    for (int i = 0; i < delay; i++) {
        ring[i].data[0] = (uint8_t*)malloc(fb); ring[i].linesize[0] = W * 4; ring[i].width = W; ring[i].height = H;
        memset(ring[i].data[0], 0, fb);
    }
    f = bench ? NULL : fopen(argv[9], "wb");
    size_t index = 0;
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int t = 0; t < T; t++) {
        for (int l = 0; l < nl; l++) {
            AVFrame s;
            s.data[0] = src.data() + ((size_t)t * nl + l) * fb; s.linesize[0] = W * 4; s.width = W; s.height = H;
            composite_layer(&ring[index], present[t * nl + l] == '1' ? &s : NULL, in[l], current);
        }
        if (f) fwrite(ring[index].data[0], 1, fb, f);
        if ((++index) >= (size_t)delay) index = 0;
        current++;
    }
    clock_gettime(CLOCK_MONOTONIC, &b);
    if (bench) printf("%.3f\n", T / ((b.tv_sec - a.tv_sec) + 1e-9 * (b.tv_nsec - a.tv_nsec)));
    if (f) fclose(f);
    return 0;
}
"""


def ref_lines(a, b):
    with open(REF) as f:
        lines = f.readlines()
    return "".join(lines[a - 1:b])


def build(tmp):
    exe = os.path.join(tmp, "avg_ref")
    text = PRE + ref_lines(800, 837) + DRIVER
    subprocess.run(["g++", "-x", "c++", "-O2", "-w", "-", "-o", exe], input=text.encode(), check=True)
    return exe


def run(exe, tmp, mode, w, h, delay, levels, src, present, field0=0):
    """src uint8 [T, nl, H, W, 4], present [T][nl] of 0/1 -> outputs [T, H, W, 4] (or the --bench figure)"""
    T, nl = src.shape[0], src.shape[1]
    sf, of = os.path.join(tmp, "avg.src"), os.path.join(tmp, "avg.out")
    src.tofile(sf)
    args = [exe, mode, str(w), str(h), str(delay), str(T), str(nl), str(field0), sf, of,
            "".join(str(int(x)) for row in present for x in row)] + [str(n) for n in levels]
    r = subprocess.run(args, stdout=subprocess.PIPE, check=True, text=True)
    if mode == "bench":
        return r.stdout.strip()
    return np.fromfile(of, dtype=np.uint8).reshape(T, h, w, 4)


# name: (W, H, delay, T, newlevels, first field, present rows or None)
CASES = {
    "levels": (40, 9, 1, 2, [0, 1, 128, 255, 256], 0, None),
    "levels_wrap": (37, 7, 1, 3, [257, 1000, -1, 65536], 0, None),
    "ring_d1": (40, 6, 1, 7, [128, 64], 0, None),
    "ring_d2": (40, 6, 2, 7, [128, 64], 0, None),
    "ring_d3_absent": (38, 6, 3, 12, [200, 300], 0,
                       [[1, 1], [1, 1], [1, 1], [0, 1], [1, 1], [0, 0], [1, 0], [0, 0], [1, 1], [1, 1], [0, 1], [1, 1]]),
    "field_big": (33, 5, 3, 4, [100], (1 << 32) + 5, None),
}


def case_source(name, w, h, T, nl):
    seed = sum(ord(c) for c in name)
    return np.stack([np.stack([R.make_frame(w, h, seed * 100 + t * 10 + l) for l in range(nl)]) for t in range(T)])


def main():
    if not os.path.exists(REF):
        sys.exit("reference not present: " + REF)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        if "--bench" in sys.argv:
            w, h, T = 720, 486, 60
            for levels in ([128], [128, 64]):
                src = case_source("bench", w, h, T, len(levels))
                fps = run(exe, tmp, "bench", w, h, 1, levels, src, [[1] * len(levels)] * T)
                print("reference loop, one CPU thread, 720x486, %d layer(s), delay 1: %s frames/s" % (len(levels), fps))
            return
        for name, (w, h, delay, T, levels, field0, present) in CASES.items():
            nl = len(levels)
            src = case_source(name, w, h, T, nl)
            pres = present if present is not None else [[1] * nl] * T
            got = run(exe, tmp, "run", w, h, delay, levels, src, pres, field0)
            out["avg_%s_geom" % name] = np.array([w, h, delay, T, nl, field0], dtype=np.int64)
            out["avg_%s_levels" % name] = np.array(levels, dtype=np.int64)
            out["avg_%s_present" % name] = np.array(pres, dtype=np.uint8)
            out["avg_%s_src" % name] = src
            out["avg_%s_out" % name] = got
    path = os.path.join(HERE, "avgdelay_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
