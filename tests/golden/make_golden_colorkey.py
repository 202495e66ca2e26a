"""Generates tests/golden/colorkey_golden.npz from the reference's own ffmpeg_colorkey.cpp (run once, where the
reference tree exists: NTSC_REFERENCE_DIR, default /root/reference).  Only DATA is written into this repository.

Line range :832-886 of ffmpeg_colorkey.cpp -- composite_layer() whole -- is streamed into g++'s stdin together with a
driver of ours (the pattern of make_golden_frameblend.py) and built in a temporary directory.  The function
dereferences two AVFrames (data[0], linesize[0], width, height) and an InputFile (color, threshhold, fade, xdivr,
invert, noisekey): structs of ours with those members stand in for libavutil's and the tool's, so by this project's
rule every fixture here is reported UNPINNED.  rand() is this machine's glibc, never seeded; every case runs in a
fresh process, so its stream starts at position 0, and the multi-frame cases walk it to non-zero positions.

The driver is ours: it is the tool's frame loop (:1013-1016 the ring zeroed once, :1118-1171 every layer of a frame
onto ring slot index, index = (index + 1) % delay) with the frames read from a file instead of decoded.

parse_argv() :629-739 does not extract without libav; tests/test_key_params.py derives its expected values by hand
from the cited lines.

--bench times the reference's loop (one thread, 720x486, two layers, delay 1, with and without -noise) on this
machine's CPU and prints frames per second: the CPU figure quoted beside the GPU figures (profiles/key.json).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _key_ref as R  # noqa: E402

REF = os.path.join(os.environ.get("NTSC_REFERENCE_DIR", "/root/reference"), "ffmpeg_colorkey.cpp")

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
struct InputFile { uint32_t color; int threshhold; unsigned int fade; unsigned int xdivr; bool invert; unsigned int noisekey; };
"""

DRIVER = r"""
/* driver (ours): run|bench <W> <H> <delay> <T> <nl> <src file> <out file> <present: T*nl chars 0/1> then per layer
 * color threshhold fade xdivr invert noisekey */
int main(int argc, char **argv) {
    if (argc < 10) return 2;
    const bool bench = !strcmp(argv[1], "bench");
    const int W = atoi(argv[2]), H = atoi(argv[3]), delay = atoi(argv[4]), T = atoi(argv[5]), nl = atoi(argv[6]);
    const char *present = argv[9];
    if (argc != 10 + 6 * nl || (int)strlen(present) != T * nl) return 2;
    std::vector<InputFile> in(nl);
    for (int l = 0; l < nl; l++) {
        char **a = argv + 10 + 6 * l;
        in[l].color = (uint32_t)strtoul(a[0], NULL, 0); in[l].threshhold = atoi(a[1]);
        in[l].fade = (unsigned int)strtoul(a[2], NULL, 0); in[l].xdivr = (unsigned int)strtoul(a[3], NULL, 0);
        in[l].invert = atoi(a[4]) != 0; in[l].noisekey = (unsigned int)strtoul(a[5], NULL, 0);
    }
    const size_t fb = (size_t)W * H * 4;
    std::vector<uint8_t> src((size_t)T * nl * fb);
    FILE *f = fopen(argv[7], "rb");
    if (!f || fread(src.data(), 1, src.size(), f) != src.size()) return 3;
    fclose(f);
    std::vector<AVFrame> ring(delay);
    for (int i = 0; i < delay; i++) {
        ring[i].data[0] = (uint8_t*)malloc(fb); ring[i].linesize[0] = W * 4; ring[i].width = W; ring[i].height = H;
        memset(ring[i].data[0], 0, fb);
    }
    f = bench ? NULL : fopen(argv[8], "wb");
    size_t index = 0;
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int t = 0; t < T; t++) {
        for (int l = 0; l < nl; l++) {
            AVFrame s;
            s.data[0] = src.data() + ((size_t)t * nl + l) * fb; s.linesize[0] = W * 4; s.width = W; s.height = H;
            composite_layer(&ring[index], present[t * nl + l] == '1' ? &s : NULL, in[l]);
        }
        if (f) fwrite(ring[index].data[0], 1, fb, f);
        if ((++index) >= (size_t)delay) index = 0;
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
    exe = os.path.join(tmp, "ck_ref")
    text = PRE + ref_lines(832, 886) + DRIVER
    subprocess.run(["g++", "-x", "c++", "-O2", "-w", "-", "-o", exe], input=text.encode(), check=True)
    return exe


def run(exe, tmp, mode, w, h, delay, layers, src, present):
    """src uint8 [T, nl, H, W, 4], present [T][nl] of 0/1 -> outputs [T, H, W, 4] (or the --bench figure)"""
    T, nl = src.shape[0], src.shape[1]
    sf, of = os.path.join(tmp, "ck.src"), os.path.join(tmp, "ck.out")
    src.tofile(sf)
    args = [exe, mode, str(w), str(h), str(delay), str(T), str(nl), sf, of, "".join(str(int(x)) for row in present for x in row)]
    for lay in layers:
        args += [str(lay[k]) for k in ("color", "threshhold", "fade", "xdivr", "invert", "noisekey")]
    r = subprocess.run(args, stdout=subprocess.PIPE, check=True, text=True)      # a fresh process: rand() at position 0
    if mode == "bench":
        return r.stdout.strip()
    return np.fromfile(of, dtype=np.uint8).reshape(T, h, w, 4)


KEY = 0x8020C040            # non-black, high byte set (:854-856 ignore it)
L = R.layer
# name: (W, H, delay, T, layers, present rows or None)
CASES = {
    "single_plain": (40, 9, 1, 1, [L(color=KEY, threshhold=96)], None),
    "single_inv_fade": (37, 7, 1, 1, [L(color=KEY, threshhold=96, invert=1, fade=128)], None),
    "single_fade_wrap": (37, 7, 1, 2, [L(color=KEY, threshhold=300, fade=300)], None),
    "single_xd3": (41, 6, 1, 1, [L(color=KEY, threshhold=96, xdivr=3)], None),
    "single_xd0_thr_neg": (36, 5, 1, 1, [L(color=KEY, threshhold=-1, xdivr=0), L(color=KEY, threshhold=766, invert=1)], None),
    "single_noise": (40, 9, 1, 1, [L(color=KEY, threshhold=96, noisekey=2000)], None),
    "single_noise_xd7": (43, 8, 1, 1, [L(color=KEY, threshhold=96, noisekey=2000, xdivr=7)], None),
    "single_noise_always": (36, 5, 1, 1, [L(color=KEY, threshhold=96, noisekey=20001, xdivr=64)], None),
    "ring_d1": (40, 6, 1, 7, [L(color=KEY, threshhold=96, fade=8), L(color=0x102030, threshhold=200, invert=1)], None),
    "ring_d2": (40, 6, 2, 7, [L(color=KEY, threshhold=96, fade=8), L(color=0x102030, threshhold=200, invert=1)], None),
    "ring_d3": (40, 6, 3, 7, [L(color=KEY, threshhold=96, fade=8), L(color=0x102030, threshhold=200, invert=1)], None),
    "ring_d1_noise": (38, 6, 1, 7, [L(color=KEY, threshhold=96), L(color=KEY, threshhold=96, noisekey=500, xdivr=3, fade=8)], None),
    "ring_d2_noise": (38, 6, 2, 7, [L(color=KEY, threshhold=96, noisekey=3000), L(color=KEY, threshhold=96, noisekey=500, xdivr=3, fade=8)], None),
    "ring_d3_noise_absent": (38, 6, 3, 7, [L(color=KEY, threshhold=96, noisekey=3000), L(color=0x102030, threshhold=150),
                                           L(color=KEY, threshhold=96, noisekey=500, xdivr=5)],
                             [[1, 1, 1], [0, 1, 1], [1, 0, 1], [1, 1, 0], [0, 0, 1], [1, 1, 1], [0, 1, 0]]),
}


def case_source(name, w, h, T, nl):
    seed = sum(ord(c) for c in name)
    return np.stack([np.stack([R.make_frame(w, h, seed * 100 + t * 10 + l, key=KEY) for l in range(nl)]) for t in range(T)])


def main():
    if not os.path.exists(REF):
        sys.exit("reference not present: " + REF)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        if "--bench" in sys.argv:
            w, h, T = 720, 486, 60
            src = case_source("bench", w, h, T, 2)
            for nk in (0, 500):
                layers = [L(color=KEY, threshhold=96, fade=8), L(color=KEY, threshhold=96, noisekey=nk)]
                fps = run(exe, tmp, "bench", w, h, 1, layers, src, [[1, 1]] * T)
                print("reference loop, one CPU thread, 720x486, 2 layers, delay 1, -noise %d: %s frames/s" % (nk, fps))
            return
        for name, (w, h, delay, T, layers, present) in CASES.items():
            nl = len(layers)
            src = case_source(name, w, h, T, nl)
            pres = present if present is not None else [[1] * nl] * T
            got = run(exe, tmp, "run", w, h, delay, layers, src, pres)
            out["ck_%s_geom" % name] = np.array([w, h, delay, T, nl], dtype=np.int64)
            out["ck_%s_layers" % name] = np.array([[lay[k] for k in ("color", "threshhold", "fade", "xdivr", "invert", "noisekey")]
                                                   for lay in layers], dtype=np.int64)
            out["ck_%s_present" % name] = np.array(pres, dtype=np.uint8)
            out["ck_%s_src" % name] = src
            out["ck_%s_out" % name] = got
    path = os.path.join(HERE, "colorkey_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
