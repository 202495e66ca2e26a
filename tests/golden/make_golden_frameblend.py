"""Generates tests/golden/frameblend_golden.npz from the reference's own frameblend.cpp (run once, where the
reference tree exists: NTSC_REFERENCE_DIR, default /root/reference).  Only DATA is written into this repository.

Line ranges of frameblend.cpp are streamed into g++'s stdin together with a driver of ours (the pattern of
oracle/build_ref_pure.sh) and built in a temporary directory:

  stand-in-free (libc / STL headers only) -- these fixtures PIN tests/_blend_ref.py:
    :44-51      the globals of the blend (squelch, fullframealt, framealt, gamma_correction, underscan)
    :685-732    clamp255, gamma_dec / gamma_enc, the two tables and gamma16_do_init
    :929-1030   the weight scan, squelch and weight16 of one output period, wrapped as the body of a function over
                `frames` / `frame_t` / `current` (the pointer vector is used for its size only)
  with a stand-in -- fixtures reported UNPINNED:
    :1032-1081  the two pixel loops.  They dereference two AVFrames (data[0], linesize[0]): a two-member struct of
                ours stands in for libavutil's, so by this project's rule these frames do not pin anything.

The driver around :929-1030 is ours: it appends frames with the tool's read-ahead (:910), calls the extracted body
once per period and erases the first `cutoff` frames when cutoff >= 32 (:1107-1120), reporting stable frame ids.
The frame times come from tests/_blend_ref.frame_time (:100-110 is an InputFile method and does not extract).

--bench additionally times the reference's gamma pixel loop (one thread, 720x486, 2 taps) on this machine's CPU and
prints frames per second: the honest CPU figure quoted in profiles/blend.json.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _blend_ref as R  # noqa: E402

REF = os.path.join(os.environ.get("NTSC_REFERENCE_DIR", "/root/reference"), "frameblend.cpp")

PRE = r"""
#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <map>
#include <string>
#include <vector>
using namespace std;
"""

STANDIN = r"""
/* stand-in (ours) for the two AVFrames the pixel loops dereference */
struct AVFrame { uint8_t *data[1]; int linesize[1]; };
static AVFrame *output_avstream_video_frame;
static struct { AVFrame *input_avstream_video_frame_rgb; } input_file;
static int output_width, output_height;
"""

PLAN_HEAD = r"""
static void ref_period(std::vector<uint32_t*> &frames, std::vector<double> &frame_t, signed long long current,
                       std::vector< pair<size_t,double> > &weights_out, std::vector<unsigned int> &weight16_out,
                       size_t &cutoff_out) {
"""
PLAN_TAIL = r"""
    weights_out = weights; weight16_out = weight16; cutoff_out = cutoff;
}
"""
PIX_HEAD = r"""
static void ref_pixels(std::vector<uint32_t*> &frames, std::vector< pair<size_t,double> > &weights,
                       std::vector<unsigned int> &weight16) {
"""
PIX_TAIL = "}\n"

DRIVER = r"""
/* driver (ours) */
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "tables")) {                   /* tables <gamma> */
        gamma_correction = atof(argv[2]);
        gamma16_init = false;
        gamma16_do_init();
        for (int i = 0; i < 256; i++) printf("%lu\n", gamma_dec16_table[i]);
        for (int i = 0; i <= 8192; i++) printf("%lu\n", gamma_enc16_table[i]);
        return 0;
    }
    if (!strcmp(argv[1], "plan")) {                     /* plan <sqnr> <ffa> <fa> <periods> <times file> */
        squelch_frameblend_near_match = atoi(argv[2]) != 0;
        fullframealt = atoi(argv[3]) != 0;
        framealt = atoi(argv[4]);
        long long periods = atoll(argv[5]);
        std::vector<double> all;
        FILE *f = fopen(argv[6], "rb");
        double t;
        while (fread(&t, sizeof(t), 1, f) == 1) all.push_back(t);
        fclose(f);
        std::vector<uint32_t*> frames;
        std::vector<double> frame_t;
        size_t pushed = 0, base = 0;
        frame_t.push_back(all[pushed++]); frames.push_back(NULL);
        for (signed long long current = 0; current < periods; current++) {
            while (pushed < all.size() && all[pushed - 1] < (current + 30LL)) {
                frame_t.push_back(all[pushed++]); frames.push_back(NULL);
            }
            std::vector< pair<size_t,double> > weights;
            std::vector<unsigned int> weight16;
            size_t cutoff = 0;
            ref_period(frames, frame_t, current, weights, weight16, cutoff);
            printf("%zu", weights.size());
            for (size_t i = 0; i < weights.size(); i++) printf(" %zu %u %.17g", base + weights[i].first, weight16[i], weights[i].second);
            printf(" # %zu\n", cutoff);
            if (cutoff >= 32) {
                frame_t.erase(frame_t.begin(), frame_t.begin() + cutoff);
                frames.erase(frames.begin(), frames.begin() + cutoff);
                base += cutoff;
            }
        }
        return 0;
    }
    if (!strcmp(argv[1], "pixels") || !strcmp(argv[1], "bench")) {   /* pixels <gamma> <W> <H> <ntaps> <src file> <out file> w16... */
        gamma_correction = atof(argv[2]);
        gamma16_init = false;
        output_width = atoi(argv[3]); output_height = atoi(argv[4]);
        int ntaps = atoi(argv[5]);
        size_t fb = (size_t)output_width * output_height * 4;
        std::vector<uint32_t*> frames;
        std::vector< pair<size_t,double> > weights;
        std::vector<unsigned int> weight16;
        FILE *f = fopen(argv[6], "rb");
        for (int k = 0; k < ntaps; k++) {
            uint32_t *p = (uint32_t*)malloc(fb);
            if (fread(p, 1, fb, f) != fb) return 3;
            frames.push_back(p);
            weights.push_back(pair<size_t,double>((size_t)k, 0.0));
            weight16.push_back((unsigned int)strtoul(argv[8 + k], NULL, 10));
        }
        fclose(f);
        AVFrame in, out;
        in.data[0] = NULL; in.linesize[0] = output_width * 4;
        out.data[0] = (uint8_t*)calloc(1, fb); out.linesize[0] = output_width * 4;
        input_file.input_avstream_video_frame_rgb = &in;
        output_avstream_video_frame = &out;
        if (!strcmp(argv[1], "bench")) {
            ref_pixels(frames, weights, weight16);
            struct timespec a, b;
            int reps = 40;
            clock_gettime(CLOCK_MONOTONIC, &a);
            for (int i = 0; i < reps; i++) ref_pixels(frames, weights, weight16);
            clock_gettime(CLOCK_MONOTONIC, &b);
            printf("%.3f\n", reps / ((b.tv_sec - a.tv_sec) + 1e-9 * (b.tv_nsec - a.tv_nsec)));
            return 0;
        }
        ref_pixels(frames, weights, weight16);
        f = fopen(argv[7], "wb");
        fwrite(out.data[0], 1, fb, f);
        fclose(f);
        return 0;
    }
    return 2;
}
"""


def ref_lines(a, b):
    with open(REF) as f:
        lines = f.readlines()
    return "".join(lines[a - 1:b])


def build(tmp):
    exe = os.path.join(tmp, "fb_ref")
    text = (PRE + ref_lines(44, 51) + ref_lines(685, 732) + STANDIN + PLAN_HEAD + ref_lines(929, 1030) + PLAN_TAIL +
            PIX_HEAD + ref_lines(1032, 1081) + PIX_TAIL + DRIVER)
    subprocess.run(["g++", "-x", "c++", "-O2", "-w", "-ffp-contract=off", "-", "-o", exe], input=text.encode(), check=True)
    return exe


def times(n, in_num, in_den, rate_num, rate_den, jitter=None):
    t = [R.frame_time(k, in_den, in_num, rate_num, rate_den) for k in range(n)]
    if jitter is not None:
        rs = np.random.RandomState(jitter)
        step = t[1] - t[0]
        t = [x + (rs.uniform(-0.35, 0.35) * step if i else 0.0) for i, x in enumerate(t)]
    return t


# name: (frames, input rate, output rate as -or stores it, sqnr, ffa, fa, jitter seed)
PLAN_CASES = {
    "film_to_ntsc": (48, (24000, 1001), (60000, 1001), 0, 0, 1, None),
    "pal_to_ntsc": (50, (25, 1), (599400, 10000), 0, 0, 1, None),
    "r30_to_ntsc": (60, (30, 1), (599400, 10000), 0, 0, 1, None),
    "r30_to_ntsc_sqnr": (60, (30, 1), (599400, 10000), 1, 0, 1, None),
    "near_match": (90, (298, 10), (299700, 10000), 0, 0, 1, None),
    "near_match_sqnr": (90, (298, 10), (299700, 10000), 1, 0, 1, None),
    "nearer_match_sqnr": (90, (2998, 100), (299700, 10000), 1, 0, 1, None),
    "r60_to_24": (120, (60, 1), (240000, 10000), 0, 0, 1, None),
    "r60_to_24_sqnr": (120, (60, 1), (240000, 10000), 1, 0, 1, None),
    "r120_to_5": (240, (120, 1), (50000, 10000), 0, 0, 1, None),
    "fa2": (48, (24000, 1001), (60000, 1001), 0, 0, 2, None),
    "fa3_ffa": (60, (24000, 1001), (60000, 1001), 0, 1, 3, None),
    "jitter": (64, (24000, 1001), (60000, 1001), 0, 0, 1, 7),
    "jitter_sqnr_fa2": (64, (30000, 1001), (60000, 1001), 1, 0, 2, 11),
    "single": (1, (24000, 1001), (60000, 1001), 0, 0, 1, None),
    "long_fa2": (240, (24000, 1001), (60000, 1001), 0, 0, 2, None),
    "long_plain": (240, (60, 1), (599400, 10000), 0, 0, 1, None),
}

# name: (W, H, gamma or -1, weights)
PIX_CASES = {
    "g22_96x32_65536": (96, 32, 2.2, (26214, 39322)),
    "g22_100x35_65535": (100, 35, 2.2, (16384, 49151)),
    "g22_98x33_65537": (98, 33, 2.2, (32769, 32768)),
    "g18_98x33_3taps": (98, 33, 1.8, (10000, 45536, 10000)),
    "plain_96x32_65536": (96, 32, -1, (26214, 39322)),
    "plain_100x35_65535": (100, 35, -1, (16384, 49151)),
    "plain_98x33_65537": (98, 33, -1, (65537, 0)),
    "plain_98x33_over": (98, 33, -1, (65536, 40000)),
    "g22_96x32_over": (96, 32, 2.2, (65536, 40000)),
}


def main():
    if not os.path.exists(REF):
        sys.exit("reference not present: " + REF)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp)
        if "--bench" in sys.argv:
            w, h = 720, 486
            src = os.path.join(tmp, "bench.src")
            np.concatenate([R.noise_frame(w, h, 1), R.noise_frame(w, h, 2)]).tofile(src)
            r = subprocess.run([exe, "bench", "2.2", str(w), str(h), "2", src, "-", "26214", "39322"],
                               stdout=subprocess.PIPE, check=True, text=True)
            print("reference pixel loop, one CPU thread, 720x486, 2 taps, gamma 2.2: %s frames/s" % r.stdout.strip())
            return
        gammas = [2.2, 1.8, 2.4, 1.0001]
        out["tab_gamma"] = np.array(gammas)
        dec, enc = [], []
        for g in gammas:
            r = subprocess.run([exe, "tables", repr(g)], stdout=subprocess.PIPE, check=True, text=True)
            v = [int(x) for x in r.stdout.split()]
            assert len(v) == 256 + 8193 and max(v[:256]) <= 8192 and max(v[256:]) <= 255
            dec.append(v[:256])
            enc.append(v[256:])
        out["tab_dec"] = np.array(dec, dtype=np.uint16)
        out["tab_enc"] = np.array(enc, dtype=np.uint8)

        plans = {}
        for name, (n, irate, orate, sqnr, ffa, fa, jit) in PLAN_CASES.items():
            t = times(n, irate[0], irate[1], orate[0], orate[1], jit)
            periods = R.clip_periods(t[-1])
            tf = os.path.join(tmp, "times.bin")
            np.array(t, dtype=np.float64).tofile(tf)
            r = subprocess.run([exe, "plan", str(sqnr), str(ffa), str(fa), str(periods), tf],
                               stdout=subprocess.PIPE, check=True, text=True)
            counts, ids, w16, wd, cut = [], [], [], [], []
            for line in r.stdout.splitlines():
                body, c = line.split("#")
                f = body.split()
                k = int(f[0])
                counts.append(k)
                for j in range(k):
                    ids.append(int(f[1 + 3 * j]))
                    w16.append(int(f[2 + 3 * j]))
                    wd.append(float(f[3 + 3 * j]))
                cut.append(int(c))
            assert len(counts) == periods
            plans[name] = (counts, ids, w16)
            out["plan_%s_args" % name] = np.array([orate[0], orate[1], sqnr, ffa, fa], dtype=np.int64)
            out["plan_%s_times" % name] = np.array(t, dtype=np.float64)
            out["plan_%s_n" % name] = np.array(counts, dtype=np.int32)
            out["plan_%s_ids" % name] = np.array(ids, dtype=np.int64)
            out["plan_%s_w16" % name] = np.array(w16, dtype=np.uint32)
            out["plan_%s_wd" % name] = np.array(wd, dtype=np.float64)
            out["plan_%s_cutoff" % name] = np.array(cut, dtype=np.int64)
        # the branches the cases exist for are really taken
        assert any(k in (2, 3) for k in plans["r30_to_ntsc_sqnr"][0]), "squelch block not entered"
        assert plans["near_match_sqnr"][2] != plans["near_match"][2], "squelch (sq > 0.01) changed nothing"
        assert 0 in plans["nearer_match_sqnr"][2] and 65536 in plans["nearer_match_sqnr"][2], "squelch (sq <= 0.01) not taken"
        assert max(plans["r60_to_24"][0]) > 2
        assert max(plans["r120_to_5"][0]) >= 20
        for name in ("long_fa2", "long_plain"):
            assert sum(1 for c in out["plan_%s_cutoff" % name] if c >= 32) >= 3, "fewer than three erases in " + name

        for name, (w, h, g, wts) in PIX_CASES.items():
            src = np.stack([R.noise_frame(w, h, 1000 + 17 * k + w) for k in range(len(wts))])
            sf, of = os.path.join(tmp, "px.src"), os.path.join(tmp, "px.out")
            src.tofile(sf)
            subprocess.run([exe, "pixels", repr(float(g)), str(w), str(h), str(len(wts)), sf, of] + [str(x) for x in wts], check=True)
            out["px_%s_src" % name] = src
            out["px_%s_w16" % name] = np.array(wts, dtype=np.uint32)
            out["px_%s_gamma" % name] = np.array(float(g))
            out["px_%s_out" % name] = np.fromfile(of, dtype=np.uint8).reshape(h, w, 4)
    path = os.path.join(HERE, "frameblend_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d arrays)" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
