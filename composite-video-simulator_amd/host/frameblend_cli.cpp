// frameblend_cli -- frameblend's command line on raw BGRA frames (no container, no codec: SURVEY.md section 2 keeps
// media I/O out of scope).  Switches are the tool's (frameblend.cpp:512-634, parsed by ntscsim_blend_parse_argv);
// because a raw file carries neither a size nor a frame rate, -width / -height are required and the extension
//     -ir n[/d]      input frame rate (pts = frame number, time base = d / n; default 24000/1001)
// gives the times.  The loop is the tool's (:901-1121): the first frame, then per output period the read-ahead
// of 30 periods (:910), the end-of-clip test (:924-927), the weights, the blend, one frame written.  Source frames
// live in device memory from the moment they are read until the planner releases them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ntscsim.h"

#define HIPOK(call)                                                                      \
    do {                                                                                 \
        hipError_t e__ = (call);                                                         \
        if (e__ != hipSuccess) {                                                         \
            std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e__));             \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

static void help(const char *arg0)
{
    std::fprintf(stderr, "%s [options]\n", arg0);
    std::fprintf(stderr, " -i <input file>               raw BGRA frames, width x height\n");
    std::fprintf(stderr, " -o <output file>              raw BGRA frames\n");
    std::fprintf(stderr, " -ir <frame rate>              input frame rate n[/d] (extension; default 24000/1001)\n");
    std::fprintf(stderr, " -or <frame rate>\n -width <x>\n -height <x>\n");
    std::fprintf(stderr, " -sqnr                         Squelch frame interpolation when frame rates match (1%% margin)\n");
    std::fprintf(stderr, " -ffa                          Full frame alternate interpolation\n");
    std::fprintf(stderr, " -fa <x>                       Interpolate alternate frames\n");
    std::fprintf(stderr, " -gamma <x>                    Interpolate with gamma correction (number, ntsc, vga)\n");
    std::fprintf(stderr, " -underscan <x>, -422, -420    accepted, no effect on raw frames\n");
}

int main(int argc, char **argv)
{
    // take the extension switch out, hand the rest to the mirror of the tool's parser
    std::vector<const char *> args;
    long ir_num = 24000, ir_den = 1001;
    for (int i = 0; i < argc; i++) {
        const char *a = argv[i];
        const char *s = a;
        while (i > 0 && *s == '-') s++;
        if (i > 0 && a[0] == '-' && !std::strcmp(s, "ir")) {
            if (++i >= argc) return 1;
            char *end = nullptr;
            ir_num = std::strtol(argv[i], &end, 10);
            ir_den = (*end == '/' || *end == ':') ? std::strtol(end + 1, nullptr, 10) : 1;
            if (ir_num < 1 || ir_den < 1) { std::fprintf(stderr, "Bad -ir\n"); return 1; }
            continue;
        }
        args.push_back(a);
    }
    ntscsim_blend_params bp;
    ntscsim_blend_params_init(&bp);
    const int prc = ntscsim_blend_parse_argv(&bp, (int)args.size(), args.data(), 1);
    if (prc == NTSCSIM_E_HELP) { help(argv[0]); return 1; }
    if (prc != NTSCSIM_OK) { std::fprintf(stderr, "Bad or missing switch (see -h)\n"); return 1; }
    if (bp.output_width < 32 || bp.output_height < 32) { std::fprintf(stderr, "Raw frames need -width and -height\n"); return 1; }
    const int W = bp.output_width, H = bp.output_height;
    const size_t fbytes = (size_t)W * H * 4;

    FILE *fin = std::fopen(bp.input_path, "rb");
    if (!fin) { std::fprintf(stderr, "Failed to open %s\n", bp.input_path); return 1; }
    FILE *fout = std::fopen(bp.output_path, "wb");
    if (!fout) { std::fprintf(stderr, "Failed to open %s\n", bp.output_path); return 1; }

    ntscsim_params sp;
    ntscsim_params_init(&sp);
    ntscsim_ctx *ctx = nullptr;
    int rc = ntscsim_create(&sp, 0, &ctx);
    if (rc == NTSCSIM_OK) rc = ntscsim_blend_bind(ctx, &bp);
    ntscsim_blend_plan *plan = nullptr;
    if (rc == NTSCSIM_OK) rc = ntscsim_blend_plan_create(&bp, &plan);
    if (rc != NTSCSIM_OK) { std::fprintf(stderr, "ntscsim: %s\n", ntscsim_strerror(rc)); return 2; }

    unsigned char *h_buf = nullptr, *d_out = nullptr;
    HIPOK(hipHostMalloc((void **)&h_buf, fbytes, hipHostMallocPortable));
    HIPOK(hipMalloc((void **)&d_out, fbytes));
    std::map<int64_t, unsigned char *> live;       // stable id -> device frame
    std::vector<unsigned char *> spare;
    long long nread = 0;
    double last_t = -1e30;
    bool eof = false;
    // one frame from the file into device memory and into the planner; false at end of file
    auto read_frame = [&]() -> int {
        const size_t got = std::fread(h_buf, 1, fbytes, fin);
        if (got != fbytes) {
            if (got) std::fprintf(stderr, "Input ends inside a frame (%zu of %zu bytes): dropped\n", got, fbytes);
            return 0;
        }
        unsigned char *d = nullptr;
        if (!spare.empty()) { d = spare.back(); spare.pop_back(); }
        else if (hipMalloc((void **)&d, fbytes) != hipSuccess) return -1;
        if (hipMemcpy(d, h_buf, fbytes, hipMemcpyHostToDevice) != hipSuccess) return -1;
        last_t = ntscsim_blend_frame_time(nread++, (int32_t)ir_den, (int32_t)ir_num, &bp);
        live[ntscsim_blend_plan_push(plan, last_t)] = d;
        return 1;
    };
    int r = read_frame();                                                      // :896-907
    if (r < 0) return 2;
    if (r == 0) eof = true;
    std::vector<int64_t> ids(64);
    std::vector<uint32_t> w16(64);
    std::vector<ntscsim_blend_tap> taps;
    long long nout = 0;
    for (int64_t current = 0;; current++) {
        while (!eof && last_t < (double)(current + 30)) {                      // :910-922
            r = read_frame();
            if (r < 0) return 2;
            if (r == 0) eof = true;
        }
        if (eof && (last_t < -1000 || current >= ntscsim_blend_clip_periods(last_t))) break;    // :924-927
        int nt = 0;
        int64_t release = 0;
        rc = ntscsim_blend_plan_next(plan, current, ids.data(), w16.data(), (int)ids.size(), &nt, &release);
        if (rc == NTSCSIM_E_SIZE) {
            ids.resize((size_t)nt); w16.resize((size_t)nt);
            rc = ntscsim_blend_plan_next(plan, current, ids.data(), w16.data(), nt, &nt, &release);
        }
        if (rc != NTSCSIM_OK) { std::fprintf(stderr, "planner: %s\n", ntscsim_strerror(rc)); return 2; }
        taps.clear();
        for (int k = 0; k < nt; k++) taps.push_back(ntscsim_blend_tap{live.at(ids[(size_t)k]), W * 4, w16[(size_t)k]});
        ntscsim_blend_desc d;
        d.dst_dev = d_out; d.dst_linesize = W * 4; d.width = W; d.height = H; d.n_taps = nt; d.taps = taps.data();
        rc = ntscsim_blend_frames_device(ctx, &d, 1, nullptr);
        if (rc == NTSCSIM_OK) rc = ntscsim_sync(ctx);
        if (rc != NTSCSIM_OK) { std::fprintf(stderr, "blend: %s (%s)\n", ntscsim_strerror(rc), ntscsim_last_error(ctx)); return 2; }
        HIPOK(hipMemcpy(h_buf, d_out, fbytes, hipMemcpyDeviceToHost));
        if (std::fwrite(h_buf, 1, fbytes, fout) != fbytes) { std::fprintf(stderr, "Write failed\n"); return 2; }
        nout++;
        while (!live.empty() && live.begin()->first < release) {               // :1107-1120
            spare.push_back(live.begin()->second);
            live.erase(live.begin());
        }
    }
    std::fprintf(stderr, "%lld frames in, %lld frames out\n", nread, nout);
    std::fclose(fin);
    if (std::fclose(fout) != 0) return 2;
    for (auto &kv : live) (void)hipFree(kv.second);
    for (unsigned char *p : spare) (void)hipFree(p);
    (void)hipFree(d_out);
    (void)hipHostFree(h_buf);
    ntscsim_blend_plan_destroy(plan);
    ntscsim_destroy(ctx);
    return 0;
}
