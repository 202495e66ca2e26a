// pixmap_inputs.hpp -- what posterize_cli and colormap_cli share, which is everything but the call per output frame:
// the tools' command line (ffmpeg_posterize.cpp:620-696, ffmpeg_colormap.cpp:622-693) on raw BGRA frames (no container,
// no codec: SURVEY.md section 2 keeps media I/O out of scope).  Every -i names a file of raw BGRA frames, -o the file
// the output frames go to.  Because the tools have no switch for it and a raw file carries no size, the extension
//     -height <n>    frame height (default: the TV standard's, 480 / 576)
// completes -width.  The loop is the tools' (`while (!eof)`) with one frame of every input per output frame: it runs
// until every input has ended, an input that has ended keeps its last frame, and an input that has not delivered a
// frame yet is the all-zero frame the tools allocate (:198).  Frames stay in device memory between the read and the write.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ntscsim.h"

struct PixmapTool {
    const char *name;
    const char *help;                                                           // the tool's own switches, for -h
    int (*parse)(ntscsim_pixmap_params *, int, const char *const *, int);
    int (*bind)(ntscsim_ctx *, const ntscsim_pixmap_params *);
    // one output frame: src[l] is the current frame of input l (device, linesize 4 * width), dst the output frame
    int (*frame)(ntscsim_ctx *, const ntscsim_pixmap_params &, unsigned char *const *src, unsigned char *dst);
};

#define PIXMAP_HIPOK(call)                                                               \
    do {                                                                                 \
        hipError_t e__ = (call);                                                         \
        if (e__ != hipSuccess) {                                                         \
            std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e__));             \
            return 2;                                                                    \
        }                                                                                \
    } while (0)

inline int pixmap_cli_main(const PixmapTool &tool, int argc, char **argv)
{
    // take the extension switch out, hand the rest to the mirror of the tool's parser
    std::vector<const char *> args;
    long height = -1;
    for (int i = 0; i < argc; i++) {
        const char *a = argv[i];
        const char *s = a;
        while (i > 0 && *s == '-') s++;
        if (i > 0 && a[0] == '-' && !std::strcmp(s, "height")) {
            if (++i >= argc) return 1;
            height = std::strtol(argv[i], nullptr, 0);
            if (height < 1) { std::fprintf(stderr, "Bad -height\n"); return 1; }
            continue;
        }
        args.push_back(a);
    }
    ntscsim_pixmap_params pp;
    ntscsim_pixmap_params_init(&pp);
    const int prc = tool.parse(&pp, (int)args.size(), args.data(), 1);
    if (prc == NTSCSIM_E_HELP) {
        std::fprintf(stderr, "%s [options]\n", argv[0]);
        std::fprintf(stderr, " -i <input file>               raw BGRA frames; more than one, in order\n");
        std::fprintf(stderr, " -o <output file>              raw BGRA frames\n");
        std::fprintf(stderr, "%s", tool.help);
        std::fprintf(stderr, " -width <w>                    Width in pixels\n");
        std::fprintf(stderr, " -height <h>                   Height in pixels (extension)\n");
        std::fprintf(stderr, " -tvstd <pal|ntsc>, -422, -420\n");
        return 1;
    }
    if (prc != NTSCSIM_OK) { std::fprintf(stderr, "Bad or missing switch (see -h)\n"); return 1; }
    if (height > 0) pp.height = (int)height;
    const int W = pp.width, H = pp.height, nl = pp.n_layers;
    const size_t fbytes = (size_t)W * H * 4;

    std::vector<FILE *> fin((size_t)nl);
    for (int l = 0; l < nl; l++) {
        fin[(size_t)l] = std::fopen(pp.layers[l].path, "rb");
        if (!fin[(size_t)l]) { std::fprintf(stderr, "Failed to open %s\n", pp.layers[l].path); return 1; }
    }
    FILE *fout = std::fopen(pp.output_path, "wb");
    if (!fout) { std::fprintf(stderr, "Failed to open %s\n", pp.output_path); return 1; }

    ntscsim_params sp;
    ntscsim_params_init(&sp);
    ntscsim_ctx *ctx = nullptr;
    int rc = ntscsim_create(&sp, 0, &ctx);
    if (rc == NTSCSIM_OK) rc = tool.bind(ctx, &pp);
    if (rc != NTSCSIM_OK) { std::fprintf(stderr, "ntscsim: %s\n", ntscsim_strerror(rc)); return 2; }

    unsigned char *h_buf = nullptr, *d_dst = nullptr;
    PIXMAP_HIPOK(hipHostMalloc((void **)&h_buf, fbytes, hipHostMallocPortable));
    PIXMAP_HIPOK(hipMalloc((void **)&d_dst, fbytes));
    std::vector<unsigned char *> d_src((size_t)nl);
    for (unsigned char *&p : d_src) {
        PIXMAP_HIPOK(hipMalloc((void **)&p, fbytes));
        PIXMAP_HIPOK(hipMemset(p, 0, fbytes));                                  // nothing decoded yet :198
    }
    std::vector<bool> ended((size_t)nl, false);
    long long nout = 0;
    for (;;) {
        bool any = false;
        for (int l = 0; l < nl; l++) {
            if (ended[(size_t)l]) continue;
            const size_t got = std::fread(h_buf, 1, fbytes, fin[(size_t)l]);
            if (got != fbytes) {
                if (got) std::fprintf(stderr, "%s ends inside a frame (%zu of %zu bytes): dropped\n", pp.layers[l].path, got, fbytes);
                ended[(size_t)l] = true;
                continue;
            }
            PIXMAP_HIPOK(hipMemcpy(d_src[(size_t)l], h_buf, fbytes, hipMemcpyHostToDevice));
            any = true;
        }
        if (!any) break;                                                        // every input has ended
        rc = tool.frame(ctx, pp, d_src.data(), d_dst);
        if (rc == NTSCSIM_OK) rc = ntscsim_sync(ctx);
        if (rc != NTSCSIM_OK) { std::fprintf(stderr, "%s: %s (%s)\n", tool.name, ntscsim_strerror(rc), ntscsim_last_error(ctx)); return 2; }
        PIXMAP_HIPOK(hipMemcpy(h_buf, d_dst, fbytes, hipMemcpyDeviceToHost));
        if (std::fwrite(h_buf, 1, fbytes, fout) != fbytes) { std::fprintf(stderr, "Write failed\n"); return 2; }
        nout++;
    }
    std::fprintf(stderr, "%d inputs, %lld frames out\n", nl, nout);
    for (FILE *f : fin) std::fclose(f);
    if (std::fclose(fout) != 0) return 2;
    for (unsigned char *p : d_src) (void)hipFree(p);
    (void)hipFree(d_dst);
    (void)hipHostFree(h_buf);
    ntscsim_destroy(ctx);
    ntscsim_pixmap_params_free(&pp);
    return 0;
}
