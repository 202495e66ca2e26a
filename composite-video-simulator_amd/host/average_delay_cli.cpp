// average_delay_cli -- ffmpeg_average_delay's command line on raw BGRA frames (no container, no codec: SURVEY.md
// section 2 keeps media I/O out of scope).  Switches are the tool's (ffmpeg_average_delay.cpp:623-708, parsed by
// ntscsim_avg_parse_argv); every -i names a file of raw BGRA frames, -o the file the averaged frames go to.  Because
// the tool has no switch for it and a raw file carries no size, the extension
//     -height <n>    frame height (default: the TV standard's, 480 / 576)
// completes -width.  The loop is the tool's (:1069-1122) with one frame of every input per output frame: the ring of
// -d destination frames is zeroed once (:948-970), frame t is averaged onto slot t % d with field = t and written out.
// It runs until every input has ended; an input that has ended keeps its last frame.  Frames stay in device memory
// between the read and the write.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    std::fprintf(stderr, " -i <input file>               raw BGRA frames; more than one, in order of layering\n");
    std::fprintf(stderr, " -o <output file>              raw BGRA frames\n");
    std::fprintf(stderr, " -d <n>                        Video delay buffer (n frames)\n");
    std::fprintf(stderr, " -n <n>                        New content averaging level (256=100%% 0=0%%)\n");
    std::fprintf(stderr, " -width <w>                    Width in pixels\n");
    std::fprintf(stderr, " -height <h>                   Height in pixels (extension)\n");
    std::fprintf(stderr, " -tvstd <pal|ntsc>, -422, -420\n");
}

int main(int argc, char **argv)
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
    ntscsim_avg_params kp;
    ntscsim_avg_params_init(&kp);
    const int prc = ntscsim_avg_parse_argv(&kp, (int)args.size(), args.data(), 1);
    if (prc == NTSCSIM_E_HELP) { help(argv[0]); return 1; }
    if (prc != NTSCSIM_OK) { std::fprintf(stderr, "Bad or missing switch (see -h)\n"); return 1; }
    if (height > 0) kp.height = (int)height;
    const int W = kp.width, H = kp.height, nl = kp.n_layers, delay = kp.delay;
    const size_t fbytes = (size_t)W * H * 4;

    std::vector<FILE *> fin((size_t)nl);
    for (int l = 0; l < nl; l++) {
        fin[(size_t)l] = std::fopen(kp.layers[l].path, "rb");
        if (!fin[(size_t)l]) { std::fprintf(stderr, "Failed to open %s\n", kp.layers[l].path); return 1; }
    }
    FILE *fout = std::fopen(kp.output_path, "wb");
    if (!fout) { std::fprintf(stderr, "Failed to open %s\n", kp.output_path); return 1; }

    ntscsim_params sp;
    ntscsim_params_init(&sp);
    ntscsim_ctx *ctx = nullptr;
    int rc = ntscsim_create(&sp, 0, &ctx);
    if (rc == NTSCSIM_OK) rc = ntscsim_avg_bind(ctx, &kp);
    if (rc != NTSCSIM_OK) { std::fprintf(stderr, "ntscsim: %s\n", ntscsim_strerror(rc)); return 2; }

    unsigned char *h_buf = nullptr;
    HIPOK(hipHostMalloc((void **)&h_buf, fbytes, hipHostMallocPortable));
    std::vector<unsigned char *> ring((size_t)delay), d_src((size_t)nl);
    for (unsigned char *&p : ring) {
        HIPOK(hipMalloc((void **)&p, fbytes));
        HIPOK(hipMemset(p, 0, fbytes));                                         // the ring is zeroed once :948-970
    }
    for (unsigned char *&p : d_src) HIPOK(hipMalloc((void **)&p, fbytes));
    std::vector<bool> ended((size_t)nl, false), have((size_t)nl, false);
    std::vector<ntscsim_avg_src> lays((size_t)nl);
    uint64_t current = 0;                                                       // the tool's frame counter, the `field` of composite_layer()
    long long nout = 0;
    for (size_t index = 0;; index = (index + 1) % (size_t)delay) {              // :1117-1118
        bool any = false;
        for (int l = 0; l < nl; l++) {
            if (ended[(size_t)l]) continue;
            const size_t got = std::fread(h_buf, 1, fbytes, fin[(size_t)l]);
            if (got != fbytes) {
                if (got) std::fprintf(stderr, "%s ends inside a frame (%zu of %zu bytes): dropped\n", kp.layers[l].path, got, fbytes);
                ended[(size_t)l] = true;
                continue;
            }
            HIPOK(hipMemcpy(d_src[(size_t)l], h_buf, fbytes, hipMemcpyHostToDevice));
            have[(size_t)l] = true;
            any = true;
        }
        if (!any) break;                                                        // every input has ended
        for (int l = 0; l < nl; l++) {
            lays[(size_t)l].src_dev = have[(size_t)l] ? d_src[(size_t)l] : nullptr;   // no frame yet: the early return :808
            lays[(size_t)l].src_linesize = W * 4;
            lays[(size_t)l]._pad = 0;
        }
        ntscsim_avg_desc d;
        d.dst_dev = ring[index]; d.dst_linesize = W * 4; d.width = W; d.height = H; d.n_layers = nl; d.layers = lays.data();
        d.field = current++;
        rc = ntscsim_avg_frames_device(ctx, &d, 1, nullptr);
        if (rc == NTSCSIM_OK) rc = ntscsim_sync(ctx);
        if (rc != NTSCSIM_OK) { std::fprintf(stderr, "average: %s (%s)\n", ntscsim_strerror(rc), ntscsim_last_error(ctx)); return 2; }
        HIPOK(hipMemcpy(h_buf, ring[index], fbytes, hipMemcpyDeviceToHost));
        if (std::fwrite(h_buf, 1, fbytes, fout) != fbytes) { std::fprintf(stderr, "Write failed\n"); return 2; }
        nout++;
    }
    std::fprintf(stderr, "%d layers, %lld frames out\n", nl, nout);
    for (FILE *f : fin) std::fclose(f);
    if (std::fclose(fout) != 0) return 2;
    for (unsigned char *p : ring) (void)hipFree(p);
    for (unsigned char *p : d_src) (void)hipFree(p);
    (void)hipHostFree(h_buf);
    ntscsim_destroy(ctx);
    ntscsim_avg_params_free(&kp);
    return 0;
}
