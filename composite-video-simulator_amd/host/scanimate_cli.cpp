// scanimate_cli -- ffmpeg_scanimate's command line on raw BGRA frames (no container, no codec: SURVEY.md section 2
// keeps media I/O out of scope).  Switches are the tool's (ffmpeg_scanimate.cpp:643-723, parsed by
// ntscsim_scan_parse_argv); -i names a file of raw BGRA source frames of the size the tool scales its input to
// (600 x 800, with -inntsc 480 x 480 or 480 x 576: ntscsim_scan_params.src_width / src_height), -o the file the raw
// BGRA fields go to.  With several -i the tool's output is the last input's (every composite_layer() overwrites the
// frame), so only the last -i is read.  Because the tool has no switch for them and a raw file carries no size or
// length, two extensions:
//     -height <n>    output height (default: the TV standard's)
//     -fields <n>    fields to write; behind the end of the input the last frame repeats (default: one per frame read)
// The loop is the tool's (:1195-1244) with one source frame per output field: the frame is zeroed, field number t is
// drawn from source frame t with field = (t & 1) ^ 1 and written out.
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
    std::fprintf(stderr, " -i <input file>               raw BGRA source frames; the last one given is drawn\n");
    std::fprintf(stderr, " -o <output file>              raw BGRA fields\n");
    std::fprintf(stderr, " -inntsc                       the source is an interlaced 480-line picture\n");
    std::fprintf(stderr, " -width <w>                    Width in pixels\n");
    std::fprintf(stderr, " -height <h>                   Height in pixels (extension)\n");
    std::fprintf(stderr, " -fields <n>                   Fields to write (extension)\n");
    std::fprintf(stderr, " -tvstd <pal|ntsc|720p60|1080p60>, -422, -420\n");
}

int main(int argc, char **argv)
{
    // take the extension switches out, hand the rest to the mirror of the tool's parser
    std::vector<const char *> args;
    long height = -1;
    long long fields = -1;
    for (int i = 0; i < argc; i++) {
        const char *a = argv[i];
        const char *s = a;
        while (i > 0 && *s == '-') s++;
        const bool sw = i > 0 && a[0] == '-';
        if (sw && !std::strcmp(s, "height")) {
            if (++i >= argc) return 1;
            height = std::strtol(argv[i], nullptr, 0);
            if (height < 1) { std::fprintf(stderr, "Bad -height\n"); return 1; }
            continue;
        }
        if (sw && !std::strcmp(s, "fields")) {
            if (++i >= argc) return 1;
            fields = std::strtoll(argv[i], nullptr, 0);
            if (fields < 0) { std::fprintf(stderr, "Bad -fields\n"); return 1; }
            continue;
        }
        args.push_back(a);
    }
    ntscsim_scan_params kp;
    ntscsim_scan_params_init(&kp);
    const int prc = ntscsim_scan_parse_argv(&kp, (int)args.size(), args.data(), 1);
    if (prc == NTSCSIM_E_HELP) { help(argv[0]); return 1; }
    if (prc != NTSCSIM_OK) { std::fprintf(stderr, "Bad or missing switch (see -h)\n"); return 1; }
    if (height > 0) kp.output_height = (int)height;
    const int W = kp.output_width, H = kp.output_height, SW = kp.src_width, SH = kp.src_height;
    const size_t obytes = (size_t)W * H * 4, sbytes = (size_t)SW * SH * 4;

    FILE *fin = std::fopen(kp.last_input_path, "rb");
    if (!fin) { std::fprintf(stderr, "Failed to open %s\n", kp.last_input_path); return 1; }
    FILE *fout = std::fopen(kp.output_path, "wb");
    if (!fout) { std::fprintf(stderr, "Failed to open %s\n", kp.output_path); return 1; }

    ntscsim_params sp;
    ntscsim_params_init(&sp);
    ntscsim_ctx *ctx = nullptr;
    int rc = ntscsim_create(&sp, 0, &ctx);
    if (rc == NTSCSIM_OK) rc = ntscsim_scan_bind(ctx, &kp);
    if (rc != NTSCSIM_OK) { std::fprintf(stderr, "ntscsim: %s\n", ntscsim_strerror(rc)); return 2; }

    unsigned char *h_src = nullptr, *h_out = nullptr, *d_src = nullptr, *d_out = nullptr;
    HIPOK(hipHostMalloc((void **)&h_src, sbytes, hipHostMallocPortable));
    HIPOK(hipHostMalloc((void **)&h_out, obytes, hipHostMallocPortable));
    HIPOK(hipMalloc((void **)&d_src, sbytes));
    HIPOK(hipMalloc((void **)&d_out, obytes));
    uint64_t current = 0;                                                       // the tool's field counter
    bool ended = false, have = false;
    long long nread = 0;
    for (;;) {
        if (fields >= 0 && (long long)current >= fields) break;
        if (!ended) {
            const size_t got = std::fread(h_src, 1, sbytes, fin);
            if (got == sbytes) {
                HIPOK(hipMemcpy(d_src, h_src, sbytes, hipMemcpyHostToDevice));
                have = true;
                nread++;
            } else {
                if (got) std::fprintf(stderr, "%s ends inside a frame (%zu of %zu bytes): dropped\n", kp.last_input_path, got, sbytes);
                ended = true;
            }
        }
        if (ended && (fields < 0 || !have)) break;                               // no length given: one field per frame read
        const void *src = d_src;
        void *out = d_out;
        rc = ntscsim_scan_clip_device(ctx, &src, SW * 4, SW, SH, &out, W * 4, 1, &current, nullptr);   // advances `current`
        if (rc == NTSCSIM_OK) rc = ntscsim_sync(ctx);
        if (rc != NTSCSIM_OK) { std::fprintf(stderr, "scanimate: %s (%s)\n", ntscsim_strerror(rc), ntscsim_last_error(ctx)); return 2; }
        HIPOK(hipMemcpy(h_out, d_out, obytes, hipMemcpyDeviceToHost));
        if (std::fwrite(h_out, 1, obytes, fout) != obytes) { std::fprintf(stderr, "Write failed\n"); return 2; }
    }
    std::fprintf(stderr, "%lld frames in, %llu fields out\n", nread, (unsigned long long)current);
    std::fclose(fin);
    if (std::fclose(fout) != 0) return 2;
    (void)hipFree(d_src);
    (void)hipFree(d_out);
    (void)hipHostFree(h_src);
    (void)hipHostFree(h_out);
    ntscsim_destroy(ctx);
    return 0;
}
