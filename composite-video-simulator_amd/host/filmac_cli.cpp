// filmac_cli -- filmac's command line on raw BGRA frames (no container, no codec: SURVEY.md section 2 keeps media I/O
// out of scope).  Switches are the tool's (filmac.cpp:476-584, parsed by ntscsim_filmac_parse_argv); -i names a file of
// raw BGRA frames, -o the file the stretched frames go to.  The tool takes the frame size from its input when -width /
// -height are not given; a raw file carries none, so here both are required.  Frames go through the device in batches
// of up to 16, each batch one call of ntscsim_filmac_frames_device(); the level state stays on the device between them.
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
    std::fprintf(stderr, " -i <input file>               raw BGRA frames\n");
    std::fprintf(stderr, " -o <output file>              raw BGRA frames\n");
    std::fprintf(stderr, " -width <x>                    required: a raw file carries no size\n");
    std::fprintf(stderr, " -height <x>                   required\n");
    std::fprintf(stderr, " -gamma <x|vga|ntsc>           measure and stretch in linear light\n");
    std::fprintf(stderr, " -or <frame rate>, -underscan <x>, -422, -420    recorded, as in the tool\n");
}

int main(int argc, char **argv)
{
    ntscsim_filmac_params lp;
    ntscsim_filmac_params_init(&lp);
    const int prc = ntscsim_filmac_parse_argv(&lp, argc, argv, 1);
    if (prc == NTSCSIM_E_HELP) { help(argv[0]); return 1; }
    if (prc != NTSCSIM_OK) { std::fprintf(stderr, "Bad or missing switch (see -h)\n"); return 1; }
    if (lp.width < 16 || lp.height < 16) { std::fprintf(stderr, "None or invalid output dimensions\n"); return 1; }   // :705
    const int W = lp.width, H = lp.height, BATCH = 16;
    const size_t fbytes = (size_t)W * H * 4;

    FILE *fin = std::fopen(lp.input_path, "rb");
    if (!fin) { std::fprintf(stderr, "Failed to open %s\n", lp.input_path); return 1; }
    FILE *fout = std::fopen(lp.output_path, "wb");
    if (!fout) { std::fprintf(stderr, "Failed to open %s\n", lp.output_path); return 1; }

    ntscsim_params sp;
    ntscsim_params_init(&sp);
    ntscsim_ctx *ctx = nullptr;
    int rc = ntscsim_create(&sp, 0, &ctx);
    if (rc == NTSCSIM_OK) rc = ntscsim_filmac_bind(ctx, &lp);
    if (rc != NTSCSIM_OK) { std::fprintf(stderr, "ntscsim: %s\n", ntscsim_strerror(rc)); return 2; }

    unsigned char *h_buf = nullptr, *d_src = nullptr, *d_dst = nullptr;
    HIPOK(hipHostMalloc((void **)&h_buf, fbytes * BATCH, hipHostMallocPortable));
    HIPOK(hipMalloc((void **)&d_src, fbytes * BATCH));
    HIPOK(hipMalloc((void **)&d_dst, fbytes * BATCH));
    std::vector<ntscsim_filmac_desc> descs((size_t)BATCH, ntscsim_filmac_desc{});
    long long nout = 0;
    for (bool more = true; more;) {
        int m = 0;
        for (; m < BATCH; m++) {
            const size_t got = std::fread(h_buf + (size_t)m * fbytes, 1, fbytes, fin);
            if (got != fbytes) {
                if (got) std::fprintf(stderr, "%s ends inside a frame (%zu of %zu bytes): dropped\n", lp.input_path, got, fbytes);
                more = false;
                break;
            }
        }
        if (m == 0) break;
        HIPOK(hipMemcpy(d_src, h_buf, fbytes * (size_t)m, hipMemcpyHostToDevice));
        for (int i = 0; i < m; i++) {
            ntscsim_filmac_desc &d = descs[(size_t)i];
            d.src = d_src + (size_t)i * fbytes; d.src_linesize = W * 4;
            d.dst = d_dst + (size_t)i * fbytes; d.dst_linesize = W * 4;
        }
        rc = ntscsim_filmac_frames_device(ctx, descs.data(), m, nullptr);
        if (rc == NTSCSIM_OK) rc = ntscsim_sync(ctx);
        if (rc != NTSCSIM_OK) { std::fprintf(stderr, "filmac: %s (%s)\n", ntscsim_strerror(rc), ntscsim_last_error(ctx)); return 2; }
        HIPOK(hipMemcpy(h_buf, d_dst, fbytes * (size_t)m, hipMemcpyDeviceToHost));
        if (std::fwrite(h_buf, 1, fbytes * (size_t)m, fout) != fbytes * (size_t)m) { std::fprintf(stderr, "Write failed\n"); return 2; }
        nout += m;
    }
    std::fprintf(stderr, "%lld frames out\n", nout);
    std::fclose(fin);
    if (std::fclose(fout) != 0) return 2;
    (void)hipFree(d_src);
    (void)hipFree(d_dst);
    (void)hipHostFree(h_buf);
    ntscsim_destroy(ctx);
    return 0;
}
