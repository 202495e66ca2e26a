// posterize_cli -- ffmpeg_posterize's command line on raw BGRA frames; the switches, the inputs and the loop are
// host/pixmap_inputs.hpp, the frame is ntscsim_post_frames_device().
#include "pixmap_inputs.hpp"

// The tool's loop :1035-1062 calls composite_layer() for every input in list order on one output frame, and every call
// overwrites the whole frame with `input & mask` -- nothing of the frame before survives a call.  An input is only
// skipped when it has no frame object (:799), and here every input has one: the all-zero frame before its first read,
// its last frame after its end.  So the output is the last input masked with its own threshhold, and that one
// descriptor is all the library is handed.
static int post_frame(ntscsim_ctx *ctx, const ntscsim_pixmap_params &p, unsigned char *const *src, unsigned char *dst)
{
    const int last = p.n_layers - 1;
    const ntscsim_post_desc d = {src[last], p.width * 4, 0, dst, p.width * 4, last};
    return ntscsim_post_frames_device(ctx, &d, 1, nullptr);
}

int main(int argc, char **argv)
{
    const PixmapTool tool = {"posterize", " -threshhold <n>               Threshhold (8 for no effect, 1 for maximum posterization)\n",
                             ntscsim_post_parse_argv, ntscsim_post_bind, post_frame};
    return pixmap_cli_main(tool, argc, argv);
}
