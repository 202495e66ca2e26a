// colormap_cli -- ffmpeg_colormap's command line on raw BGRA frames; the switches, the inputs and the loop are
// host/pixmap_inputs.hpp, the frame is ntscsim_cmap_frames_device().
#include "pixmap_inputs.hpp"

// :1072-1075: the table from the second input's current frame when there is a second input, then the first input
// through it.  With one -i no table is ever taken and the output is the identity grey of the green channel.
static int cmap_frame(ntscsim_ctx *ctx, const ntscsim_pixmap_params &p, unsigned char *const *src, unsigned char *dst)
{
    const ntscsim_cmap_desc d = {src[0], p.width * 4, 0, dst, p.width * 4, 0, p.n_layers > 1 ? src[1] : nullptr, p.width * 4, 0};
    return ntscsim_cmap_frames_device(ctx, &d, 1, nullptr);
}

int main(int argc, char **argv)
{
    const PixmapTool tool = {"colormap", "", ntscsim_cmap_parse_argv, ntscsim_cmap_bind, cmap_frame};
    return pixmap_cli_main(tool, argc, argv);
}
