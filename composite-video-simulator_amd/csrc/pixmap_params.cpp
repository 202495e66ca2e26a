// pixmap_params.cpp -- host half of the posterize and colormap stages (include/ntscsim.h: ntscsim_pixmap_*,
// ntscsim_post_*, ntscsim_cmap_*): the tools' switches and their input list.  Plain C++: no HIP, usable without a GPU.
// Line numbers refer to ffmpeg_posterize.cpp of the reference; ffmpeg_colormap.cpp has the same text (:622-693) without
// the -threshhold branch, which `with_threshhold` switches off.
#include <cstdlib>
#include <cstring>

#include "ntscsim.h"

extern "C" void ntscsim_pixmap_params_init(ntscsim_pixmap_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->width = 720;                      // preset_NTSC() :604-611, called first by main() :816
    p->height = 480;
    p->field_rate_num = 60000;
    p->field_rate_den = 1001;
}

extern "C" void ntscsim_pixmap_params_free(ntscsim_pixmap_params *p)
{
    if (!p || p->struct_size != sizeof(*p)) return;
    std::free(p->layers);
    p->layers = nullptr;
    p->n_layers = p->layers_cap = 0;
}

// new_input_file() :569-587: an input that copies the one before, but for its path; InputFile() :71 for the first
static int pixmap_add_layer(ntscsim_pixmap_params *p, const char *path)
{
    if (p->n_layers < 0 || p->n_layers > p->layers_cap) return NTSCSIM_E_ARG;
    if (p->n_layers == p->layers_cap) {
        const int cap = p->layers_cap ? p->layers_cap * 2 : 4;
        void *m = std::realloc(p->layers, (size_t)cap * sizeof(ntscsim_pixmap_layer));
        if (!m) return NTSCSIM_E_NOMEM;
        p->layers = static_cast<ntscsim_pixmap_layer *>(m);
        p->layers_cap = cap;
    }
    ntscsim_pixmap_layer &l = p->layers[p->n_layers];
    std::memset(&l, 0, sizeof(l));
    l.threshhold = p->n_layers > 0 ? p->layers[p->n_layers - 1].threshhold : 3;
    l.path = path;
    return p->n_layers++;
}

extern "C" int ntscsim_pixmap_parse_argv(ntscsim_pixmap_params *p, int argc, const char *const *argv, int require_io, int with_threshhold)
{
    if (!p || p->struct_size != sizeof(*p) || argc < 0 || (argc > 0 && !argv)) return NTSCSIM_E_ARG;
    // `a = argv[i++]; if (a == NULL) return 1;` -- argv[argc] is the NULL the tool runs into
    auto value = [&](int &i) -> const char * { return i < argc ? argv[i++] : (i++, nullptr); };
    for (int i = 1; i < argc;) {
        const char *a = argv[i++];
        if (!a) return NTSCSIM_E_ARG;
        if (*a != '-') return NTSCSIM_E_FLAG;                                   // "Unhandled arg" :680-683
        do { a++; } while (*a == '-');
        if (!std::strcmp(a, "h") || !std::strcmp(a, "help")) return NTSCSIM_E_HELP;
        else if (!std::strcmp(a, "width")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->width = (int)std::strtoul(a, nullptr, 0);
            if (p->width < 32) return NTSCSIM_E_FLAG;                           // :638
        }
        else if (with_threshhold && !std::strcmp(a, "threshhold")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (p->n_layers == 0) return NTSCSIM_E_FLAG;                        // current_input_file() :560-567 throws
            p->layers[p->n_layers - 1].threshhold = (int)std::strtoul(a, nullptr, 0);   // :643
        }
        else if (!std::strcmp(a, "i")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            const int rc = pixmap_add_layer(p, a);
            if (rc < 0) return rc;
        }
        else if (!std::strcmp(a, "o")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->output_path = a;
        }
        else if (!std::strcmp(a, "422")) p->use_422_colorspace = 1;
        else if (!std::strcmp(a, "420")) p->use_422_colorspace = 0;
        else if (!std::strcmp(a, "tvstd")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;                         // the tool hands the NULL to strcmp :662-664
            const bool pal = !std::strcmp(a, "pal");
            if (!pal && std::strcmp(a, "ntsc")) return NTSCSIM_E_FLAG;          // "Unknown tv std" :670-673
            p->output_pal = pal;                                                // preset_PAL() / preset_NTSC() :595-611
            p->width = 720;
            p->height = pal ? 576 : 480;
            p->field_rate_num = pal ? 50 : 60000;
            p->field_rate_den = pal ? 1 : 1001;
        }
        else return NTSCSIM_E_FLAG;                                             // "Unknown switch" :675-678
    }
    if (require_io && (!p->output_path || !*p->output_path)) return NTSCSIM_E_FLAG;   // :686-693
    if (require_io && p->n_layers == 0) return NTSCSIM_E_FLAG;
    return NTSCSIM_OK;
}

extern "C" void ntscsim_post_params_init(ntscsim_post_params *p) { ntscsim_pixmap_params_init(p); }
extern "C" void ntscsim_post_params_free(ntscsim_post_params *p) { ntscsim_pixmap_params_free(p); }
extern "C" int ntscsim_post_parse_argv(ntscsim_post_params *p, int argc, const char *const *argv, int require_io)
{
    return ntscsim_pixmap_parse_argv(p, argc, argv, require_io, 1);
}

extern "C" void ntscsim_cmap_params_init(ntscsim_cmap_params *p) { ntscsim_pixmap_params_init(p); }
extern "C" void ntscsim_cmap_params_free(ntscsim_cmap_params *p) { ntscsim_pixmap_params_free(p); }
extern "C" int ntscsim_cmap_parse_argv(ntscsim_cmap_params *p, int argc, const char *const *argv, int require_io)
{
    return ntscsim_pixmap_parse_argv(p, argc, argv, require_io, 0);
}
