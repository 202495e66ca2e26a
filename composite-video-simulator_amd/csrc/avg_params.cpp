// avg_params.cpp -- host half of the average_delay stage (include/ntscsim.h: ntscsim_avg_*): the tool's switches and
// its layer list.  Plain C++: no HIP, usable without a GPU.  Line numbers refer to ffmpeg_average_delay.cpp of the
// reference.
#include <cstdlib>
#include <cstring>

#include "ntscsim.h"

extern "C" void ntscsim_avg_params_init(ntscsim_avg_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->width = 720;                      // preset_NTSC() :606-613, called first by main() :840
    p->height = 480;
    p->delay = 1;                        // output_avstream_video_frame_delay :67
}

extern "C" void ntscsim_avg_params_free(ntscsim_avg_params *p)
{
    if (!p || p->struct_size != sizeof(*p)) return;
    std::free(p->layers);
    p->layers = nullptr;
    p->n_layers = p->layers_cap = 0;
}

extern "C" int ntscsim_avg_params_add_layer(ntscsim_avg_params *p, const char *path)
{
    if (!p || p->struct_size != sizeof(*p) || p->n_layers < 0 || p->n_layers > p->layers_cap) return NTSCSIM_E_ARG;
    if (p->n_layers == p->layers_cap) {
        const int cap = p->layers_cap ? p->layers_cap * 2 : 4;
        void *m = std::realloc(p->layers, (size_t)cap * sizeof(ntscsim_avg_layer));
        if (!m) return NTSCSIM_E_NOMEM;
        p->layers = static_cast<ntscsim_avg_layer *>(m);
        p->layers_cap = cap;
    }
    ntscsim_avg_layer &l = p->layers[p->n_layers];
    if (p->n_layers > 0) l = p->layers[p->n_layers - 1];                        // new_input_file() :571-589
    else {                                                                      // InputFile() :73
        std::memset(&l, 0, sizeof(l));
        l.newlevel = 128;
    }
    l.path = path;                                                              // reset_on_dup() :94-96
    return p->n_layers++;
}

extern "C" int ntscsim_avg_parse_argv(ntscsim_avg_params *p, int argc, const char *const *argv, int require_io)
{
    if (!p || p->struct_size != sizeof(*p) || argc < 0 || (argc > 0 && !argv)) return NTSCSIM_E_ARG;
    // `a = argv[i++]; if (a == NULL) return 1;` -- argv[argc] is the NULL the tool runs into
    auto value = [&](int &i) -> const char * { return i < argc ? argv[i++] : (i++, nullptr); };
    for (int i = 1; i < argc;) {
        const char *a = argv[i++];
        if (!a) return NTSCSIM_E_ARG;
        if (*a != '-') return NTSCSIM_E_FLAG;                                   // "Unhandled arg" :692-695
        do { a++; } while (*a == '-');
        if (!std::strcmp(a, "h") || !std::strcmp(a, "help")) return NTSCSIM_E_HELP;
        else if (!std::strcmp(a, "width")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->width = (int)std::strtoul(a, nullptr, 0);
            if (p->width < 32) return NTSCSIM_E_FLAG;                           // :641
        }
        else if (!std::strcmp(a, "d")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            const unsigned int d = (unsigned int)std::strtoul(a, nullptr, 0);
            if (d == 0 || d > 256) return NTSCSIM_E_FLAG;                        // "Invalid delay" :647-650
            p->delay = (int32_t)d;
        }
        else if (!std::strcmp(a, "n")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (p->n_layers == 0) return NTSCSIM_E_ARG;                          // current_input_file() :562-569 throws
            p->layers[p->n_layers - 1].newlevel = (int)std::strtoul(a, nullptr, 0);   // :655
        }
        else if (!std::strcmp(a, "i")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            const int rc = ntscsim_avg_params_add_layer(p, a);
            if (rc < 0) return rc;
        }
        else if (!std::strcmp(a, "o")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->output_path = a;
        }
        else if (!std::strcmp(a, "422")) p->use_422_colorspace = 1;
        else if (!std::strcmp(a, "420")) p->use_422_colorspace = 0;
        else if (!std::strcmp(a, "tvstd")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;                          // the tool hands the NULL to strcmp
            if (!std::strcmp(a, "pal")) { p->tv_standard = 1; p->width = 720; p->height = 576; }     // :597-604
            else if (!std::strcmp(a, "ntsc")) { p->tv_standard = 0; p->width = 720; p->height = 480; }
            else return NTSCSIM_E_FLAG;                                         // "Unknown tv std" :682-685
        }
        else return NTSCSIM_E_FLAG;                                             // "Unknown switch" :687-690
    }
    if (require_io && (!p->output_path || !*p->output_path)) return NTSCSIM_E_FLAG;   // :698-705
    if (require_io && p->n_layers == 0) return NTSCSIM_E_FLAG;
    return NTSCSIM_OK;
}
