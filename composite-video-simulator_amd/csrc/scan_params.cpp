// scan_params.cpp -- host half of the scanimate stage (include/ntscsim.h: ntscsim_scan_*): the tool's switches, the
// source size it derives from them and the two small definitions the veneer, the CLI and the tests share.  Plain C++:
// no HIP, usable without a GPU.  Line numbers refer to ffmpeg_scanimate.cpp of the reference.
#include <cstdlib>
#include <cstring>

#include "ntscsim.h"

namespace {

void preset(ntscsim_scan_params *p, int std_, int num, int den, int w, int h, int pal)   // preset_*() :601-635
{
    p->tv_standard = std_;
    p->field_rate_num = num;
    p->field_rate_den = den;
    p->output_width = w;
    p->output_height = h;
    p->output_pal = pal;
}

void derive_source_size(ntscsim_scan_params *p)                                 // :190-197
{
    if (p->input_ntsc) {
        p->src_width = 480;
        p->src_height = p->output_pal ? 576 : 480;
    } else {
        p->src_width = 600;
        p->src_height = 800;
    }
}

} // namespace

extern "C" void ntscsim_scan_params_init(ntscsim_scan_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    preset(p, 0, 60000, 1001, 720, 480, 0);                                     // preset_NTSC(), called first by main() :977
    derive_source_size(p);
}

extern "C" int ntscsim_scan_parse_argv(ntscsim_scan_params *p, int argc, const char *const *argv, int require_io)
{
    if (!p || p->struct_size != sizeof(*p) || argc < 0 || (argc > 0 && !argv)) return NTSCSIM_E_ARG;
    // `a = argv[i++]; if (a == NULL) return 1;` -- argv[argc] is the NULL the tool runs into
    auto value = [&](int &i) -> const char * { return i < argc ? argv[i++] : (i++, nullptr); };
    for (int i = 1; i < argc;) {
        const char *a = argv[i++];
        if (!a) return NTSCSIM_E_ARG;
        if (*a != '-') return NTSCSIM_E_FLAG;                                   // "Unhandled arg" :707-710
        do { a++; } while (*a == '-');
        if (!std::strcmp(a, "h") || !std::strcmp(a, "help")) return NTSCSIM_E_HELP;
        else if (!std::strcmp(a, "width")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->output_width = (int)std::strtoul(a, nullptr, 0);
            if (p->output_width < 32) return NTSCSIM_E_FLAG;                    // :661
        }
        else if (!std::strcmp(a, "i")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->last_input_path = a;
            p->n_inputs++;
        }
        else if (!std::strcmp(a, "o")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->output_path = a;
        }
        else if (!std::strcmp(a, "422")) p->use_422_colorspace = 1;
        else if (!std::strcmp(a, "420")) p->use_422_colorspace = 0;
        else if (!std::strcmp(a, "inntsc")) p->input_ntsc = 1;
        else if (!std::strcmp(a, "tvstd")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;                          // the tool hands the NULL to strcmp
            if (!std::strcmp(a, "pal")) preset(p, 1, 50, 1, 720, 576, 1);
            else if (!std::strcmp(a, "ntsc")) preset(p, 0, 60000, 1001, 720, 480, 0);
            else if (!std::strcmp(a, "720p60")) preset(p, 2, 60000, 1001, 1280, 720, 0);
            else if (!std::strcmp(a, "1080p60")) preset(p, 3, 60000, 1001, 1920, 1080, 0);
            else return NTSCSIM_E_FLAG;                                         // "Unknown tv std" :697-700
        }
        else return NTSCSIM_E_FLAG;                                             // "Unknown switch" :702-705
    }
    if (require_io && (!p->output_path || !*p->output_path)) return NTSCSIM_E_FLAG;   // :713-720
    if (require_io && p->n_inputs == 0) return NTSCSIM_E_FLAG;
    derive_source_size(p);                                                      // when the inputs are opened: behind all of argv
    return NTSCSIM_OK;
}

extern "C" void ntscsim_scan_effect(uint64_t fieldno, uint32_t *effect, uint32_t *ef_field)
{
    // effect = fieldno / 180 is an unsigned int in the tool: the quotient is cut to 32 bits before the product and the % 4
    const uint32_t e = (uint32_t)(fieldno / (60 * 3));
    if (ef_field) *ef_field = (uint32_t)(fieldno - (uint64_t)(e * (uint32_t)(60 * 3)));
    if (effect) *effect = e % 4;
}

extern "C" uint32_t ntscsim_scan_field_of(uint64_t fieldno)
{
    return (uint32_t)((fieldno & 1) ^ 1);
}
