// led_params.cpp -- host half of the vhsled stage (include/ntscsim.h: ntscsim_led_*): the tool's switches.  Plain
// C++: no HIP, usable without a GPU.  Line numbers refer to ffmpeg_vhsled.cpp of the reference.  filmac.cpp has the
// same globals and the same parse_argv(), text for text, at the same lines, so ntscsim_filmac_params_init() and
// _parse_argv() at the end of this file are these functions under the other stage's name.
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "ntscsim.h"

extern "C" void ntscsim_led_params_init(ntscsim_led_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->width = -1;                       // :50-51: taken from the input unless -width / -height say otherwise
    p->height = -1;
    p->gamma_correction = -1;            // :44
    p->field_rate_num = 60000;           // preset_NTSC() :457-460, called first by main() :695
    p->field_rate_den = 1001;
}

extern "C" int ntscsim_led_parse_argv(ntscsim_led_params *p, int argc, const char *const *argv, int require_io)
{
    if (!p || p->struct_size != sizeof(*p) || argc < 0 || (argc > 0 && !argv)) return NTSCSIM_E_ARG;
    // `a = argv[i++]; if (a == NULL) return 1;` -- argv[argc] is the NULL the tool runs into
    auto value = [&](int &i) -> const char * { return i < argc ? argv[i++] : (i++, nullptr); };
    for (int i = 1; i < argc;) {
        const char *a = argv[i++];
        if (!a) return NTSCSIM_E_ARG;
        if (*a != '-') return NTSCSIM_E_FLAG;                                   // "Unhandled arg" :568-571
        do { a++; } while (*a == '-');
        if (!std::strcmp(a, "h") || !std::strcmp(a, "help")) return NTSCSIM_E_HELP;
        else if (!std::strcmp(a, "width")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->width = (int)std::strtoul(a, nullptr, 0);
            if (p->width < 32) return NTSCSIM_E_FLAG;                           // :494
        }
        else if (!std::strcmp(a, "height")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->height = (int)std::strtoul(a, nullptr, 0);
            if (p->height < 32) return NTSCSIM_E_FLAG;                          // :500
        }
        else if (!std::strcmp(a, "gamma")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (std::isdigit((unsigned char)*a)) p->gamma_correction = std::atof(a);
            else if (!std::strcmp(a, "vga") || !std::strcmp(a, "ntsc")) p->gamma_correction = 2.2;
        }
        else if (!std::strcmp(a, "i")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->input_path = a;                                                  // one input: a later -i replaces it :514
        }
        else if (!std::strcmp(a, "or")) {                                       // :516-544
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            int d = 1;
            char *end = nullptr;
            double n = std::strtof(a, &end);
            a = end;
            if (*a == ':' || *a == '/' || *a == '\\') {
                a++;
                d = (int)std::strtoul(a, &end, 10);
                if (d < 1) d = 1;
            }
            if (n < 0) n = 0;
            if ((n / d) < 5) { n = 5; d = 1; }                                   // "can cause problems below 5fps"
            if (d > 1) {
                p->field_rate_num = (int32_t)(long)std::floor(n + 0.5);
                p->field_rate_den = (int32_t)(long)d;
            } else {
                p->field_rate_num = (int32_t)(long)std::floor((n * 10000) + 0.5);
                p->field_rate_den = 10000;
            }
        }
        else if (!std::strcmp(a, "o")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->output_path = a;
        }
        else if (!std::strcmp(a, "underscan")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->underscan = std::atoi(a);
            if (p->underscan < 0) p->underscan = 0;
            if (p->underscan > 99) p->underscan = 99;
        }
        else if (!std::strcmp(a, "422")) p->use_422_colorspace = 1;
        else if (!std::strcmp(a, "420")) p->use_422_colorspace = 0;
        else return NTSCSIM_E_FLAG;                                             // "Unknown switch" :563-566; -fa is one: help() lists it, the parser has no branch for it
    }
    if (require_io && (!p->output_path || !*p->output_path)) return NTSCSIM_E_FLAG;   // :574-581
    if (require_io && (!p->input_path || !*p->input_path)) return NTSCSIM_E_FLAG;
    return NTSCSIM_OK;
}

extern "C" void ntscsim_filmac_params_init(ntscsim_filmac_params *p) { ntscsim_led_params_init(p); }

extern "C" int ntscsim_filmac_parse_argv(ntscsim_filmac_params *p, int argc, const char *const *argv, int require_io)
{
    return ntscsim_led_parse_argv(p, argc, argv, require_io);
}
