// blend_params.cpp -- host half of the frameblend stage (include/ntscsim.h: ntscsim_blend_*): the tool's switches,
// frame times, the stateful weight planner and the gamma tables.  Plain C++: no HIP, usable without a GPU.
// Line numbers refer to frameblend.cpp of the reference.
#include <cctype>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "ntscsim.h"

extern "C" void ntscsim_blend_params_init(ntscsim_blend_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->rate_num = 60000;                 // preset_NTSC() :491-494
    p->rate_den = 1001;
    p->output_width = -1;                // :55-56
    p->output_height = -1;
    p->framealt = 1;                     // :47
    p->gamma_correction = -1;            // :49
}

extern "C" int ntscsim_blend_parse_argv(ntscsim_blend_params *p, int argc, const char *const *argv, int require_io)
{
    if (!p || p->struct_size != sizeof(*p) || argc < 0 || (argc > 0 && !argv)) return NTSCSIM_E_ARG;
    // `a = argv[i++]; if (a == NULL) return 1;` -- argv[argc] is the NULL the tool runs into
    auto value = [&](int &i) -> const char * { return i < argc ? argv[i++] : (i++, nullptr); };
    for (int i = 1; i < argc;) {
        const char *a = argv[i++];
        if (!a) return NTSCSIM_E_ARG;
        if (*a != '-') return NTSCSIM_E_FLAG;                                   // "Unhandled arg" :618-621
        do { a++; } while (*a == '-');
        if (!std::strcmp(a, "h") || !std::strcmp(a, "help")) return NTSCSIM_E_HELP;
        else if (!std::strcmp(a, "width")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->output_width = (int)std::strtoul(a, nullptr, 0);
            if (p->output_width < 32) return NTSCSIM_E_FLAG;
        }
        else if (!std::strcmp(a, "height")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->output_height = (int)std::strtoul(a, nullptr, 0);
            if (p->output_height < 32) return NTSCSIM_E_FLAG;
        }
        else if (!std::strcmp(a, "sqnr")) p->squelch_near_match = 1;
        else if (!std::strcmp(a, "ffa")) p->fullframealt = 1;
        else if (!std::strcmp(a, "fa")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->framealt = std::atoi(a);
            if (p->framealt < 1) p->framealt = 1;
            if (p->framealt > 8) p->framealt = 8;
        }
        else if (!std::strcmp(a, "gamma")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            if (std::isdigit((unsigned char)*a)) p->gamma_correction = std::atof(a);
            else if (!std::strcmp(a, "vga") || !std::strcmp(a, "ntsc")) p->gamma_correction = 2.2;
        }
        else if (!std::strcmp(a, "i")) {
            if (!(a = value(i))) return NTSCSIM_E_FLAG;
            p->input_path = a;
            p->n_inputs++;
        }
        else if (!std::strcmp(a, "or")) {                                       // :566-594
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
                p->rate_num = (int32_t)(long)std::floor(n + 0.5);
                p->rate_den = (int32_t)(long)d;
            } else {
                p->rate_num = (int32_t)(long)std::floor((n * 10000) + 0.5);
                p->rate_den = 10000;
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
        else return NTSCSIM_E_FLAG;                                             // "Unknown switch" :613-616
    }
    if (require_io && (!p->output_path || !*p->output_path)) return NTSCSIM_E_FLAG;   // :624-631
    if (require_io && p->n_inputs == 0) return NTSCSIM_E_FLAG;
    return NTSCSIM_OK;
}

extern "C" double ntscsim_blend_frame_time(int64_t pts, int32_t tb_num, int32_t tb_den, const ntscsim_blend_params *p)
{
    if (!p) return 0;
    double n = (double)pts;                                                     // :103-106
    n *= (signed long long)tb_num * (signed long long)p->rate_num;
    n /= (signed long long)tb_den * (signed long long)p->rate_den;
    return n;
}

struct ntscsim_blend_plan {
    bool squelch = false, fullframealt = false;
    int framealt = 1;
    std::vector<double> frame_t;         // the tool's frame_t (its `frames` is used for its size only here)
    int64_t base = 0;                    // frames erased so far: stable id = base + index
    std::vector<std::pair<size_t, double>> weights;
};

extern "C" int ntscsim_blend_plan_create(const ntscsim_blend_params *p, ntscsim_blend_plan **out)
{
    if (!p || !out || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    *out = nullptr;
    if (p->framealt < 1 || p->framealt > 8) return NTSCSIM_E_PARAM;
    ntscsim_blend_plan *pl = new (std::nothrow) ntscsim_blend_plan();
    if (!pl) return NTSCSIM_E_NOMEM;
    pl->squelch = p->squelch_near_match != 0;
    pl->fullframealt = p->fullframealt != 0;
    pl->framealt = p->framealt;
    *out = pl;
    return NTSCSIM_OK;
}

extern "C" void ntscsim_blend_plan_destroy(ntscsim_blend_plan *pl) { delete pl; }

extern "C" void ntscsim_blend_plan_reset(ntscsim_blend_plan *pl)
{
    if (!pl) return;
    pl->frame_t.clear();
    pl->base = 0;
}

extern "C" int64_t ntscsim_blend_plan_push(ntscsim_blend_plan *pl, double t)
{
    if (!pl) return NTSCSIM_E_ARG;
    pl->frame_t.push_back(t);
    return pl->base + (int64_t)pl->frame_t.size() - 1;
}

extern "C" int ntscsim_blend_plan_next(ntscsim_blend_plan *pl, int64_t current_, int64_t *ids, uint32_t *weight16,
                                       int cap, int *n, int64_t *release_below)
{
    if (!pl || !n || cap < 0 || (cap > 0 && (!ids || !weight16)) || current_ < 0) return NTSCSIM_E_ARG;
    const signed long long current = current_;
    const std::vector<double> &frame_t = pl->frame_t;
    const size_t nframes = frame_t.size();
    const int framealt = pl->framealt;
    const bool fullframealt = pl->fullframealt;
    std::vector<std::pair<size_t, double>> &weights = pl->weights;
    weights.clear();
    size_t cutoff = 0;

    if (nframes > 1) {
        if (framealt > 1) {                                                     // :936-961
            for (size_t i = (size_t)((unsigned long long)current % (unsigned long long)framealt);
                 (i + (size_t)framealt) < nframes; i += (size_t)framealt) {
                double bt = frame_t[i];
                double et = frame_t[i + framealt];
                if (i != 0) {
                    if ((et + 2.0) < current) cutoff = i - (i % framealt);
                }
                const signed long long hi = current + (fullframealt ? framealt : 1);
                if (bt < current) bt = current;
                if (bt > hi) bt = hi;
                if (et < current) et = current;
                if (et > hi) et = hi;
                if (bt < et) weights.push_back(std::pair<size_t, double>(i, (et - bt) / (fullframealt ? framealt : 1)));
            }
        } else {                                                                // :964-988
            for (size_t i = 0; (i + 1ul) < nframes; i++) {
                double bt = frame_t[i];
                double et = frame_t[i + 1];
                if (i != 0) {
                    if ((et + 2.0) < current) cutoff = i;
                }
                if (bt < current) bt = current;
                if (bt > (current + 1ll)) bt = (current + 1ll);
                if (et < current) et = current;
                if (et > (current + 1ll)) et = (current + 1ll);
                if (bt < et) weights.push_back(std::pair<size_t, double>(i, et - bt));
            }
        }
    }

    if (weights.size() == 0 && nframes > cutoff) weights.push_back(std::pair<size_t, double>(cutoff, 1.0));   // :992-993

    if (pl->squelch && (weights.size() == 2 || weights.size() == 3)) {          // :995-1023
        const double bt = frame_t[weights[0].first];
        const double et = frame_t[weights[1].first];
        double sq = std::fabs((et - bt) - 1.0) / 0.01;
        if (sq < 1.0) {
            sq = std::pow(sq, 2.0);
            if (sq > 0.01) {
                if (weights[0].second > sq) weights[0].second = sq;
                weights[0].second /= sq;
                weights[1].second = 1.0 - weights[0].second;
            } else {
                weights[0].second = 1.0;
                weights[1].second = 0.0;
            }
            if (weights.size() > 2) weights[2].second = 0.0;
        }
    }

    *n = (int)weights.size();
    if ((int)weights.size() > cap) return NTSCSIM_E_SIZE;
    for (size_t i = 0; i < weights.size(); i++) {
        ids[i] = pl->base + (int64_t)weights[i].first;
        weight16[i] = (unsigned int)std::floor((weights[i].second * 0x10000) + 0.5);   // :1027-1028
    }
    if (cutoff >= 32) {                                                         // :1107-1120
        pl->frame_t.erase(pl->frame_t.begin(), pl->frame_t.begin() + cutoff);
        pl->base += (int64_t)cutoff;
    }
    if (release_below) *release_below = pl->base;
    return NTSCSIM_OK;
}

extern "C" int64_t ntscsim_blend_clip_periods(double last_frame_t)
{
    // :924-927: break at the first current with current > (unsigned long long)ceil(t); periods 0 .. ceil(t) are rendered
    if (!(last_frame_t > -1000)) return 0;
    const double c = std::ceil(last_frame_t);
    return c > 0 ? (int64_t)(unsigned long long)c + 1 : 1;
}

extern "C" int ntscsim_blend_tables(double gamma, uint16_t dec[256], uint8_t enc[8193])
{
    if (!dec || !enc) return NTSCSIM_E_ARG;
    if (!(gamma > 0)) return NTSCSIM_E_PARAM;
    for (unsigned int i = 0; i < 256; i++)                                      // :727-731
        dec[i] = (uint16_t)(unsigned long)(std::pow(i / 255.0, gamma) * 8192);
    for (unsigned int i = 0; i <= 8192; i++)
        enc[i] = (uint8_t)(unsigned long)(std::pow(i / 8192.0, 1.0 / gamma) * 255);
    return NTSCSIM_OK;
}
