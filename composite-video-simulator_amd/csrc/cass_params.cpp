// cass_params.cpp -- the host half of the cassette stage (include/ntscsim.h: ntscsim_cass_*): ffmpeg_cassette's switches
// as parse_argv() :441-590 reads them and the settings composite_audio_process() runs on as :582, :338 and the set-up
// :864-880 derive them.  No HIP in it.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "cass_chain.hpp"
#include "ntscsim.h"

namespace {
double dBFS(double dB) { return std::pow(10.0, dB / 20.0); }   // :57-64
} // namespace

extern "C" void ntscsim_cass_params_init(ntscsim_cass_params *p)
{
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->struct_size = sizeof(*p);
    p->channels = 2;                                           // :448
    p->rate = 44100;                                           // :236
    p->passes = ntscsim::AUDIO_PASSES;                         // :868
    p->hiss_db = -45;                                          // :237
    p->lowpass_hz = 20000;                                     // :446-447
    p->highpass_hz = 20;
    p->emphasis_hz = 4000;                                     // :873, :878
    p->head_tilt = 0.2;                                        // :328-329
    p->head_tilt_waver = 0.5;
    p->transcode_start = p->transcode_end = p->transcode_dur = -1;   // :231-233
    (void)ntscsim_cass_params_derive(p);
}

extern "C" int ntscsim_cass_params_derive(ntscsim_cass_params *p)
{
    if (!p || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    if (p->lowpass_hz == 0 || p->highpass_hz == 0 || p->rate == 0) return NTSCSIM_E_ARG;   // HiLoComboPass::init :198, assert :335
    if (p->lowpass_hz < 0 || p->highpass_hz < 0 || p->rate < 0) return NTSCSIM_E_PARAM;
    const double level = dBFS(p->hiss_db) * 5000;              // :582
    if (!(level >= 0 && level < 1073741824.0)) return NTSCSIM_E_PARAM;
    const double ntaps = std::floor(std::fabs(p->head_tilt * 2) + std::fabs(p->head_tilt * 3) + 7.5);   // :338
    if (!(ntaps <= (double)NTSCSIM_CASS_MAX_TAPS)) return NTSCSIM_E_PARAM;
    p->hiss_level = (int)level;
    p->taps = ntscsim::cass_taps(p->head_tilt);
    p->alpha_lowpass = ntscsim::audio_alpha(p->rate, p->lowpass_hz);
    p->alpha_highpass = ntscsim::audio_alpha(p->rate, p->highpass_hz);
    p->alpha_pre = ntscsim::audio_alpha(p->rate, p->emphasis_hz);
    p->alpha_post = ntscsim::audio_alpha(p->rate, p->emphasis_hz);
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cass_parse_argv(ntscsim_cass_params *p, int argc, const char *const *argv, int require_io)
{
    if (!p || argc < 0 || (argc > 0 && !argv)) return NTSCSIM_E_ARG;
    ntscsim_cass_params_init(p);                               // :446-448 run at every parse
    int i = 1;
    // the tool reads argv[i++] blindly (argv[argc] is NULL, and a NULL goes to atoi); a missing value is refused here
    const auto value = [&]() -> const char * { return i < argc ? argv[i++] : nullptr; };
    while (i < argc) {
        const char *a = argv[i++];
        if (!a || *a != '-') return NTSCSIM_E_FLAG;            // "Unhandled arg"
        do { a++; } while (*a == '-');
        const char *v = nullptr;
        if (!std::strcmp(a, "h") || !std::strcmp(a, "help")) return NTSCSIM_E_HELP;
        if (!std::strcmp(a, "mono")) { p->mono = 1; continue; }
        if (!std::strcmp(a, "an")) { p->audio_stream_index = -1; continue; }
        static const char *const with_value[] = {"headalign", "headalignwaver", "low", "high", "ss", "se", "t", "a", "audio-hiss", "preemphasis",
                                                 "deemphasis", "i", "o", "preset"};
        bool known = false;
        for (const char *w : with_value) known = known || !std::strcmp(a, w);
        if (!known) return NTSCSIM_E_FLAG;                     // "Unknown switch"
        if (!(v = value())) return NTSCSIM_E_FLAG;
        if (!std::strcmp(a, "headalign")) p->head_tilt = std::atoi(v);
        else if (!std::strcmp(a, "headalignwaver")) p->head_tilt_waver = std::atoi(v);
        else if (!std::strcmp(a, "low")) p->lowpass_hz = (int)std::strtoul(v, nullptr, 0);
        else if (!std::strcmp(a, "high")) p->highpass_hz = (int)std::strtoul(v, nullptr, 0);
        else if (!std::strcmp(a, "ss")) p->transcode_start = std::atof(v);
        else if (!std::strcmp(a, "se")) p->transcode_end = std::atof(v);
        else if (!std::strcmp(a, "t")) p->transcode_dur = std::atof(v);
        else if (!std::strcmp(a, "a")) p->audio_stream_index = std::atoi(v);
        else if (!std::strcmp(a, "audio-hiss")) p->hiss_db = std::atof(v);
        else if (!std::strcmp(a, "preemphasis")) p->preemphasis = std::atoi(v) > 0;
        else if (!std::strcmp(a, "deemphasis")) p->deemphasis = std::atoi(v) > 0;
        else if (!std::strcmp(a, "i")) p->input_path = v;
        else if (!std::strcmp(a, "o")) p->output_path = v;
        else {                                                 // -preset :515-556
            static const struct { double low, high, waver, tilt; } presets[5] = {
                {16000, 100, 0.55, 3.5}, {14000, 100, 0.6, 6}, {10000, 100, 0.5, 3}, {16000, 20, 0.75, 10}, {16000, 20, 0.25, 1.1}};
            const int k = std::atoi(v);
            if (k < 0 || k > 4) return NTSCSIM_E_FLAG;         // "Unknown preset"
            p->lowpass_hz = presets[k].low;
            p->highpass_hz = presets[k].high;
            p->head_tilt_waver = presets[k].waver;
            p->head_tilt = presets[k].tilt;
        }
    }
    // :568-577
    if (p->transcode_start >= 0 && p->transcode_end >= 0) p->transcode_dur = p->transcode_end - p->transcode_start;
    if (p->transcode_start < 0) p->transcode_start = 0;
    if (p->transcode_end < 0 && p->transcode_dur >= 0) p->transcode_end = p->transcode_start + p->transcode_dur;
    if (p->transcode_start >= 0 && p->transcode_end >= 0 && p->transcode_start >= p->transcode_end) return NTSCSIM_E_FLAG;   // "nothing to transcode"
    if (require_io && (!p->input_path || !*p->input_path || !p->output_path || !*p->output_path)) return NTSCSIM_E_FLAG;
    return ntscsim_cass_params_derive(p);
}
