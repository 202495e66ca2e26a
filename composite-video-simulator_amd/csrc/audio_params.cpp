// audio_params.cpp -- the host half of the audio stage (include/ntscsim.h: ntscsim_audio_*): the settings
// composite_audio_process() reads, derived from what the two parsers record as ffmpeg_ntsc.cpp:1229-1267 and :2031-2067
// derive them.  No HIP in it.
#include <cmath>
#include <cstring>

#include "audio_chain.hpp"
#include "ntscsim.h"

namespace {
double dBFS(double dB) { return std::pow(10.0, dB / 20.0); }   // :51-58
} // namespace

extern "C" int ntscsim_audio_params_from_cli(ntscsim_audio_params *ap, const ntscsim_params *p, const ntscsim_cli *cli)
{
    if (!ap || !p || !cli || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    std::memset(ap, 0, sizeof(*ap));
    ap->struct_size = sizeof(*ap);
    ap->enabled = p->enable_composite_emulation != 0;          // -nocomp clears both :1052-1053
    ap->rate = 44100;                                          // :212
    ap->passes = ntscsim::AUDIO_PASSES;
    ap->hifi = cli->output_vhs_hifi != 0;
    ap->preemphasis = cli->emulating_preemphasis != 0;
    ap->deemphasis = cli->emulating_deemphasis != 0;
    // :1229-1262 -- output_vhs_linear_audio is !output_vhs_hifi wherever it is set (:1193), and nothing sets
    // output_vhs_linear_stereo
    ap->channels = 2;
    ap->highpass_hz = 20;
    ap->lowpass_hz = 20000;
    if (p->emulating_vhs && !ap->hifi) {
        ap->highpass_hz = 100;
        ap->lowpass_hz = p->output_vhs_tape_speed == NTSCSIM_VHS_EP ? 4000 : (p->output_vhs_tape_speed == NTSCSIM_VHS_LP ? 7000 : 10000);
        ap->channels = 1;
    }
    ap->hiss_level = (int)(dBFS(cli->output_audio_hiss_db) * 5000);   // :1267
    ap->tv_standard = p->tv_standard;
    const bool ntsc = p->tv_standard == NTSCSIM_TV_NTSC;
    ap->hsync_hz = ntsc ? 15734 : 15625;                       // :904-907
    ap->vsync_lines = ntsc ? 525 : 625;
    ap->vpulse_end = ntsc ? 10 : 12;
    ap->hpulse_end = ntsc ? (ap->hsync_hz * (4.7 / 1000000)) : (ap->hsync_hz * (4.0 / 1000000));
    ap->buzz = dBFS(cli->output_audio_linear_buzz);            // :903
    ap->boost_gain = cli->vhs_linear_high_boost;
    ap->boost_hz = 10000;                                      // :2040
    ap->emphasis_hz = ap->hifi ? 16000 : 8000;                 // :2044-2067
    ap->alpha_lowpass = ntscsim::audio_alpha(ap->rate, ap->lowpass_hz);
    ap->alpha_highpass = ntscsim::audio_alpha(ap->rate, ap->highpass_hz);
    ap->alpha_pre = ntscsim::audio_alpha(ap->rate, ap->emphasis_hz);
    ap->alpha_post = ap->alpha_pre;
    ap->alpha_boost = ntscsim::audio_alpha(ap->rate, ap->boost_hz);
    return NTSCSIM_OK;
}
