// vhsaudio_cli -- the audio half of ffmpeg_ntsc / ffmpeg_to_composite on raw samples: interleaved s16le in, the tool's
// composite_audio_process() (ffmpeg_ntsc.cpp:889-970) over it, interleaved s16le out.  Takes the tool's switches:
//
//   vhsaudio_cli [--tool to_composite] [--rng-pos N] [--block N] [--host] <switches of the tool> -i in.s16 -o out.s16
//
// -i / -o "-" are stdin / stdout.  The channel count follows the switches (2, or 1 for VHS linear audio).  --rng-pos:
// rand() position of the first draw (the tool's video noise shares the stream).  --block N: feed the stream N frames per
// call, as the tool's packets would arrive; the bytes do not depend on it.  Runs ntscsim_audio_host() on the GPU; where
// there is none, or with --host, the same arithmetic (csrc/audio_chain.hpp) runs serially on the host.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "audio_chain.hpp"
#include "glibc_rand.hpp"
#include "ntscsim.h"

static ntscsim::AudioCfg cfg_of(const ntscsim_audio_params &p)
{
    ntscsim::AudioCfg c;
    std::memset(&c, 0, sizeof(c));
    c.enabled = p.enabled;
    c.channels = p.channels;
    c.hifi = p.hifi;
    c.pre = p.preemphasis;
    c.post = p.deemphasis;
    c.hiss_level = p.hiss_level;
    c.vsync_lines = p.vsync_lines;
    c.vpulse_end = p.vpulse_end;
    c.rate = p.rate;
    c.highpass_hz = p.highpass_hz;
    c.hsync_hz = p.hsync_hz;
    c.hpulse_end = p.hpulse_end;
    c.buzz = p.buzz;
    c.boost_gain = p.boost_gain;
    c.a_lo = p.alpha_lowpass;
    c.a_hi = p.alpha_highpass;
    c.a_pre = p.alpha_pre;
    c.a_post = p.alpha_post;
    c.a_boost = p.alpha_boost;
    return c;
}

int main(int argc, char **argv)
{
    bool sibling = false, force_host = false;
    unsigned long long rng_pos = 0, block = 0;
    std::vector<const char *> rest;
    rest.push_back(argv[0]);
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--tool" && i + 1 < argc) sibling = !std::strcmp(argv[++i], "to_composite");
        else if (a == "--rng-pos" && i + 1 < argc) rng_pos = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--block" && i + 1 < argc) block = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--host") force_host = true;
        else rest.push_back(argv[i]);
    }
    ntscsim_params p;
    ntscsim_cli cli;
    ntscsim_cli_init(&cli);
    int rc;
    if (sibling) {
        ntscsim_params_init_to_composite(&p);
        rc = ntscsim_params_parse_argv_to_composite(&p, &cli, (int)rest.size(), rest.data(), 1);
    } else {
        ntscsim_params_init(&p);
        rc = ntscsim_params_parse_argv(&p, &cli, (int)rest.size(), rest.data(), 1);
    }
    if (rc != NTSCSIM_OK) {
        std::fprintf(stderr, "vhsaudio_cli: %s\n", ntscsim_strerror(rc));
        return 1;
    }
    ntscsim_audio_params ap;
    if (ntscsim_audio_params_from_cli(&ap, &p, &cli) != NTSCSIM_OK) return 1;
    const std::string in_path = cli.input_paths[0], out_path = cli.output_path;
    FILE *in = in_path == "-" ? stdin : std::fopen(in_path.c_str(), "rb");
    if (!in) {
        std::fprintf(stderr, "vhsaudio_cli: cannot open %s\n", in_path.c_str());
        return 1;
    }
    std::vector<unsigned char> bytes;                                           // a pipe delivers in pieces: gather them all
    unsigned char buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof(buf), in)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
    if (in != stdin) std::fclose(in);
    const size_t fbytes = (size_t)ap.channels * sizeof(int16_t);
    const size_t frames = bytes.size() / fbytes;                                // a torn last frame is dropped
    std::vector<int16_t> audio(frames * (size_t)ap.channels + 1);
    std::memcpy(audio.data(), bytes.data(), frames * fbytes);
    if (block == 0 || block > 0xFFFFFFFFull) block = 0xFFFFFFFFull;

    ntscsim_ctx *ctx = nullptr;
    if (!force_host) {
        rc = ntscsim_create(&p, 0, &ctx);
        if (rc != NTSCSIM_OK && rc != NTSCSIM_E_NODEV) {
            std::fprintf(stderr, "vhsaudio_cli: %s\n", ntscsim_strerror(rc));
            return 1;
        }
    }
    if (ctx) {
        rc = ntscsim_audio_bind(ctx, &ap);
        ntscsim_set_rng_pos(ctx, rng_pos);
        for (size_t f = 0; rc == NTSCSIM_OK && f < frames; f += (size_t)block) {
            const size_t n = frames - f < block ? frames - f : (size_t)block;
            rc = ntscsim_audio_host(ctx, audio.data() + f * ap.channels, (uint32_t)n);
        }
        if (rc != NTSCSIM_OK) {
            std::fprintf(stderr, "vhsaudio_cli: %s (%s)\n", ntscsim_strerror(rc), ntscsim_last_error(ctx));
            return 1;
        }
        std::fprintf(stderr, "vhsaudio_cli: %zu frames x %d on the device, rand() position %llu\n", frames, ap.channels,
                     (unsigned long long)ntscsim_get_rng_pos(ctx));
        ntscsim_destroy(ctx);
    } else {
        const ntscsim::AudioCfg c = cfg_of(ap);
        ntscsim::AudioState st;
        std::memset(&st, 0, sizeof(st));
        ntscsim::RandSeq seq(ntscsim::rand_state_at(rng_pos));
        unsigned long long draws = 0;
        for (size_t f = 0; f < frames; f += (size_t)block) {
            const size_t n = frames - f < block ? frames - f : (size_t)block;
            int16_t *a = audio.data() + f * ap.channels;
            ntscsim::audio_run_serial(c, st, a, a, n, [&]() { draws++; return seq.next(); });
        }
        std::fprintf(stderr, "vhsaudio_cli: %zu frames x %d on the host, rand() position %llu\n", frames, ap.channels, rng_pos + draws);
    }
    FILE *out = out_path == "-" ? stdout : std::fopen(out_path.c_str(), "wb");
    if (!out) {
        std::fprintf(stderr, "vhsaudio_cli: cannot open %s\n", out_path.c_str());
        return 1;
    }
    const bool ok = std::fwrite(audio.data(), fbytes, frames, out) == frames && std::fflush(out) == 0;
    if (out != stdout) std::fclose(out);
    return ok ? 0 : 1;
}
