// vhsaudio_cli -- the audio half of ffmpeg_ntsc / ffmpeg_to_composite on raw samples: interleaved s16le in, the tool's
// composite_audio_process() (ffmpeg_ntsc.cpp:889-970) over it, interleaved s16le out.  Takes the tool's switches:
//
//   vhsaudio_cli [--tool to_composite] [--rng-pos N] [--block N] [--host] <switches of the tool> -i in.s16 -o out.s16
//
// -i / -o "-" are stdin / stdout.  The channel count follows the switches (2, or 1 for VHS linear audio).  --rng-pos:
// rand() position of the first draw (the tool's video noise shares the stream).  --block N: feed the stream N frames per
// call, as the tool's packets would arrive; the bytes do not depend on it.  Runs ntscsim_audio_host() on the GPU; where
// there is none, or with --host, the same arithmetic (csrc/audio_chain.hpp) runs serially on the host.
//
//   vhsaudio_cli --tracks LIST [--tool to_composite] [--rng-pos N] [--host] <common switches>
//
// Many independent streams, each with its own switches: every line of LIST that is not empty and does not start with #
// is "<in> <out> [switches of the tool for this track]", separated by white space.  A track's parameters are the common
// switches followed by its own, through the tool's parser; its channel count follows them.  All tracks go through ONE
// ntscsim_audio_mixed_tracks_host() call, in the order of the file, the rand() position running through them -- the
// result equals one vhsaudio_cli run per line with --rng-pos chained.  Nothing is written unless every line parses and
// every input can be read.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
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

static bool read_all(const std::string &path, std::vector<unsigned char> &bytes)
{
    FILE *in = path == "-" ? stdin : std::fopen(path.c_str(), "rb");
    if (!in) return false;
    unsigned char buf[65536];                                                   // a pipe delivers in pieces: gather them all
    for (size_t got; (got = std::fread(buf, 1, sizeof(buf), in)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
    if (in != stdin) std::fclose(in);
    return true;
}

struct TrackJob {
    std::string in, out;
    ntscsim_params p;
    ntscsim_audio_params ap;
    std::vector<int16_t> audio;
    size_t frames;
};

// --tracks: common = argv[0] and the switches every track starts from
static int run_tracks(const std::string &list, bool sibling, bool force_host, unsigned long long rng_pos, const std::vector<const char *> &common)
{
    std::ifstream f(list);
    if (!f) {
        std::fprintf(stderr, "vhsaudio_cli: cannot open %s\n", list.c_str());
        return 1;
    }
    std::vector<TrackJob> jobs;
    std::string line;
    for (int lineno = 1; std::getline(f, line); lineno++) {
        std::istringstream words(line);
        std::vector<std::string> w;
        for (std::string x; words >> x;) w.push_back(x);
        if (w.empty() || w[0][0] == '#') continue;
        if (w.size() < 2) {
            std::fprintf(stderr, "vhsaudio_cli: %s:%d: <in> <out> [switches] expected\n", list.c_str(), lineno);
            return 1;
        }
        std::vector<const char *> av(common);
        for (size_t i = 2; i < w.size(); i++) av.push_back(w[i].c_str());
        av.push_back("-i");
        av.push_back(w[0].c_str());
        av.push_back("-o");
        av.push_back(w[1].c_str());
        TrackJob j;
        ntscsim_cli cli;
        ntscsim_cli_init(&cli);
        int rc;
        if (sibling) {
            ntscsim_params_init_to_composite(&j.p);
            rc = ntscsim_params_parse_argv_to_composite(&j.p, &cli, (int)av.size(), av.data(), 1);
        } else {
            ntscsim_params_init(&j.p);
            rc = ntscsim_params_parse_argv(&j.p, &cli, (int)av.size(), av.data(), 1);
        }
        if (rc == NTSCSIM_OK) rc = ntscsim_audio_params_from_cli(&j.ap, &j.p, &cli);
        if (rc != NTSCSIM_OK) {
            std::fprintf(stderr, "vhsaudio_cli: %s:%d: %s\n", list.c_str(), lineno, ntscsim_strerror(rc));
            return 1;
        }
        j.in = w[0];
        j.out = w[1];
        std::vector<unsigned char> bytes;
        if (!read_all(j.in, bytes)) {
            std::fprintf(stderr, "vhsaudio_cli: %s:%d: cannot open %s\n", list.c_str(), lineno, j.in.c_str());
            return 1;
        }
        const size_t fbytes = (size_t)j.ap.channels * sizeof(int16_t);
        j.frames = bytes.size() / fbytes;                                       // a torn last frame is dropped
        if (j.frames > 0xFFFFFFFFull) {
            std::fprintf(stderr, "vhsaudio_cli: %s:%d: more than 2^32-1 frames\n", list.c_str(), lineno);
            return 1;
        }
        j.audio.resize(j.frames * (size_t)j.ap.channels + 1);
        std::memcpy(j.audio.data(), bytes.data(), j.frames * fbytes);
        jobs.push_back(std::move(j));
    }
    const int n = (int)jobs.size();
    ntscsim_ctx *ctx = nullptr;
    if (!force_host && n) {
        const int rc = ntscsim_create(&jobs[0].p, 0, &ctx);
        if (rc != NTSCSIM_OK && rc != NTSCSIM_E_NODEV) {
            std::fprintf(stderr, "vhsaudio_cli: %s\n", ntscsim_strerror(rc));
            return 1;
        }
    }
    // where the rand() position stands behind each track: the rule of the call, and what the serial loop counts
    std::vector<unsigned long long> behind((size_t)n);
    if (ctx) {
        std::vector<ntscsim_audio_params> sets;                                 // the distinct ones
        std::vector<ntscsim_audio_desc> descs((size_t)n);
        std::vector<ntscsim_audio_mixed_track> tracks((size_t)n);
        unsigned long long pos = rng_pos;
        for (int t = 0; t < n; t++) {
            TrackJob &j = jobs[(size_t)t];
            size_t s = 0;
            while (s < sets.size() && std::memcmp(&sets[s], &j.ap, sizeof(j.ap)) != 0) s++;
            if (s == sets.size()) sets.push_back(j.ap);
            std::memset(&descs[(size_t)t], 0, sizeof(ntscsim_audio_desc));
            descs[(size_t)t].src = descs[(size_t)t].dst = j.audio.data();
            descs[(size_t)t].samples = (uint32_t)j.frames;
            descs[(size_t)t].rng_pos = NTSCSIM_RNG_AUTO;
            tracks[(size_t)t].blocks = &descs[(size_t)t];
            tracks[(size_t)t].n_blocks = 1;
            tracks[(size_t)t].set = (int32_t)s;
            tracks[(size_t)t].state = nullptr;
            if (j.ap.enabled && j.ap.hiss_level != 0) pos += (unsigned long long)j.frames * (unsigned)j.ap.channels;
            behind[(size_t)t] = pos;
        }
        int rc = ntscsim_audio_bind(ctx, &jobs[0].ap);
        ntscsim_set_rng_pos(ctx, rng_pos);
        if (rc == NTSCSIM_OK) rc = ntscsim_audio_mixed_tracks_host(ctx, sets.data(), (int)sets.size(), tracks.data(), n);
        if (rc != NTSCSIM_OK || (unsigned long long)ntscsim_get_rng_pos(ctx) != pos) {
            std::fprintf(stderr, "vhsaudio_cli: %s (%s)\n", ntscsim_strerror(rc), ntscsim_last_error(ctx));
            return 1;
        }
        ntscsim_destroy(ctx);
    } else {
        unsigned long long pos = rng_pos;
        for (int t = 0; t < n; t++) {
            TrackJob &j = jobs[(size_t)t];
            const ntscsim::AudioCfg c = cfg_of(j.ap);
            ntscsim::AudioState st;
            std::memset(&st, 0, sizeof(st));
            ntscsim::RandSeq seq(ntscsim::rand_state_at(pos));
            ntscsim::audio_run_serial(c, st, j.audio.data(), j.audio.data(), j.frames, [&]() { pos++; return seq.next(); });
            behind[(size_t)t] = pos;
        }
    }
    for (int t = 0; t < n; t++) {
        const TrackJob &j = jobs[(size_t)t];
        std::fprintf(stderr, "vhsaudio_cli: track %d: %zu frames x %d on the %s, rand() position %llu\n", t, j.frames, j.ap.channels,
                     ctx ? "device" : "host", behind[(size_t)t]);
        FILE *out = j.out == "-" ? stdout : std::fopen(j.out.c_str(), "wb");
        if (!out) {
            std::fprintf(stderr, "vhsaudio_cli: cannot open %s\n", j.out.c_str());
            return 1;
        }
        const bool ok = std::fwrite(j.audio.data(), (size_t)j.ap.channels * sizeof(int16_t), j.frames, out) == j.frames && std::fflush(out) == 0;
        if (out != stdout) std::fclose(out);
        if (!ok) return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    bool sibling = false, force_host = false;
    unsigned long long rng_pos = 0, block = 0;
    std::string tracks_list;
    std::vector<const char *> rest;
    rest.push_back(argv[0]);
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--tool" && i + 1 < argc) sibling = !std::strcmp(argv[++i], "to_composite");
        else if (a == "--rng-pos" && i + 1 < argc) rng_pos = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--block" && i + 1 < argc) block = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--host") force_host = true;
        else if (a == "--tracks" && i + 1 < argc) tracks_list = argv[++i];
        else rest.push_back(argv[i]);
    }
    if (!tracks_list.empty()) return run_tracks(tracks_list, sibling, force_host, rng_pos, rest);
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
