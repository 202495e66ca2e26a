// cassette_cli -- ffmpeg_cassette on raw samples: interleaved s16le stereo in, the tool's composite_audio_process()
// (ffmpeg_cassette.cpp:334-416) over it, interleaved s16le stereo out.  Takes the tool's switches:
//
//   cassette_cli [--rng-pos N] [--block N] [--host] <switches of the tool> -i in.s16 -o out.s16
//
// -i / -o "-" are stdin / stdout.  --rng-pos: rand() position of the first draw.  --block N: feed the stream N frames per
// call, as the tool's packets would arrive; the bytes do not depend on it.  Runs ntscsim_cass_host() on the GPU; where
// there is none, or with --host, the same arithmetic (csrc/cass_chain.hpp) runs serially on the host.  Decoding,
// resampling and muxing are the caller's.
//
//   cassette_cli --tracks LIST [--rng-pos N] [--host] <common switches>
//
// A library of tapes, each with its own switches: every line of LIST that is not empty and does not start with # is
// "<in> <out> [switches of the tool for this track]", separated by white space.  A track's parameters are the common
// switches followed by its own, through the tool's parser.  Every tape starts at sample count 0.  All tracks go through
// ONE ntscsim_cass_mixed_tracks_host() call, in the order of the file, the rand() position running through them -- the
// result equals one cassette_cli run per line with --rng-pos chained.  Nothing is written unless every line parses and
// every input can be read.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "cass_chain.hpp"
#include "glibc_rand.hpp"
#include "ntscsim.h"

static ntscsim::CassCfg cfg_of(const ntscsim_cass_params &p)
{
    ntscsim::CassCfg c;
    std::memset(&c, 0, sizeof(c));
    c.pre = p.preemphasis;
    c.post = p.deemphasis;
    c.mono = p.mono;
    c.hiss_level = p.hiss_level;
    c.taps = p.taps;
    c.rate = p.rate;
    c.highpass_hz = p.highpass_hz;
    c.tilt = p.head_tilt;
    c.waver = p.head_tilt_waver;
    c.a_lo = p.alpha_lowpass;
    c.a_hi = p.alpha_highpass;
    c.a_pre = p.alpha_pre;
    c.a_post = p.alpha_post;
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
    ntscsim_cass_params cp;              // its paths cleared: they pointed into the line
    std::vector<int16_t> audio;
    size_t frames;
};

// --tracks: common = argv[0] and the switches every track starts from
static int run_tracks(const std::string &list, bool force_host, unsigned long long rng_pos, const std::vector<const char *> &common)
{
    std::ifstream f(list);
    if (!f) {
        std::fprintf(stderr, "cassette_cli: cannot open %s\n", list.c_str());
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
            std::fprintf(stderr, "cassette_cli: %s:%d: <in> <out> [switches] expected\n", list.c_str(), lineno);
            return 1;
        }
        std::vector<const char *> av(common);
        for (size_t i = 2; i < w.size(); i++) av.push_back(w[i].c_str());
        av.push_back("-i");
        av.push_back(w[0].c_str());
        av.push_back("-o");
        av.push_back(w[1].c_str());
        TrackJob j;
        const int rc = ntscsim_cass_parse_argv(&j.cp, (int)av.size(), av.data(), 1);
        if (rc != NTSCSIM_OK) {
            std::fprintf(stderr, "cassette_cli: %s:%d: %s\n", list.c_str(), lineno, ntscsim_strerror(rc));
            return 1;
        }
        j.cp.input_path = j.cp.output_path = nullptr;
        j.in = w[0];
        j.out = w[1];
        std::vector<unsigned char> bytes;
        if (!read_all(j.in, bytes)) {
            std::fprintf(stderr, "cassette_cli: %s:%d: cannot open %s\n", list.c_str(), lineno, j.in.c_str());
            return 1;
        }
        const size_t fbytes = 2 * sizeof(int16_t);
        j.frames = bytes.size() / fbytes;                                       // a torn last frame is dropped
        if (j.frames > 0xFFFFFFFFull) {
            std::fprintf(stderr, "cassette_cli: %s:%d: more than 2^32-1 frames\n", list.c_str(), lineno);
            return 1;
        }
        j.audio.resize(j.frames * 2 + 1);
        std::memcpy(j.audio.data(), bytes.data(), j.frames * fbytes);
        jobs.push_back(std::move(j));
    }
    const int n = (int)jobs.size();
    ntscsim_ctx *ctx = nullptr;
    if (!force_host && n) {
        ntscsim_params p;
        ntscsim_params_init(&p);
        const int rc = ntscsim_create(&p, 0, &ctx);
        if (rc != NTSCSIM_OK && rc != NTSCSIM_E_NODEV) {
            std::fprintf(stderr, "cassette_cli: %s\n", ntscsim_strerror(rc));
            return 1;
        }
    }
    // where the rand() position stands behind each track: the rule of the call, and what the serial loop counts
    std::vector<unsigned long long> behind((size_t)n);
    if (ctx) {
        std::vector<ntscsim_cass_params> sets;                                  // the distinct ones
        std::vector<ntscsim_cass_desc> descs((size_t)n);
        std::vector<ntscsim_cass_mixed_track> tracks((size_t)n);
        unsigned long long pos = rng_pos;
        for (int t = 0; t < n; t++) {
            TrackJob &j = jobs[(size_t)t];
            size_t s = 0;
            while (s < sets.size() && std::memcmp(&sets[s], &j.cp, sizeof(j.cp)) != 0) s++;
            if (s == sets.size()) sets.push_back(j.cp);
            std::memset(&descs[(size_t)t], 0, sizeof(ntscsim_cass_desc));
            descs[(size_t)t].src = descs[(size_t)t].dst = j.audio.data();
            descs[(size_t)t].samples = (uint32_t)j.frames;
            descs[(size_t)t].rng_pos = NTSCSIM_RNG_AUTO;
            tracks[(size_t)t].blocks = &descs[(size_t)t];
            tracks[(size_t)t].n_blocks = 1;
            tracks[(size_t)t].set = (int32_t)s;
            tracks[(size_t)t].count = 0;                                        // every tape starts at its beginning
            tracks[(size_t)t].state = nullptr;
            if (j.cp.hiss_level != 0) pos += (unsigned long long)j.frames * 2;
            behind[(size_t)t] = pos;
        }
        int rc = ntscsim_cass_bind(ctx, &jobs[0].cp);
        ntscsim_set_rng_pos(ctx, rng_pos);
        if (rc == NTSCSIM_OK) rc = ntscsim_cass_mixed_tracks_host(ctx, sets.data(), (int)sets.size(), tracks.data(), n);
        if (rc != NTSCSIM_OK || (unsigned long long)ntscsim_get_rng_pos(ctx) != pos) {
            std::fprintf(stderr, "cassette_cli: %s (%s)\n", ntscsim_strerror(rc), ntscsim_last_error(ctx));
            return 1;
        }
        ntscsim_destroy(ctx);
    } else {
        unsigned long long pos = rng_pos;
        std::vector<ntscsim::CassState> st(1);
        std::vector<double> tf;
        for (int t = 0; t < n; t++) {
            TrackJob &j = jobs[(size_t)t];
            const ntscsim::CassCfg c = cfg_of(j.cp);
            std::memset(st.data(), 0, sizeof(ntscsim::CassState));
            st[0].taps = (uint32_t)c.taps;
            ntscsim::RandSeq seq(ntscsim::rand_state_at(pos));
            tf.resize(j.frames + 1);
            ntscsim::cass_fill_tilt(c, 0, j.frames, tf.data());
            ntscsim::cass_run_serial(c, st[0], j.audio.data(), j.audio.data(), j.frames, tf.data(), [&]() { pos++; return seq.next(); });
            behind[(size_t)t] = pos;
        }
    }
    for (int t = 0; t < n; t++) {
        const TrackJob &j = jobs[(size_t)t];
        std::fprintf(stderr, "cassette_cli: track %d: %zu frames, %d taps, on the %s, rand() position %llu\n", t, j.frames, j.cp.taps,
                     ctx ? "device" : "host", behind[(size_t)t]);
        FILE *out = j.out == "-" ? stdout : std::fopen(j.out.c_str(), "wb");
        if (!out) {
            std::fprintf(stderr, "cassette_cli: cannot open %s\n", j.out.c_str());
            return 1;
        }
        const bool ok = std::fwrite(j.audio.data(), 2 * sizeof(int16_t), j.frames, out) == j.frames && std::fflush(out) == 0;
        if (out != stdout) std::fclose(out);
        if (!ok) return 1;
    }
    return 0;
}

int main(int argc, char **argv)
{
    bool force_host = false;
    unsigned long long rng_pos = 0, block = 0;
    std::string tracks_list;
    std::vector<const char *> rest;
    rest.push_back(argv[0]);
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--rng-pos" && i + 1 < argc) rng_pos = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--block" && i + 1 < argc) block = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--host") force_host = true;
        else if (a == "--tracks" && i + 1 < argc) tracks_list = argv[++i];
        else rest.push_back(argv[i]);
    }
    if (!tracks_list.empty()) return run_tracks(tracks_list, force_host, rng_pos, rest);
    ntscsim_cass_params cp;
    int rc = ntscsim_cass_parse_argv(&cp, (int)rest.size(), rest.data(), 1);
    if (rc != NTSCSIM_OK) {
        std::fprintf(stderr, "cassette_cli: %s\n", ntscsim_strerror(rc));
        return 1;
    }
    const std::string in_path = cp.input_path, out_path = cp.output_path;
    FILE *in = in_path == "-" ? stdin : std::fopen(in_path.c_str(), "rb");
    if (!in) {
        std::fprintf(stderr, "cassette_cli: cannot open %s\n", in_path.c_str());
        return 1;
    }
    std::vector<unsigned char> bytes;                                           // a pipe delivers in pieces: gather them all
    unsigned char buf[65536];
    for (size_t got; (got = std::fread(buf, 1, sizeof(buf), in)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
    if (in != stdin) std::fclose(in);
    const size_t fbytes = 2 * sizeof(int16_t);
    const size_t frames = bytes.size() / fbytes;                                // a torn last frame is dropped
    std::vector<int16_t> audio(frames * 2 + 1);
    std::memcpy(audio.data(), bytes.data(), frames * fbytes);
    if (block == 0 || block > 0xFFFFFFFFull) block = 0xFFFFFFFFull;

    ntscsim_ctx *ctx = nullptr;
    if (!force_host) {
        ntscsim_params p;
        ntscsim_params_init(&p);
        rc = ntscsim_create(&p, 0, &ctx);
        if (rc != NTSCSIM_OK && rc != NTSCSIM_E_NODEV) {
            std::fprintf(stderr, "cassette_cli: %s\n", ntscsim_strerror(rc));
            return 1;
        }
    }
    if (ctx) {
        rc = ntscsim_cass_bind(ctx, &cp);
        ntscsim_set_rng_pos(ctx, rng_pos);
        for (size_t f = 0; rc == NTSCSIM_OK && f < frames; f += (size_t)block) {
            const size_t n = frames - f < block ? frames - f : (size_t)block;
            rc = ntscsim_cass_host(ctx, audio.data() + f * 2, (uint32_t)n);
        }
        if (rc != NTSCSIM_OK) {
            std::fprintf(stderr, "cassette_cli: %s (%s)\n", ntscsim_strerror(rc), ntscsim_last_error(ctx));
            return 1;
        }
        std::fprintf(stderr, "cassette_cli: %zu frames, %d taps, on the device, rand() position %llu\n", frames, cp.taps,
                     (unsigned long long)ntscsim_get_rng_pos(ctx));
        ntscsim_destroy(ctx);
    } else {
        const ntscsim::CassCfg c = cfg_of(cp);
        std::vector<ntscsim::CassState> st(1);
        std::memset(st.data(), 0, sizeof(ntscsim::CassState));
        st[0].taps = (uint32_t)c.taps;
        ntscsim::RandSeq seq(ntscsim::rand_state_at(rng_pos));
        unsigned long long draws = 0;
        std::vector<double> tf;
        for (size_t f = 0; f < frames; f += (size_t)block) {
            const size_t n = frames - f < block ? frames - f : (size_t)block;
            int16_t *a = audio.data() + f * 2;
            tf.resize(n);
            ntscsim::cass_fill_tilt(c, st[0].front.count, n, tf.data());
            ntscsim::cass_run_serial(c, st[0], a, a, n, tf.data(), [&]() { draws++; return seq.next(); });
        }
        std::fprintf(stderr, "cassette_cli: %zu frames, %d taps, on the host, rand() position %llu\n", frames, cp.taps, rng_pos + draws);
    }
    FILE *out = out_path == "-" ? stdout : std::fopen(out_path.c_str(), "wb");
    if (!out) {
        std::fprintf(stderr, "cassette_cli: cannot open %s\n", out_path.c_str());
        return 1;
    }
    const bool ok = std::fwrite(audio.data(), fbytes, frames, out) == frames && std::fflush(out) == 0;
    if (out != stdout) std::fclose(out);
    return ok ? 0 : 1;
}
