// cassette_cli -- ffmpeg_cassette on raw samples: interleaved s16le stereo in, the tool's composite_audio_process()
// (ffmpeg_cassette.cpp:334-416) over it, interleaved s16le stereo out.  Takes the tool's switches:
//
//   cassette_cli [--rng-pos N] [--block N] [--host] <switches of the tool> -i in.s16 -o out.s16
//
// -i / -o "-" are stdin / stdout.  --rng-pos: rand() position of the first draw.  --block N: feed the stream N frames per
// call, as the tool's packets would arrive; the bytes do not depend on it.  Runs ntscsim_cass_host() on the GPU; where
// there is none, or with --host, the same arithmetic (csrc/cass_chain.hpp) runs serially on the host.  Decoding,
// resampling and muxing are the caller's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

int main(int argc, char **argv)
{
    bool force_host = false;
    unsigned long long rng_pos = 0, block = 0;
    std::vector<const char *> rest;
    rest.push_back(argv[0]);
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--rng-pos" && i + 1 < argc) rng_pos = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--block" && i + 1 < argc) block = std::strtoull(argv[++i], nullptr, 10);
        else if (a == "--host") force_host = true;
        else rest.push_back(argv[i]);
    }
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
