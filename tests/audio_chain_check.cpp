// audio_chain_check -- csrc/audio_chain.hpp on the host, as a stand-alone program (tests/test_audio_*.py build it plain
// and with the address and undefined-behaviour sanitizers and run it as the program it is).  Linked with
// csrc/glibc_rand.cpp for the rand() stream.
//
//   audio_chain_check serial   CFG IN OUT COUNT0 RNGPOS BLOCK   the chain, serially, BLOCK frames per call (0: one call; or
//                                                               blocks=FRAMES:POS,... with a rand() position per block, a = as it stands);
//                                                               prints the final state, the sample count and the rand() position
//   audio_chain_check planned  CFG IN COUNT0 RNGPOS NONSILENT   plan + run + verify + repair for L x W, over calls of unequal
//                                                               length, against the serial run; prints "<n> bad"
//   audio_chain_check tracks   CFG IN OUT RNGPOS SPEC           `serial` per track, each from zeros: the tracks lie back to back
//                                                               in IN, SPEC is a file with a line "FRAMES COUNT0 BLOCKS" per track
//                                                               (BLOCKS as behind blocks=, or - for one block); the rand() position
//                                                               runs through; prints a state line per track
//   audio_chain_check plan     CFG IN COUNT0 RNGPOS L W         one planned call; prints its segments, its repairs and which
//                                                               segments were repaired
//   audio_chain_check converge CFG IN COUNT0 RNGPOS             frames a zero-state run needs to meet the true states bit for
//                                                               bit, from 24 start points; prints the worst and the default W
//   audio_chain_check pulses   CFG COUNT0 N OUT                 audio_pulse_count() of N frames as bytes
//
// CFG: a text file, the fields of AudioCfg in order, doubles as hexadecimal floats.  IN / OUT: raw interleaved s16le.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "audio_chain.hpp"
#include "glibc_rand.hpp"

using namespace ntscsim;

static bool read_cfg(const char *path, AudioCfg &c)
{
    FILE *f = std::fopen(path, "r");
    if (!f) return false;
    char d[14][64];
    int iv[8];
    bool ok = true;
    for (int i = 0; i < 8; i++) ok = ok && std::fscanf(f, "%d", &iv[i]) == 1;
    for (int i = 0; i < 11; i++) ok = ok && std::fscanf(f, "%63s", d[i]) == 1;
    std::fclose(f);
    if (!ok) return false;
    std::memset(&c, 0, sizeof(c));
    c.enabled = iv[0]; c.channels = iv[1]; c.hifi = iv[2]; c.pre = iv[3]; c.post = iv[4]; c.hiss_level = iv[5];
    c.vsync_lines = iv[6]; c.vpulse_end = iv[7];
    double *dv[11] = {&c.rate, &c.highpass_hz, &c.hsync_hz, &c.hpulse_end, &c.buzz, &c.boost_gain, &c.a_lo, &c.a_hi, &c.a_pre, &c.a_post, &c.a_boost};
    for (int i = 0; i < 11; i++) *dv[i] = std::strtod(d[i], nullptr);
    return c.channels >= 1 && c.channels <= 2;
}

static std::vector<int16_t> read_s16(const char *path)
{
    std::vector<int16_t> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    int16_t buf[4096];
    for (size_t g; (g = std::fread(buf, 2, 4096, f)) > 0;) v.insert(v.end(), buf, buf + g);
    std::fclose(f);
    return v;
}

static void print_state(const AudioState &st, uint64_t pos)
{
    std::printf("state");
    for (int i = 0; i < AUDIO_STATE_VALUES; i++) {
        uint64_t u;
        std::memcpy(&u, &st.v[i], 8);
        std::printf(" %016" PRIx64, u);
    }
    std::printf(" count %" PRIu64 " pos %" PRIu64 "\n", st.count, pos);
}

// FRAMES:POS,... -- the chain serially over `frames` frames at a, a call per block; POS "a": where the stream stands
static bool run_blocks(const AudioCfg &c, AudioState &st, int16_t *a, uint64_t frames, const char *spec, uint64_t &pos)
{
    RandSeq seq(rand_state_at(pos));
    uint64_t f = 0;
    for (const char *p = spec; *p;) {
        char *e;
        const uint64_t n = std::strtoull(p, &e, 10);
        if (*e != ':' || f + n > frames) return false;
        p = e + 1;
        if (*p == 'a') p++;
        else {
            pos = std::strtoull(p, &e, 10);
            seq = RandSeq(rand_state_at(pos));
            p = e;
        }
        if (*p == ',') p++;
        int16_t *q = a + f * c.channels;
        audio_run_serial(c, st, q, q, n, [&]() { pos++; return seq.next(); });
        f += n;
    }
    return f == frames;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    AudioCfg c;
    if (!read_cfg(argv[2], c)) {
        std::fprintf(stderr, "audio_chain_check: bad cfg %s\n", argv[2]);
        return 2;
    }
    if (mode == "pulses" && argc == 6) {
        const uint64_t count0 = std::strtoull(argv[3], nullptr, 10), n = std::strtoull(argv[4], nullptr, 10);
        std::vector<uint8_t> out((size_t)n);
        for (uint64_t i = 0; i < n; i++) out[(size_t)i] = (uint8_t)audio_pulse_count(c, count0 + i);
        FILE *f = std::fopen(argv[5], "wb");
        if (!f) return 2;
        std::fwrite(out.data(), 1, out.size(), f);
        std::fclose(f);
        return 0;
    }
    if (mode == "serial" && argc == 8) {
        std::vector<int16_t> a = read_s16(argv[3]);
        const uint64_t frames = a.size() / c.channels;
        AudioState st;
        std::memset(&st, 0, sizeof(st));
        st.count = std::strtoull(argv[5], nullptr, 10);
        uint64_t pos = std::strtoull(argv[6], nullptr, 10);
        if (!std::strncmp(argv[7], "blocks=", 7)) {
            if (!run_blocks(c, st, a.data(), frames, argv[7] + 7, pos)) return 2;
        } else {
            RandSeq seq(rand_state_at(pos));
            uint64_t block = std::strtoull(argv[7], nullptr, 10);
            if (block == 0) block = frames ? frames : 1;
            for (uint64_t f = 0; f < frames; f += block) {
                const uint64_t n = frames - f < block ? frames - f : block;
                int16_t *p = a.data() + f * c.channels;
                audio_run_serial(c, st, p, p, n, [&]() { pos++; return seq.next(); });
            }
        }
        FILE *f = std::fopen(argv[4], "wb");
        if (!f) return 2;
        std::fwrite(a.data(), 2, (size_t)frames * c.channels, f);
        std::fclose(f);
        print_state(st, pos);
        return 0;
    }
    if (mode == "tracks" && argc == 7) {                                        // `serial` per track, the tracks back to back in IN
        std::vector<int16_t> a = read_s16(argv[3]);
        const uint64_t frames = a.size() / c.channels;
        uint64_t pos = std::strtoull(argv[5], nullptr, 10), at = 0;
        FILE *spec = std::fopen(argv[6], "r");
        if (!spec) return 2;
        std::vector<char> blocks(1 << 20);
        unsigned long long n, count0;
        while (std::fscanf(spec, "%llu %llu %1048575s", &n, &count0, blocks.data()) == 3) {
            AudioState st;
            std::memset(&st, 0, sizeof(st));
            st.count = count0;
            const std::string one = std::to_string(n) + ":a";
            if (at + n > frames || !run_blocks(c, st, a.data() + at * c.channels, n, blocks[0] == '-' ? one.c_str() : blocks.data(), pos)) {
                std::fclose(spec);
                return 2;
            }
            at += n;
            print_state(st, pos);
        }
        std::fclose(spec);
        if (at != frames) return 2;
        FILE *f = std::fopen(argv[4], "wb");
        if (!f) return 2;
        std::fwrite(a.data(), 2, (size_t)frames * c.channels, f);
        std::fclose(f);
        return 0;
    }
    if (mode == "plan" && argc == 8) {                                          // one planned call: what the device's stats must say
        const std::vector<int16_t> in = read_s16(argv[3]);
        const uint64_t frames = in.size() / c.channels;
        AudioState st;
        std::memset(&st, 0, sizeof(st));
        st.count = std::strtoull(argv[4], nullptr, 10);
        std::vector<int32_t> hiss;
        if (c.hiss_level != 0 && c.enabled) {
            RandSeq seq(rand_state_at(std::strtoull(argv[5], nullptr, 10)));
            hiss.resize((size_t)frames * c.channels);
            for (int32_t &h : hiss) h = audio_hiss_num(seq.next(), c.hiss_level);
        }
        std::vector<int16_t> out(in.size() + 1);
        AudioPlanStats ps;
        std::vector<uint64_t> which;
        audio_run_planned(c, st, in.data(), out.data(), hiss.empty() ? nullptr : hiss.data(), frames, (uint32_t)std::strtoul(argv[6], nullptr, 10),
                          (uint32_t)std::strtoul(argv[7], nullptr, 10), &ps, &which);
        std::printf("plan: segments %" PRIu64 " repaired %" PRIu64 " which", ps.segments, ps.repaired);
        for (uint64_t j : which) std::printf(" %" PRIu64, j);
        std::printf("\n");
        return 0;
    }
    if ((mode == "planned" && argc == 7) || (mode == "converge" && argc == 6)) {
        const std::vector<int16_t> in = read_s16(argv[3]);
        const uint64_t frames = in.size() / c.channels;
        AudioState st0;
        std::memset(&st0, 0, sizeof(st0));
        st0.count = std::strtoull(argv[4], nullptr, 10);
        const uint64_t pos0 = std::strtoull(argv[5], nullptr, 10);
        std::vector<int32_t> hiss;                                              // numerators of the whole input
        if (c.hiss_level != 0 && c.enabled) {
            RandSeq seq(rand_state_at(pos0));
            hiss.resize((size_t)frames * c.channels);
            for (int32_t &h : hiss) h = audio_hiss_num(seq.next(), c.hiss_level);
        }
        const int32_t *hp = hiss.empty() ? nullptr : hiss.data();
        if (mode == "planned") {
            const bool nonsilent = std::atoi(argv[6]) != 0;
            std::vector<int16_t> want(in.size() + 1), got(in.size() + 1);
            AudioState ws = st0;                                                // the serial run
            if (c.enabled) audio_run_span(c, ws, in.data(), want.data(), hp, 0, frames);
            else std::memcpy(want.data(), in.data(), in.size() * 2);
            long bad = 0, runs = 0;
            const uint32_t Ls[4] = {1, 63, 64, 1000}, Ws[4] = {0, 1, 64, audio_default_warmup(c)};
            // calls of unequal length: none, one frame, 777 frames, 64 frames (shorter than the default warm-up), the rest
            const uint64_t cuts[4] = {0, 1, 777, 64};
            for (uint32_t L : Ls)
                for (uint32_t W : Ws) {
                    std::fill(got.begin(), got.end(), (int16_t)0x5555);
                    AudioState st = st0;
                    uint64_t at = 0;
                    for (int k = 0; k < 5; k++) {
                        const uint64_t n = k < 4 ? (cuts[k] < frames - at ? cuts[k] : frames - at) : frames - at;
                        AudioPlanStats ps;
                        audio_run_planned(c, st, in.data() + at * c.channels, got.data() + at * c.channels, hp ? hp + at * c.channels : nullptr, n, L, W, &ps);
                        if (c.enabled && ps.segments != audio_seg_count(n, L)) bad++;
                        // W = 0 on input that is not silent: only the segments that start from the carried state pass
                        if (c.enabled && W == 0 && nonsilent && n > 0 && ps.repaired != ps.segments - 1) bad++;
                        at += n;
                    }
                    if (std::memcmp(got.data(), want.data(), in.size() * 2) != 0) bad++;
                    if (c.enabled && !audio_state_same(st, ws)) bad++;
                    runs++;
                }
            std::printf("planned: %ld runs, %ld bad\n", runs, bad);
            print_state(ws, pos0 + hiss.size());
            return bad ? 1 : 0;
        }
        // converge: the true state in front of every frame, then zero-state runs from 24 start points
        std::vector<AudioState> truth((size_t)frames + 1);
        {
            AudioState s = st0;
            for (uint64_t f = 0; f < frames; f++) {
                truth[(size_t)f] = s;
                audio_run_span(c, s, in.data(), nullptr, hp, f, 1);
            }
            truth[(size_t)frames] = s;
        }
        const uint32_t W = audio_default_warmup(c);
        uint64_t worst = 0;
        long unmet = 0, started = 0;
        for (int k = 0; k < 24; k++) {
            const uint64_t p = 1 + (frames - 1) * (uint64_t)k / 24;
            if (p + W > frames) break;                                          // too little input behind it to tell
            AudioState s = audio_spec_state(c, st0, p);
            uint64_t f = p;
            while (f < frames && !audio_state_same(s, truth[(size_t)f])) {
                audio_run_span(c, s, in.data(), nullptr, hp, f, 1);
                f++;
            }
            started++;
            if (!audio_state_same(s, truth[(size_t)f])) unmet++;
            else if (f - p > worst) worst = f - p;
        }
        std::printf("converge: %ld starts, %ld unmet, worst %" PRIu64 " default_warmup %u\n", started, unmet, worst, W);
        return (unmet || worst > W || started == 0) ? 1 : 0;
    }
    return 2;
}
