// audio_tracks_check -- the multi-track plan of csrc/audio_chain.hpp on the host, as a stand-alone program
// (tests/test_audio_tracks_host.py builds it plain and with the address and undefined-behaviour sanitizers and runs it as
// the program it is).  Linked with csrc/glibc_rand.cpp for the rand() stream.
//
//   audio_tracks_check CFG IN L W SPLIT RNGPOS TRACKS
//
// CFG: as audio_chain_check's.  IN: raw interleaved s16le, the tracks back to back.  L, W: the plan (W -1: the default
// warm-up).  SPLIT 1: two calls, the first third of every track and then the rest, on the same states.  TRACKS:
// FRAMES:STATE,... with STATE n (NULL: zeros, end state dropped), z (zeros) or the sample count the state starts at.
//
// Asserted: audio_run_tracks_planned equals audio_run_serial run per track from that track's state -- output bytes, the 30
// state values bitwise, the counts -- the per-track segments equal audio_seg_count, the per-track repairs equal those of
// audio_run_planned on that track alone, and audio_track_of maps every
// call-wide segment index to the (track, local segment) a linear walk finds.  Prints "tracks: <checks> checks, <bad> bad".
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
    char d[11][64];
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

struct Track {
    uint64_t frames, at;                 // at: first frame in IN
    bool null_state;
    AudioState got, want;                // the state the planned / the serial runs carry
};

int main(int argc, char **argv)
{
    if (argc != 8) return 2;
    AudioCfg c;
    if (!read_cfg(argv[1], c)) {
        std::fprintf(stderr, "audio_tracks_check: bad cfg %s\n", argv[1]);
        return 2;
    }
    const std::vector<int16_t> in = read_s16(argv[2]);
    const uint32_t L = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    const long w = std::strtol(argv[4], nullptr, 10);
    const uint32_t W = w < 0 ? audio_default_warmup(c) : (uint32_t)w;
    const bool split = std::atoi(argv[5]) != 0;
    uint64_t pos = std::strtoull(argv[6], nullptr, 10);
    std::vector<Track> tracks;
    uint64_t at = 0;
    for (const char *p = argv[7]; *p;) {
        char *e;
        Track t;
        std::memset(&t, 0, sizeof(t));
        t.frames = std::strtoull(p, &e, 10);
        if (*e != ':') return 2;
        p = e + 1;
        t.at = at;
        at += t.frames;
        if (*p == 'n') { t.null_state = true; p++; }
        else if (*p == 'z') p++;
        else { t.got.count = t.want.count = std::strtoull(p, &e, 10); p = e; }
        if (*p == ',') p++;
        tracks.push_back(t);
    }
    const int n = (int)tracks.size();
    if (at * c.channels != in.size()) {
        std::fprintf(stderr, "audio_tracks_check: %" PRIu64 " frames of tracks, %zu samples of input\n", at, in.size());
        return 2;
    }
    const int ch = c.channels;
    const bool hiss_on = c.hiss_level != 0 && c.enabled;
    long checks = 0, bad = 0;
    const auto check = [&](bool ok, const char *what, int t) {
        checks++;
        if (!ok) {
            bad++;
            std::fprintf(stderr, "audio_tracks_check: %s, track %d\n", what, t);
        }
    };

    // the lookup, against a linear walk -- over the whole tracks and over their first thirds
    for (int pass = 0; pass < 2; pass++) {
        std::vector<AudioTrackEnt> tab((size_t)n);
        for (int t = 0; t < n; t++) {
            std::memset(&tab[(size_t)t], 0, sizeof(AudioTrackEnt));
            tab[(size_t)t].frames = pass ? tracks[(size_t)t].frames / 3 : tracks[(size_t)t].frames;
        }
        const uint64_t nseg = audio_tracks_layout(tab.data(), n, L ? L : 1);
        uint64_t j = 0, plane = 0;
        for (int t = 0; t < n; t++) {
            check(tab[(size_t)t].seg0 == j && tab[(size_t)t].plane == plane, "layout", t);
            for (uint64_t jl = 0; jl < audio_seg_count(tab[(size_t)t].frames, L ? L : 1); jl++, j++) {
                const int f = audio_track_of(tab.data(), n, j);
                check(f == t && j - tab[(size_t)f].seg0 == jl, "lookup", t);
            }
            plane += tab[(size_t)t].frames;
        }
        check(j == nseg, "segments of the call", -1);
    }

    std::vector<int16_t> want(in.size() + 1, (int16_t)0x5555), got(in.size() + 1, (int16_t)0x5555), alone(in.size() + 1);
    std::vector<AudioPlanStats> last_stats;
    for (int part = 0; part < (split ? 2 : 1); part++) {
        std::vector<AudioTrackIO> io((size_t)n);
        std::vector<std::vector<int32_t>> hiss((size_t)n);
        std::vector<AudioPlanStats> alone_stats((size_t)n);
        for (int t = 0; t < n; t++) {
            Track &tr = tracks[(size_t)t];
            const uint64_t cut = tr.frames / 3;
            const uint64_t first = split && part == 1 ? cut : 0, frames = !split ? tr.frames : (part == 0 ? cut : tr.frames - cut);
            const size_t off = (size_t)(tr.at + first) * ch;
            // the serial run of this track, drawing from the stream where the tracks before it left it
            RandSeq seq(rand_state_at(pos));
            std::vector<int32_t> &h = hiss[(size_t)t];
            AudioState ws;
            std::memset(&ws, 0, sizeof(ws));
            if (!tr.null_state) ws = tr.want;
            AudioState as = ws;
            audio_run_serial(c, ws, in.data() + off, want.data() + off, frames, [&]() {
                const uint32_t r = seq.next();
                h.push_back(audio_hiss_num(r, c.hiss_level));
                pos++;
                return r;
            });
            if (!tr.null_state) tr.want = ws;
            check(!hiss_on || h.size() == (size_t)frames * ch, "draws", t);
            // the single-track plan on this track alone: what its repairs should be
            audio_run_planned(c, as, in.data() + off, alone.data() + off, hiss_on ? h.data() : nullptr, frames, L, W, &alone_stats[(size_t)t]);
            io[(size_t)t].src = in.data() + off;
            io[(size_t)t].dst = got.data() + off;
            io[(size_t)t].hiss = hiss_on ? h.data() : nullptr;
            io[(size_t)t].frames = frames;
            io[(size_t)t].state = tr.null_state ? nullptr : &tr.got;
        }
        std::vector<AudioPlanStats> stats((size_t)n);
        audio_run_tracks_planned(c, io.data(), n, L, W, stats.data());
        for (int t = 0; t < n; t++) {
            const Track &tr = tracks[(size_t)t];
            check(audio_state_same(tr.got, tr.want), "state", t);
            if (c.enabled) {
                check(stats[(size_t)t].segments == audio_seg_count(io[(size_t)t].frames, L ? L : 1), "segments", t);
                check(stats[(size_t)t].segments == alone_stats[(size_t)t].segments && stats[(size_t)t].repaired == alone_stats[(size_t)t].repaired, "repairs", t);
            } else {
                check(stats[(size_t)t].segments == 0 && stats[(size_t)t].repaired == 0, "stats without the chain", t);
            }
        }
        last_stats = stats;
    }
    // bytes: every track's own frames, and the 0x5555 behind the last
    for (int t = 0; t < n; t++) {
        const Track &tr = tracks[(size_t)t];
        check(std::memcmp(got.data() + tr.at * ch, want.data() + tr.at * ch, (size_t)tr.frames * ch * 2) == 0, "bytes", t);
    }
    check(got.back() == (int16_t)0x5555, "the sample behind the input", -1);
    std::printf("tracks: %ld checks, %ld bad\n", checks, bad);
    std::printf("stats");                                                       // of the last call
    for (const AudioPlanStats &ps : last_stats) std::printf(" %" PRIu64 "/%" PRIu64, ps.segments, ps.repaired);
    std::printf("\npos %" PRIu64 "\n", pos);
    return bad ? 1 : 0;
}
