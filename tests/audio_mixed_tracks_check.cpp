// audio_mixed_tracks_check -- the mixed-track plan of csrc/audio_chain.hpp (a cfg and a warm-up per track) on the host,
// as a stand-alone program (tests/test_audio_mixed_tracks_host.py builds it plain and with the address and
// undefined-behaviour sanitizers and runs it as the program it is).  Linked with csrc/glibc_rand.cpp for the rand() stream.
//
//   audio_mixed_tracks_check IN L W RNGPOS TRACKS CFG...
//
// CFG...: the sets, each as audio_chain_check's.  IN: raw interleaved s16le, the tracks back to back, each in the frame
// size of its set.  L, W: the plan (W -1: every track's own default warm-up).  TRACKS: FRAMES:SET:STATE,... with STATE n
// (NULL: zeros, end state dropped), z (zeros) or the sample count the state starts at.
//
// Asserted: audio_mixed_layout equals a linear walk (plane, seg0, the channel-sample offsets of the tracks that draw, the
// warm-ups); audio_run_mixed_tracks_planned equals audio_run_serial run per track with that track's cfg from that
// track's state, the rand() position running through the tracks that draw -- output bytes, the 30 state values
// bitwise, the counts; a track whose cfg is not enabled is copied, keeps its state and has no segments; the per-track
// segments equal audio_seg_count and the per-track repairs those of audio_run_planned on that track alone with its own
// warm-up.  Prints "mixed: <checks> checks, <bad> bad", the stats and the rand() position behind the call.
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
    uint64_t frames, at;                 // at: first int16 in IN
    int set;
    bool null_state;
    AudioState got, want;                // the state the planned / the serial runs carry
};

int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    std::vector<AudioCfg> cfgs((size_t)(argc - 6));
    for (int i = 6; i < argc; i++)
        if (!read_cfg(argv[i], cfgs[(size_t)(i - 6)])) {
            std::fprintf(stderr, "audio_mixed_tracks_check: bad cfg %s\n", argv[i]);
            return 2;
        }
    const std::vector<int16_t> in = read_s16(argv[1]);
    const uint32_t L = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const long w = std::strtol(argv[3], nullptr, 10);
    const uint32_t plan_w = w < 0 ? 0 : (uint32_t)w;
    const uint32_t *plan_warmup = w < 0 ? nullptr : &plan_w;
    uint64_t pos = std::strtoull(argv[4], nullptr, 10);
    std::vector<Track> tracks;
    uint64_t at = 0;
    for (const char *p = argv[5]; *p;) {
        char *e;
        Track t;
        std::memset(&t, 0, sizeof(t));
        t.frames = std::strtoull(p, &e, 10);
        if (*e != ':') return 2;
        t.set = (int)std::strtol(e + 1, &e, 10);
        if (*e != ':' || t.set < 0 || (size_t)t.set >= cfgs.size()) return 2;
        p = e + 1;
        t.at = at;
        at += t.frames * (uint64_t)cfgs[(size_t)t.set].channels;
        if (*p == 'n') { t.null_state = true; p++; }
        else if (*p == 'z') p++;
        else { t.got.count = t.want.count = std::strtoull(p, &e, 10); p = e; }
        if (*p == ',') p++;
        tracks.push_back(t);
    }
    const int n = (int)tracks.size();
    if (at != in.size()) {
        std::fprintf(stderr, "audio_mixed_tracks_check: %" PRIu64 " samples of tracks, %zu samples of input\n", at, in.size());
        return 2;
    }
    long checks = 0, bad = 0;
    const auto check = [&](bool ok, const char *what, int t) {
        checks++;
        if (!ok) {
            bad++;
            std::fprintf(stderr, "audio_mixed_tracks_check: %s, track %d\n", what, t);
        }
    };
    const uint32_t Lp = L ? L : 1;

    // the layout, against a linear walk
    std::vector<AudioTrackEnt> tab((size_t)n);
    uint64_t hiss_items = 0, plane_frames = 0;
    {
        for (int t = 0; t < n; t++) {
            std::memset(&tab[(size_t)t], 0, sizeof(AudioTrackEnt));
            tab[(size_t)t].set = tracks[(size_t)t].set;
            tab[(size_t)t].frames = cfgs[(size_t)tracks[(size_t)t].set].enabled ? tracks[(size_t)t].frames : 0;
        }
        const uint64_t nseg = audio_mixed_layout(tab.data(), n, cfgs.data(), Lp, plan_warmup, &hiss_items, &plane_frames);
        uint64_t j = 0, plane = 0, hiss = 0;
        for (int t = 0; t < n; t++) {
            const AudioTrackEnt &e = tab[(size_t)t];
            const AudioCfg &c = cfgs[(size_t)e.set];
            check(e.seg0 == j && e.plane == plane && e.hiss0 == hiss, "layout", t);
            check(e.warmup == (plan_warmup ? plan_w : audio_default_warmup(c)), "warm-up", t);
            for (uint64_t jl = 0; jl < audio_seg_count(e.frames, Lp); jl++, j++) {
                const int f = audio_track_of(tab.data(), n, j);
                check(f == t && j - tab[(size_t)f].seg0 == jl, "lookup", t);
            }
            plane += e.frames;
            if (c.enabled && c.hiss_level != 0) hiss += e.frames * (uint64_t)c.channels;
        }
        check(j == nseg && plane == plane_frames && hiss == hiss_items, "totals of the call", -1);
    }

    std::vector<int16_t> want(in.size() + 1, (int16_t)0x5555), got(in.size() + 1, (int16_t)0x5555), alone(in.size() + 1);
    std::vector<int32_t> plane(hiss_items + 1, 0x55555555);
    std::vector<AudioMixedTrackIO> io((size_t)n);
    std::vector<AudioPlanStats> alone_stats((size_t)n);
    for (int t = 0; t < n; t++) {
        Track &tr = tracks[(size_t)t];
        const AudioCfg &c = cfgs[(size_t)tr.set];
        const bool draws = c.enabled && c.hiss_level != 0;
        // the serial run of this track, drawing from the stream where the tracks before it left it
        RandSeq seq(rand_state_at(pos));
        int32_t *h = plane.data() + tab[(size_t)t].hiss0;
        uint64_t drawn = 0;
        AudioState ws;
        std::memset(&ws, 0, sizeof(ws));
        if (!tr.null_state) ws = tr.want;
        AudioState as = ws;
        audio_run_serial(c, ws, in.data() + tr.at, want.data() + tr.at, tr.frames, [&]() {
            const uint32_t r = seq.next();
            h[drawn++] = audio_hiss_num(r, c.hiss_level);
            pos++;
            return r;
        });
        if (!tr.null_state) tr.want = ws;
        check(drawn == (draws ? tr.frames * (uint64_t)c.channels : 0), "draws", t);
        // the single-stream plan on this track alone, with its own warm-up: what its repairs should be
        audio_run_planned(c, as, in.data() + tr.at, alone.data() + tr.at, draws ? h : nullptr, tr.frames, L, tab[(size_t)t].warmup, &alone_stats[(size_t)t]);
        io[(size_t)t].src = in.data() + tr.at;
        io[(size_t)t].dst = got.data() + tr.at;
        io[(size_t)t].frames = tr.frames;
        io[(size_t)t].state = tr.null_state ? nullptr : &tr.got;
        io[(size_t)t].set = tr.set;
    }
    check(plane.back() == 0x55555555, "the draw behind the hiss plane", -1);
    std::vector<AudioPlanStats> stats((size_t)n);
    audio_run_mixed_tracks_planned(cfgs.data(), io.data(), n, hiss_items ? plane.data() : nullptr, L, plan_warmup, stats.data());
    for (int t = 0; t < n; t++) {
        const Track &tr = tracks[(size_t)t];
        const AudioCfg &c = cfgs[(size_t)tr.set];
        check(audio_state_same(tr.got, tr.want), "state", t);
        if (c.enabled) {
            check(stats[(size_t)t].segments == audio_seg_count(tr.frames, Lp), "segments", t);
            check(stats[(size_t)t].segments == alone_stats[(size_t)t].segments && stats[(size_t)t].repaired == alone_stats[(size_t)t].repaired, "repairs", t);
        } else {
            check(stats[(size_t)t].segments == 0 && stats[(size_t)t].repaired == 0, "stats without the chain", t);
        }
        check(std::memcmp(got.data() + tr.at, want.data() + tr.at, (size_t)tr.frames * (size_t)c.channels * 2) == 0, "bytes", t);
    }
    check(got.back() == (int16_t)0x5555, "the sample behind the input", -1);
    std::printf("mixed: %ld checks, %ld bad\n", checks, bad);
    std::printf("stats");
    for (const AudioPlanStats &ps : stats) std::printf(" %" PRIu64 "/%" PRIu64, ps.segments, ps.repaired);
    std::printf("\npos %" PRIu64 "\n", pos);
    return bad ? 1 : 0;
}
