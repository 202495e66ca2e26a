// audio_chain.hpp -- the tools' VHS audio chain, composite_audio_process() (ffmpeg_ntsc.cpp:889-970 with the filters of
// :74-203 and their set-up :2031-2067; ffmpeg_to_composite.cpp:558-627 is the same text), stated once for the kernels
// (csrc/ntsc_audio.hip), the host checker (tests/audio_chain_check.cpp) and the command line host's fallback
// (host/vhsaudio_cli.cpp).  No HIP in it.  Built with -ffp-contract=off like everything exact here: every product and
// every sum below is rounded on its own, in the reference's order.
//
// Also here: the PLAN that cuts a call's frames into segments which start early from a zero state, and
// run / verify / repair over that plan, so that a host program executes what the device executes -- for one stream and
// for many independent tracks in one call (the track table and the segment-to-track lookup), with one cfg or one per
// track (the mixed plan).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__)
#define AUDIO_HD __host__ __device__ inline
#else
#define AUDIO_HD inline
#endif

namespace ntscsim {

constexpr int AUDIO_PASSES = 6;          // audio_hilopass.setPasses(6) :2035
constexpr int AUDIO_STATE_VALUES = 30;   // 2 * 12 band-pass, 2 pre, 2 post, 2 boost
constexpr int AUDIO_OVERSAMPLE = 16;     // :927

// what the chain reads of the tool's globals, with every alpha computed by the host (audio_alpha())
struct AudioCfg {
    int enabled;                         // enable_audio_emulation :799 (-nocomp clears it: a copy that draws nothing)
    int channels;                        // output_audio_channels
    int hifi;                            // output_vhs_hifi
    int pre, post;                       // emulating_preemphasis / emulating_deemphasis
    int hiss_level;                      // output_audio_hiss_level :1267
    int vsync_lines, vpulse_end;         // :905-906
    double rate;                         // output_audio_rate
    double highpass_hz;                  // the slowest pole: sets the default warm-up
    double hsync_hz, hpulse_end;         // :904, :907
    double buzz;                         // dBFS(output_audio_linear_buzz) :903
    double boost_gain;                   // vhs_linear_high_boost
    double a_lo, a_hi, a_pre, a_post, a_boost;
};

// v[c*12 + i]: low-pass i of channel c, v[c*12 + 6 + i]: its high-pass; v[24 + i]: pre-emphasis filter i, v[26 + i]:
// de-emphasis filter i (both shared by the channels), v[28 + c]: boost of channel c.  count: audio_proc_count :889
struct AudioState {
    double v[AUDIO_STATE_VALUES];
    uint64_t count;
};

// LowpassFilter::setFilter :78-86
inline double audio_alpha(double rate, double hz)
{
    const double timeInterval = 1.0 / rate;
    const double tau = 1 / (hz * 2 * 3.14159265358979323846);
    return timeInterval / (tau + timeInterval);
}

// LowpassFilter::lowpass :90-94 -- highpass :95-99 is x minus this
AUDIO_HD double audio_pole(double &prev, double x, double alpha)
{
    const double stage1 = x * alpha;
    const double stage2 = prev - (prev * alpha);
    return (prev = (stage1 + stage2));
}

AUDIO_HD bool audio_buzz_on(const AudioCfg &c) { return !c.hifi && c.buzz > 0.000000001; }
AUDIO_HD bool audio_boost_on(const AudioCfg &c) { return !c.hifi && c.boost_gain > 0; }

// How many of the 16 oversample points of frame `count` lie in a sync pulse (:927-941).  fmod(t, 1.0) of a t >= 0 is
// t - floor(t), exactly; floor(...) is a whole number >= 0, so its fmod by vsync_lines / 2.0 is half the remainder of
// twice it by vsync_lines, and the (int) of that drops the half.
AUDIO_HD int audio_pulse_count(const AudioCfg &c, uint64_t count)
{
    int n = 0;
    for (int oi = 0; oi < AUDIO_OVERSAMPLE; oi++) {
        const double t = ((((double)count * AUDIO_OVERSAMPLE) + oi) * c.hsync_hz) / c.rate / AUDIO_OVERSAMPLE;
        const double whole = (double)(uint64_t)t;
        const double hpos = t - whole;
        const double line = (double)(uint64_t)(t + 0.0001 - hpos);       // floor of a value >= 0
        const int vline = (int)((((uint64_t)line * 2u) % (uint64_t)c.vsync_lines) >> 1);
        if (hpos < c.hpulse_end || vline < c.vpulse_end) n++;
    }
    return n;
}

// the numerator of the hiss term :952 for the draw r
AUDIO_HD int audio_hiss_num(uint32_t r, int level) { return (int)(r % (uint32_t)((level * 2) + 1)) - level; }

AUDIO_HD int audio_clips16(int x) { return x < -32768 ? -32768 : (x > 32767 ? 32767 : x); }

// (int)(s * 32768) of :965 is undefined in C++ outside int's range; the chain cannot leave it while the boost gain is
// sane, and a gain that makes it do so saturates here as x86's conversion followed by clips16 would not -- stated, not
// reproduced
AUDIO_HD int16_t audio_pack(double s)
{
    const double v = s * 32768;
    if (!(v > -2147483648.0)) return -32768;
    if (!(v < 2147483647.0)) return 32767;
    return (int16_t)audio_clips16((int)v);
}

// One channel-sample: `in` of channel ch through the chain.  hiss: the numerator of this channel-sample's draw (read
// only when hiss_level != 0); pulses: audio_pulse_count() of this frame (read only when the buzz is on).
AUDIO_HD int16_t audio_sample(const AudioCfg &c, AudioState &st, int ch, int16_t in, int hiss, int pulses)
{
    double s = (double)in / 32768;
    double *bp = st.v + ch * 12;
    for (int i = 0; i < AUDIO_PASSES; i++) s = audio_pole(bp[i], s, c.a_lo);
    for (int i = 0; i < AUDIO_PASSES; i++) s = s - audio_pole(bp[6 + i], s, c.a_hi);
    if (c.pre)
        for (int i = 0; i < c.channels; i++) s = s + (s - audio_pole(st.v[24 + i], s, c.a_pre));
    if (audio_buzz_on(c)) {
        const double q = c.buzz / AUDIO_OVERSAMPLE / 2;
        for (int k = 0; k < pulses; k++) s -= q;
    }
    if (s > 1.0) s = 1.0;
    else if (s < -1.0) s = -1.0;
    if (c.hiss_level != 0) s += ((double)hiss) / 20000;
    if (audio_boost_on(c)) s += (s - audio_pole(st.v[28 + ch], s, c.a_boost)) * c.boost_gain;
    if (c.post)
        for (int i = 0; i < c.channels; i++) s = audio_pole(st.v[26 + i], s, c.a_post);
    return audio_pack(s);
}

// composite_audio_process(audio, frames) from src to dst (dst may be src).  draw(): the next rand(), called once per
// channel-sample when hiss_level != 0 and never otherwise.
template <class Draw>
inline void audio_run_serial(const AudioCfg &c, AudioState &st, const int16_t *src, int16_t *dst, uint64_t frames, Draw &&draw)
{
    if (!c.enabled) {
        if (dst != src) std::memmove(dst, src, (size_t)frames * (size_t)c.channels * sizeof(int16_t));
        return;
    }
    const bool buzz = audio_buzz_on(c);
    for (uint64_t f = 0; f < frames; f++) {
        const int pulses = buzz ? audio_pulse_count(c, st.count) : 0;
        for (int ch = 0; ch < c.channels; ch++) {
            const int h = c.hiss_level != 0 ? audio_hiss_num(draw(), c.hiss_level) : 0;
            dst[f * c.channels + ch] = audio_sample(c, st, ch, src[f * c.channels + ch], h, pulses);
        }
        st.count++;
    }
}

// ------------------------------------------------------------------------------------------------ the plan
// Segment j owns frames [j * L, min((j + 1) * L, total)) of the call and starts running W frames earlier, at
// max(0, start - W).  One whose run starts at frame 0 starts from the carried, true state and is exact by construction;
// every other starts from zeros in the values the chain updates (audio_spec_state()) and is checked afterwards.

// 72 tau of the slowest pole, up to a multiple of 64: 25,280 frames at 20 Hz, 5,056 at 100 Hz
inline uint32_t audio_default_warmup(const AudioCfg &c)
{
    const double tau = c.rate / (2 * 3.14159265358979323846 * c.highpass_hz);
    const uint64_t w = (uint64_t)(72.0 * tau) + 1;
    return (uint32_t)((w + 63) / 64 * 64);
}
constexpr uint32_t AUDIO_DEFAULT_SEG = 4096;

struct AudioSeg {
    uint64_t start, len, run_start;      // frames of the call
};
AUDIO_HD uint64_t audio_seg_count(uint64_t total, uint32_t L) { return (total + L - 1) / L; }
AUDIO_HD AudioSeg audio_seg(uint64_t total, uint32_t L, uint32_t W, uint64_t j)
{
    AudioSeg s;
    s.start = j * (uint64_t)L;
    s.len = total - s.start < L ? total - s.start : L;
    s.run_start = s.start > W ? s.start - W : 0;
    return s;
}

// does the chain update value i of the state?
AUDIO_HD bool audio_value_live(const AudioCfg &c, int i)
{
    if (i < 24) return i / 12 < c.channels;
    if (i < 26) return c.pre && i - 24 < c.channels;
    if (i < 28) return c.post && i - 26 < c.channels;
    return audio_boost_on(c) && i - 28 < c.channels;
}

// the state a speculative segment starts from: zeros where the chain writes, the carried values where it does not
AUDIO_HD AudioState audio_spec_state(const AudioCfg &c, const AudioState &carried, uint64_t run_start)
{
    AudioState s = carried;
    for (int i = 0; i < AUDIO_STATE_VALUES; i++)
        if (audio_value_live(c, i)) s.v[i] = 0;
    s.count = carried.count + run_start;
    return s;
}

AUDIO_HD bool audio_state_same(const AudioState &a, const AudioState &b)
{
    if (a.count != b.count) return false;
    for (int i = 0; i < AUDIO_STATE_VALUES; i++) {
        uint64_t x, y;
        memcpy(&x, &a.v[i], 8);
        memcpy(&y, &b.v[i], 8);
        if (x != y) return false;
    }
    return true;
}

struct AudioPlanStats {
    uint64_t segments, repaired;
    uint64_t worst_convergence;          // host only: most frames a speculative run needed to meet the true states
};

// frames [first, first + n) of the call from state st; hiss: numerators of the whole call (NULL: no hiss)
inline void audio_run_span(const AudioCfg &c, AudioState &st, const int16_t *src, int16_t *dst, const int32_t *hiss, uint64_t first, uint64_t n)
{
    const bool buzz = audio_buzz_on(c);
    for (uint64_t f = first; f < first + n; f++) {
        const int pulses = buzz ? audio_pulse_count(c, st.count) : 0;
        for (int ch = 0; ch < c.channels; ch++) {
            const int16_t o = audio_sample(c, st, ch, src[f * c.channels + ch], hiss ? hiss[f * c.channels + ch] : 0, pulses);
            if (dst) dst[f * c.channels + ch] = o;
        }
        st.count++;
    }
}

// Run, verify, repair: what k_audio_segments and k_audio_verify_repair do, in their order.  dst must not overlap src.
// which (may be NULL): receives the segments that were repaired, in order.
inline void audio_run_planned(const AudioCfg &c, AudioState &st, const int16_t *src, int16_t *dst, const int32_t *hiss, uint64_t total, uint32_t L,
                              uint32_t W, AudioPlanStats *stats, std::vector<uint64_t> *which = nullptr)
{
    if (which) which->clear();
    if (stats) stats->segments = stats->repaired = stats->worst_convergence = 0;
    if (!c.enabled) {
        std::memcpy(dst, src, (size_t)total * (size_t)c.channels * sizeof(int16_t));
        return;
    }
    if (L == 0) L = 1;
    const uint64_t nseg = audio_seg_count(total, L);
    std::vector<AudioState> at_start((size_t)nseg), at_end((size_t)nseg);
    for (uint64_t j = 0; j < nseg; j++) {                                       // the speculative pass
        const AudioSeg g = audio_seg(total, L, W, j);
        AudioState s = g.run_start == 0 ? st : audio_spec_state(c, st, g.run_start);
        audio_run_span(c, s, src, nullptr, hiss, g.run_start, g.start - g.run_start);
        at_start[(size_t)j] = s;
        audio_run_span(c, s, src, dst, hiss, g.start, g.len);
        at_end[(size_t)j] = s;
    }
    AudioState truth = st;
    for (uint64_t j = 0; j < nseg; j++) {                                       // verify, repair
        const AudioSeg g = audio_seg(total, L, W, j);
        if (!audio_state_same(at_start[(size_t)j], truth)) {
            audio_run_span(c, truth, src, dst, hiss, g.start, g.len);
            if (stats) stats->repaired++;
            if (which) which->push_back(j);
        } else {
            truth = at_end[(size_t)j];
        }
    }
    st = truth;
    if (stats) stats->segments = nseg;
}

// ------------------------------------------------------------------------------------------------ many tracks
// A tracks call (ntscsim_audio_tracks_device) puts independent streams side by side: each track is planned on its own,
// exactly as a call of its frames alone would be, and the segments of all tracks are numbered through -- track 0's, then
// track 1's ... -- so that one launch runs them.  A warm-up clamps at frame 0 of ITS track and starts there from that
// track's carried state.

struct AudioTrackEnt {
    uint64_t frames;                     // of the track
    uint64_t plane;                      // its first frame in the PLANE: the frames of all tracks numbered through, which the
                                         // call's hiss (times channels) and pulse scratch and the blocks' `first` are indexed by
    uint64_t seg0;                       // its first segment in the call-wide numbering (= the segments of the tracks before it)
    AudioState *state;                   // carried state: read at the start, written at the end; NULL: zeros, count 0, end discarded
    int32_t block0, nblocks;             // its blocks in the call's block array (a block's `first` counts in the plane)
    // a mixed call only (audio_mixed_layout)
    uint64_t hiss0;                      // its first channel-sample in the hiss plane: tracks differ in channels, so frames * channels
                                         // does not find it; tracks that draw nothing take no room there
    int32_t set;                         // its AudioCfg in the call's set table
    uint32_t warmup;                     // its own warm-up, in frames
};

// fills plane and seg0 of tab[0..n) from the frames; returns the segments of the call
inline uint64_t audio_tracks_layout(AudioTrackEnt *tab, int n, uint32_t L)
{
    uint64_t plane = 0, seg = 0;
    for (int t = 0; t < n; t++) {
        tab[t].plane = plane;
        tab[t].seg0 = seg;
        plane += tab[t].frames;
        seg += audio_seg_count(tab[t].frames, L);
    }
    return seg;
}

// The track of call-wide segment j (j < the call's segments): the LAST t with tab[t].seg0 <= j.  Tracks without frames
// share their seg0 with the track behind them, so the last one is the one that owns j.  j - tab[t].seg0 is the segment
// within the track.
AUDIO_HD int audio_track_of(const AudioTrackEnt *tab, int n, uint64_t j)
{
    int lo = 0, hi = n;                                                         // tab[lo].seg0 <= j < tab[hi].seg0 (tab[n]: the call's segments)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (tab[mid].seg0 <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

inline AudioState audio_track_carried(const AudioTrackEnt &e)
{
    if (e.state) return *e.state;
    AudioState z;
    for (int i = 0; i < AUDIO_STATE_VALUES; i++) z.v[i] = 0;
    z.count = 0;
    return z;
}

struct AudioTrackIO {                    // host: one track of audio_run_tracks_planned()
    const int16_t *src;
    int16_t *dst;                        // must not overlap any src
    const int32_t *hiss;                 // numerators of the track (NULL: no hiss)
    uint64_t frames;
    AudioState *state;                   // as AudioTrackEnt's
};

// Run, verify, repair over a set of tracks: what k_audio_track_segments (every call-wide segment, found through
// audio_track_of) and k_audio_track_verify (each track's records walked from its own true state) do.  stats[t]: of track t.
inline void audio_run_tracks_planned(const AudioCfg &c, const AudioTrackIO *tracks, int n, uint32_t L, uint32_t W, AudioPlanStats *stats)
{
    for (int t = 0; t < n; t++) stats[t].segments = stats[t].repaired = stats[t].worst_convergence = 0;
    if (!c.enabled) {
        for (int t = 0; t < n; t++) std::memcpy(tracks[t].dst, tracks[t].src, (size_t)tracks[t].frames * (size_t)c.channels * sizeof(int16_t));
        return;
    }
    if (L == 0) L = 1;
    std::vector<AudioTrackEnt> tab((size_t)n);
    for (int t = 0; t < n; t++) {
        tab[(size_t)t].frames = tracks[t].frames;
        tab[(size_t)t].state = tracks[t].state;
        tab[(size_t)t].block0 = t;                                              // the host has one block per track
        tab[(size_t)t].nblocks = 1;
    }
    const uint64_t nseg = audio_tracks_layout(tab.data(), n, L);
    std::vector<AudioState> at_start((size_t)nseg), at_end((size_t)nseg);
    for (uint64_t j = 0; j < nseg; j++) {                                       // the speculative pass
        const int t = audio_track_of(tab.data(), n, j);
        const AudioTrackEnt &e = tab[(size_t)t];
        const AudioSeg g = audio_seg(e.frames, L, W, j - e.seg0);
        const AudioState carried = audio_track_carried(e);
        AudioState s = g.run_start == 0 ? carried : audio_spec_state(c, carried, g.run_start);
        audio_run_span(c, s, tracks[t].src, nullptr, tracks[t].hiss, g.run_start, g.start - g.run_start);
        at_start[(size_t)j] = s;
        audio_run_span(c, s, tracks[t].src, tracks[t].dst, tracks[t].hiss, g.start, g.len);
        at_end[(size_t)j] = s;
    }
    for (int t = 0; t < n; t++) {                                               // verify, repair: per track
        const AudioTrackEnt &e = tab[(size_t)t];
        const uint64_t nt = audio_seg_count(e.frames, L);
        AudioState truth = audio_track_carried(e);
        for (uint64_t j = 0; j < nt; j++) {
            const AudioSeg g = audio_seg(e.frames, L, W, j);
            if (!audio_state_same(at_start[(size_t)(e.seg0 + j)], truth)) {
                audio_run_span(c, truth, tracks[t].src, tracks[t].dst, tracks[t].hiss, g.start, g.len);
                stats[t].repaired++;
            } else {
                truth = at_end[(size_t)(e.seg0 + j)];
            }
        }
        if (e.state) *e.state = truth;
        stats[t].segments = nt;
    }
}

// ------------------------------------------------------------------------------------------------ mixed tracks
// A mixed call (ntscsim_audio_mixed_tracks_device) is a tracks call whose tracks each name an AudioCfg of a set table:
// frame size, hiss, buzz and warm-up are the track's own.  A track whose cfg is not enabled is a copy: it has no frames
// in the table (no segments, its state stays) and its blocks set no rand() position.

// does a block of a track with this cfg advance the rand() position (and take room in the hiss plane)?
AUDIO_HD bool audio_track_draws(const AudioCfg &c) { return c.enabled && c.hiss_level != 0; }

// Fills plane, seg0, hiss0 and warmup of tab[0..n) from frames and set; returns the segments of the call.  plan_warmup:
// one warm-up for every track (the debug plan), or NULL: each track's audio_default_warmup().  hiss_items, plane_frames
// (may be NULL): what the hiss plane and the pulse plane must hold.
inline uint64_t audio_mixed_layout(AudioTrackEnt *tab, int n, const AudioCfg *cfgs, uint32_t L, const uint32_t *plan_warmup, uint64_t *hiss_items,
                                   uint64_t *plane_frames)
{
    uint64_t plane = 0, seg = 0, hiss = 0;
    for (int t = 0; t < n; t++) {
        const AudioCfg &c = cfgs[tab[t].set];
        tab[t].plane = plane;
        tab[t].seg0 = seg;
        tab[t].hiss0 = hiss;
        tab[t].warmup = plan_warmup ? *plan_warmup : audio_default_warmup(c);
        plane += tab[t].frames;
        seg += audio_seg_count(tab[t].frames, L);
        if (audio_track_draws(c)) hiss += tab[t].frames * (uint64_t)c.channels;
    }
    if (hiss_items) *hiss_items = hiss;
    if (plane_frames) *plane_frames = plane;
    return seg;
}

struct AudioMixedTrackIO {               // host: one track of audio_run_mixed_tracks_planned()
    const int16_t *src;
    int16_t *dst;                        // must not overlap any src
    uint64_t frames;                     // of channels(cfgs[set]) samples
    AudioState *state;                   // as AudioTrackEnt's
    int set;
};

// Run, verify, repair over tracks with a cfg each: what k_audio_mixed_segments and k_audio_mixed_verify do.  hiss: the
// hiss plane of the call, laid out by audio_mixed_layout() (NULL: no track draws).  stats[t]: of track t.
inline void audio_run_mixed_tracks_planned(const AudioCfg *cfgs, const AudioMixedTrackIO *tracks, int n, const int32_t *hiss, uint32_t L,
                                           const uint32_t *plan_warmup, AudioPlanStats *stats)
{
    if (L == 0) L = 1;
    std::vector<AudioTrackEnt> tab((size_t)n);
    for (int t = 0; t < n; t++) {
        stats[t].segments = stats[t].repaired = stats[t].worst_convergence = 0;
        const AudioCfg &c = cfgs[tracks[t].set];
        AudioTrackEnt &e = tab[(size_t)t];
        std::memset(&e, 0, sizeof(e));
        e.set = tracks[t].set;
        e.state = tracks[t].state;
        e.block0 = t;
        e.nblocks = 1;
        if (c.enabled) e.frames = tracks[t].frames;
        else if (tracks[t].frames) std::memmove(tracks[t].dst, tracks[t].src, (size_t)tracks[t].frames * (size_t)c.channels * sizeof(int16_t));
    }
    const uint64_t nseg = audio_mixed_layout(tab.data(), n, cfgs, L, plan_warmup, nullptr, nullptr);
    const auto hiss_of = [&](const AudioTrackEnt &e) { return audio_track_draws(cfgs[e.set]) ? hiss + e.hiss0 : nullptr; };
    std::vector<AudioState> at_start((size_t)nseg), at_end((size_t)nseg);
    for (uint64_t j = 0; j < nseg; j++) {                                       // the speculative pass
        const int t = audio_track_of(tab.data(), n, j);
        const AudioTrackEnt &e = tab[(size_t)t];
        const AudioCfg &c = cfgs[e.set];
        const AudioSeg g = audio_seg(e.frames, L, e.warmup, j - e.seg0);
        const AudioState carried = audio_track_carried(e);
        AudioState s = g.run_start == 0 ? carried : audio_spec_state(c, carried, g.run_start);
        audio_run_span(c, s, tracks[t].src, nullptr, hiss_of(e), g.run_start, g.start - g.run_start);
        at_start[(size_t)j] = s;
        audio_run_span(c, s, tracks[t].src, tracks[t].dst, hiss_of(e), g.start, g.len);
        at_end[(size_t)j] = s;
    }
    for (int t = 0; t < n; t++) {                                               // verify, repair: per track
        const AudioTrackEnt &e = tab[(size_t)t];
        const AudioCfg &c = cfgs[e.set];
        const uint64_t nt = audio_seg_count(e.frames, L);
        AudioState truth = audio_track_carried(e);
        for (uint64_t j = 0; j < nt; j++) {
            const AudioSeg g = audio_seg(e.frames, L, e.warmup, j);
            if (!audio_state_same(at_start[(size_t)(e.seg0 + j)], truth)) {
                audio_run_span(c, truth, tracks[t].src, tracks[t].dst, hiss_of(e), g.start, g.len);
                stats[t].repaired++;
            } else {
                truth = at_end[(size_t)(e.seg0 + j)];
            }
        }
        if (e.state && nt) *e.state = truth;
        stats[t].segments = nt;
    }
}

} // namespace ntscsim
