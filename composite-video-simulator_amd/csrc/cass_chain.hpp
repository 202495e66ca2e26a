// cass_chain.hpp -- ffmpeg_cassette's tape chain, composite_audio_process() (ffmpeg_cassette.cpp:334-416 with the
// filters of :80-209, the ConvolutionMap of :278-324 and the set-up :864-880), stated once for the kernels
// (csrc/ntsc_cass.hip), the host checker (tests/cass_chain_check.cpp) and the command line host's fallback
// (host/cassette_cli.cpp).  No HIP in it.  Built with -ffp-contract=off: every product and sum is rounded on its own, in
// the reference's order.  The poles, the hiss numerator, the pack and the segment plan are audio_chain.hpp's.
//
// The tool's loop body is FRONT (band-pass, pre-emphasis, clip, hiss) -> a per-sample FIR whose taps follow the head
// tilt -> BACK (de-emphasis, pack, mono downmix).  The pre-emphasis states are touched by the front alone, the
// de-emphasis states by the back alone and the FIR has a delay line per channel, so running the three as passes over a
// call's frames computes what the interleaved loop computes, draw for draw.  DESIGN.md 7m.
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>

#include "audio_chain.hpp"

namespace ntscsim {

constexpr int CASS_MAX_TAPS = 512;       // enough for |headalign| <= 100: floor(200 + 300 + 7.5) = 507
constexpr int CASS_HIST = CASS_MAX_TAPS - 1;
constexpr int CASS_FRONT_VALUES = 26;    // 2 * 12 band-pass, 2 pre
constexpr int CASS_CHANNELS = 2;         // output_audio_channels: the tool never changes it

struct CassCfg {
    int pre, post, mono;                 // emulating_preemphasis / emulating_deemphasis / mono_downmix
    int hiss_level;                      // output_audio_hiss_level :582
    int taps;                            // audio_conv[].length :338
    double rate;                         // output_audio_rate
    double highpass_hz;                  // the slowest pole: sets the front's default warm-up
    double tilt, waver;                  // head_tilt, head_tilt_waver
    double a_lo, a_hi, a_pre, a_post;
};

// v[c*12 + i]: low-pass i of channel c, v[c*12 + 6 + i]: its high-pass; v[24 + i]: pre-emphasis filter i (shared by the
// channels).  count: audio_proc_count
struct CassFront {
    double v[CASS_FRONT_VALUES];
    uint64_t count;
};
struct CassBack {
    double post[2];                      // de-emphasis filter i (shared by the channels)
};
// hist[k][c]: x of frame (next frame - (taps - 1) + k), k < taps - 1: the delay line of ConvolutionMap::calc, oldest
// first; the entries from taps - 1 on are not read and stay as they are
struct CassState {
    CassFront front;
    CassBack back;
    uint32_t taps, _pad;
    double hist[CASS_HIST][CASS_CHANNELS];
};

// :338 -- (int)floor(fabs(tilt * 2) + fabs(tilt * 3) + 7.5)
inline int cass_taps(double tilt) { return (int)std::floor(std::fabs(tilt * 2) + std::fabs(tilt * 3) + 7.5); }

// :344-345 -- the argument of the frame's sin(), in the tool's order of operations, and head_tilt_final from its result.
// sin() itself is libm's, called by the host: cass_fill_tilt().  Nothing else here evaluates it.
inline double cass_sin_arg(const CassCfg &c, uint64_t count)
{
    const double t = (double)count / c.rate;
    return t * 3.14159265358979323846 * 2 * 1.5;
}
AUDIO_HD double cass_tilt_of_sin(const CassCfg &c, double s) { return (c.waver * s) + c.tilt; }
inline void cass_fill_tilt(const CassCfg &c, uint64_t count0, uint64_t n, double *tf)
{
    for (uint64_t i = 0; i < n; i++) tf[i] = cass_tilt_of_sin(c, std::sin(cass_sin_arg(c, count0 + i)));
}

// ------------------------------------------------------------------------------------------------ front
// :376-396 of one channel-sample; hiss: the numerator of its draw (read only when hiss_level != 0)
AUDIO_HD double cass_front_sample(const CassCfg &c, CassFront &st, int ch, int16_t in, int hiss)
{
    double s = (double)in / 32768;
    double *bp = st.v + ch * 12;
    for (int i = 0; i < AUDIO_PASSES; i++) s = audio_pole(bp[i], s, c.a_lo);
    for (int i = 0; i < AUDIO_PASSES; i++) s = s - audio_pole(bp[6 + i], s, c.a_hi);
    if (c.pre)
        for (int i = 0; i < CASS_CHANNELS; i++) s = s + (s - audio_pole(st.v[24 + i], s, c.a_pre));
    if (s > 1.0) s = 1.0;
    else if (s < -1.0) s = -1.0;
    if (c.hiss_level != 0) s += ((double)hiss) / 20000;
    return s;
}

// ------------------------------------------------------------------------------------------------ taps, FIR
// :349-357 / :361-369 -- tap i of channel ch at head_tilt_final tf.  Both divisions stay divisions.
AUDIO_HD double cass_tap(int taps, double tf, int ch, int i)
{
    const double lr = tf * 1.5;
    const double inv = fabs(tf) + 1.0;
    const double mid = (ch ? -lr : lr) + ((double)taps / 2);
    double d = ((double)i - mid) / inv;
    d = 1.0 - fabs(d);
    if (d < 0) d = 0;
    d /= inv;
    return d;
}

// The taps that can be other than zero lie in [lo, hi): |i - mid| >= inv + 1 gives |(i - mid) / inv| >= 1 + 1 / inv,
// which no rounding of the subtraction and the division brings down to 1, so d < 0 there and the tap is +0.  The
// bounds leave that whole frame of slack and are clamped in double before the conversion.
AUDIO_HD void cass_tap_range(int taps, double tf, int ch, int &lo, int &hi)
{
    const double lr = tf * 1.5;
    const double inv = fabs(tf) + 1.0;
    const double mid = (ch ? -lr : lr) + ((double)taps / 2);
    double a = mid - inv - 2.0, b = mid + inv + 3.0;
    if (!(a > 0)) a = 0;
    if (!(b < (double)taps)) b = (double)taps;
    if (!(a < (double)taps)) a = (double)taps;
    if (!(b > 0)) b = 0;
    lo = (int)a;
    hi = (int)b;
    if (hi < lo) hi = lo;
}

// ConvolutionMap::calc :308-319 for the frame whose own x is w[(taps - 1) * stride]: w[i * stride] is map[i], oldest
// first.  Skip: products with a tap of +0 are left out.  That changes no bit: r starts at +0, a tap is never negative, x
// is finite (the clip, then a hiss term of at most 0.5), so a skipped product is +0 or -0; +0 + (+-0) = +0, and a sum
// of finite doubles is -0 only if both terms are, which r never is -- so r is the same double with and without them.
// The checker runs Skip = false, every tap; the kernels run Skip = true and are tested against it.
template <bool Skip>
AUDIO_HD double cass_conv(int taps, double tf, int ch, const double *w, int stride)
{
    double r = 0;
    int lo = 0, hi = taps;
    if (Skip) cass_tap_range(taps, tf, ch, lo, hi);
    for (int i = lo; i < hi; i++) {
        const double d = cass_tap(taps, tf, ch, i);
        if (Skip && d == 0) continue;
        r += w[i * stride] * d;
    }
    return r;
}

// ------------------------------------------------------------------------------------------------ back
// :402-408 of one channel-sample
AUDIO_HD int16_t cass_back_sample(const CassCfg &c, CassBack &st, double r)
{
    if (c.post)
        for (int i = 0; i < CASS_CHANNELS; i++) r = audio_pole(st.post[i], r, c.a_post);
    return audio_pack(r);
}
// :411-412 -- the int division truncates toward zero
AUDIO_HD void cass_downmix(const CassCfg &c, int16_t &o0, int16_t &o1)
{
    if (c.mono) o0 = o1 = (int16_t)(((int)o0 + (int)o1) / 2);
}

// ------------------------------------------------------------------------------------------------ serial
// Frames [first, first + n) of the call through the front, from state st.  xs (NULL: states only): the call's plane of
// x behind its taps - 1 frames of history, xs[(taps - 1 + f) * 2 + c].  hiss: numerators of the whole call (NULL: none)
inline void cass_front_span(const CassCfg &c, CassFront &st, const int16_t *src, double *xs, const int32_t *hiss, uint64_t first, uint64_t n)
{
    for (uint64_t f = first; f < first + n; f++) {
        for (int ch = 0; ch < CASS_CHANNELS; ch++) {
            const double x = cass_front_sample(c, st, ch, src[f * 2 + ch], hiss ? hiss[f * 2 + ch] : 0);
            if (xs) xs[((uint64_t)(c.taps - 1) + f) * 2 + ch] = x;
        }
        st.count++;
    }
}

// the FIR of frames [first, first + n): rs[f * 2 + c]
template <bool Skip>
inline void cass_conv_span(const CassCfg &c, const double *xs, const double *tf, double *rs, uint64_t first, uint64_t n)
{
    for (uint64_t f = first; f < first + n; f++)
        for (int ch = 0; ch < CASS_CHANNELS; ch++) rs[f * 2 + ch] = cass_conv<Skip>(c.taps, tf[f], ch, xs + f * 2 + ch, 2);
}

// frames [first, first + n) through the back, from state st; dst NULL: states only
inline void cass_back_span(const CassCfg &c, CassBack &st, const double *rs, int16_t *dst, uint64_t first, uint64_t n)
{
    for (uint64_t f = first; f < first + n; f++) {
        int16_t o0 = cass_back_sample(c, st, rs[f * 2]);
        int16_t o1 = cass_back_sample(c, st, rs[f * 2 + 1]);
        cass_downmix(c, o0, o1);
        if (dst) { dst[f * 2] = o0; dst[f * 2 + 1] = o1; }
    }
}

// the plane of x of a call: the carried history in front, room for `total` frames behind it
inline void cass_plane_begin(const CassCfg &c, const CassState &st, std::vector<double> &xs, uint64_t total)
{
    const size_t h = (size_t)(c.taps - 1);
    xs.assign((h + (size_t)total) * 2, 0.0);
    for (size_t k = 0; k < h; k++)
        for (int ch = 0; ch < CASS_CHANNELS; ch++) xs[k * 2 + ch] = st.hist[k][ch];
}
// the call's last taps - 1 values of x become the history (a call shorter than that keeps part of the old one)
inline void cass_plane_end(const CassCfg &c, CassState &st, const std::vector<double> &xs, uint64_t total)
{
    const size_t h = (size_t)(c.taps - 1);
    for (size_t k = 0; k < h; k++)
        for (int ch = 0; ch < CASS_CHANNELS; ch++) st.hist[k][ch] = xs[((size_t)total + k) * 2 + ch];
}

// composite_audio_process(audio, frames) from src to dst (dst may be src).  tf: head_tilt_final of each frame
// (cass_fill_tilt(c, st.front.count, frames, tf), or built from recorded sines).  draw(): the next rand(), called once
// per channel-sample when hiss_level != 0, in the tool's order.  Every tap is run.
template <class Draw>
inline void cass_run_serial(const CassCfg &c, CassState &st, const int16_t *src, int16_t *dst, uint64_t frames, const double *tf, Draw &&draw)
{
    std::vector<double> xs, rs((size_t)frames * 2);
    std::vector<int32_t> hiss;
    if (c.hiss_level != 0) {
        hiss.resize((size_t)frames * 2);
        for (int32_t &h : hiss) h = audio_hiss_num(draw(), c.hiss_level);
    }
    cass_plane_begin(c, st, xs, frames);
    cass_front_span(c, st.front, src, xs.data(), hiss.empty() ? nullptr : hiss.data(), 0, frames);
    cass_conv_span<false>(c, xs.data(), tf, rs.data(), 0, frames);
    cass_back_span(c, st.back, rs.data(), dst, 0, frames);
    cass_plane_end(c, st, xs, frames);
}

// ------------------------------------------------------------------------------------------------ the plan
// The front and the back are cut into the segments of audio_chain.hpp (audio_seg()), each pass with a warm-up of its
// own; a segment writes x (the back: the samples) of its own frames only, so the FIR between them reads nothing
// speculative once the front is verified and its history is no part of the speculation.

// the front's default warm-up is the audio chain's: 72 tau of the high-pass
inline uint32_t cass_default_front_warmup(const CassCfg &c)
{
    AudioCfg a;
    std::memset(&a, 0, sizeof(a));
    a.rate = c.rate;
    a.highpass_hz = c.highpass_hz;
    return audio_default_warmup(a);
}
// The back's: two poles at 4000 Hz.  Measured on the fixture's inputs (tests/test_cass_chain_host.py): a
// zero-state run meets the true states bit for bit after 52 frames at the most; a fifth on top, up to a multiple of 64
constexpr uint32_t CASS_BACK_MEASURED = 52;
constexpr uint32_t CASS_DEFAULT_BACK_WARMUP = ((CASS_BACK_MEASURED + CASS_BACK_MEASURED / 5 + 1) + 63) / 64 * 64;

AUDIO_HD CassFront cass_front_spec(const CassCfg &c, const CassFront &carried, uint64_t run_start)
{
    CassFront s = carried;
    for (int i = 0; i < CASS_FRONT_VALUES; i++)
        if (i < 24 || c.pre) s.v[i] = 0;
    s.count = carried.count + run_start;
    return s;
}
AUDIO_HD bool cass_bits_same(const double *a, const double *b, int n)
{
    for (int i = 0; i < n; i++) {
        uint64_t x, y;
        memcpy(&x, &a[i], 8);
        memcpy(&y, &b[i], 8);
        if (x != y) return false;
    }
    return true;
}
AUDIO_HD bool cass_front_same(const CassFront &a, const CassFront &b) { return a.count == b.count && cass_bits_same(a.v, b.v, CASS_FRONT_VALUES); }
AUDIO_HD bool cass_back_same(const CassBack &a, const CassBack &b) { return cass_bits_same(a.post, b.post, 2); }

struct CassPlanStats {
    uint64_t segments, repaired_front, repaired_back;
};

// Run, verify, repair: what k_cass_front, k_cass_front_verify, k_cass_conv, k_cass_back and k_cass_back_verify do, in
// their order and with the kernels' skipping FIR.  dst must not overlap src.  which_front / which_back (may be NULL):
// receive the segments that each pass repaired, in order.
inline void cass_run_planned(const CassCfg &c, CassState &st, const int16_t *src, int16_t *dst, const int32_t *hiss, const double *tf, uint64_t total,
                             uint32_t L, uint32_t Wf, uint32_t Wb, CassPlanStats *stats, std::vector<uint64_t> *which_front = nullptr,
                             std::vector<uint64_t> *which_back = nullptr)
{
    if (which_front) which_front->clear();
    if (which_back) which_back->clear();
    if (stats) stats->segments = stats->repaired_front = stats->repaired_back = 0;
    if (L == 0) L = 1;
    const uint64_t nseg = audio_seg_count(total, L);
    std::vector<double> xs, rs((size_t)total * 2);
    cass_plane_begin(c, st, xs, total);
    {
        std::vector<CassFront> at_start((size_t)nseg), at_end((size_t)nseg);
        for (uint64_t j = 0; j < nseg; j++) {                                   // the speculative pass
            const AudioSeg g = audio_seg(total, L, Wf, j);
            CassFront s = g.run_start == 0 ? st.front : cass_front_spec(c, st.front, g.run_start);
            cass_front_span(c, s, src, nullptr, hiss, g.run_start, g.start - g.run_start);
            at_start[(size_t)j] = s;
            cass_front_span(c, s, src, xs.data(), hiss, g.start, g.len);
            at_end[(size_t)j] = s;
        }
        CassFront truth = st.front;
        for (uint64_t j = 0; j < nseg; j++) {                                   // verify, repair
            const AudioSeg g = audio_seg(total, L, Wf, j);
            if (!cass_front_same(at_start[(size_t)j], truth)) {
                cass_front_span(c, truth, src, xs.data(), hiss, g.start, g.len);
                if (stats) stats->repaired_front++;
                if (which_front) which_front->push_back(j);
            } else {
                truth = at_end[(size_t)j];
            }
        }
        st.front = truth;
    }
    cass_conv_span<true>(c, xs.data(), tf, rs.data(), 0, total);
    if (!c.post) {
        cass_back_span(c, st.back, rs.data(), dst, 0, total);                   // no state: nothing to speculate on
    } else {
        std::vector<CassBack> at_start((size_t)nseg), at_end((size_t)nseg);
        for (uint64_t j = 0; j < nseg; j++) {
            const AudioSeg g = audio_seg(total, L, Wb, j);
            CassBack s = st.back;
            if (g.run_start != 0) s.post[0] = s.post[1] = 0;
            cass_back_span(c, s, rs.data(), nullptr, g.run_start, g.start - g.run_start);
            at_start[(size_t)j] = s;
            cass_back_span(c, s, rs.data(), dst, g.start, g.len);
            at_end[(size_t)j] = s;
        }
        CassBack truth = st.back;
        for (uint64_t j = 0; j < nseg; j++) {
            const AudioSeg g = audio_seg(total, L, Wb, j);
            if (!cass_back_same(at_start[(size_t)j], truth)) {
                cass_back_span(c, truth, rs.data(), dst, g.start, g.len);
                if (stats) stats->repaired_back++;
                if (which_back) which_back->push_back(j);
            } else {
                truth = at_end[(size_t)j];
            }
        }
        st.back = truth;
    }
    cass_plane_end(c, st, xs, total);
    if (stats) stats->segments = nseg;
}

// ------------------------------------------------------------------------------------------------ many tracks
// A tracks call (ntscsim_cass_tracks_device) puts independent streams side by side, as audio_chain.hpp's does: each track
// is planned on its own, exactly as a call of its frames alone would be, and the segments of all tracks -- and the FIR's
// tiles -- are numbered through, so that one launch of each kernel runs them.  What the cassette adds: a delay line per
// track (every track has a section of the x plane of its own: its taps - 1 history frames, then its frames), tiles that
// never cross a track, and one table of head_tilt_final over the UNION of the tracks' sample counts.

constexpr uint32_t CASS_TILE_FRAMES = 256;   // frames of a tile of the FIR (a workgroup of k_cass_conv / k_cass_track_conv)

struct CassTrackEnt {
    uint64_t frames;                     // of the track
    uint64_t plane;                      // its first frame in the PLANE: the frames of all tracks numbered through, which the
                                         // call's hiss and r scratch and the blocks' `first` are indexed by
    uint64_t seg0;                       // its first segment in the call-wide numbering
    uint64_t tile0;                      // its first FIR tile in the call-wide numbering
    uint64_t xs;                         // frame offset of its section of the x plane: taps - 1 history frames, then its frames
    uint64_t tilt;                       // offset of its first frame in the call's tilt table
    uint64_t count;                      // audio_proc_count of its first frame: the HOST's, never read from the state
    CassState *state;                    // carried state: read at the start, written at the end; NULL: zeros, end discarded
    int32_t block0, nblocks;             // its blocks in the call's block array (a block's `first` counts in the plane)
};

struct CassTracksTotals {
    uint64_t frames, segments, tiles, xs_frames;   // of the call; xs_frames: the x plane, histories included
};

// fills plane, seg0, tile0 and xs of tab[0..n) from the frames.  Every track has a section of the x plane, one without
// frames too (its history alone: nothing reads it).
inline CassTracksTotals cass_tracks_layout(CassTrackEnt *tab, int n, uint32_t L, int taps)
{
    CassTracksTotals z{0, 0, 0, 0};
    for (int t = 0; t < n; t++) {
        tab[t].plane = z.frames;
        tab[t].seg0 = z.segments;
        tab[t].tile0 = z.tiles;
        tab[t].xs = z.xs_frames;
        z.frames += tab[t].frames;
        z.segments += audio_seg_count(tab[t].frames, L);
        z.tiles += audio_seg_count(tab[t].frames, CASS_TILE_FRAMES);
        z.xs_frames += (uint64_t)(taps - 1) + tab[t].frames;
    }
    return z;
}

// The track of call-wide segment j / of call-wide tile i (below the call's totals): the LAST t whose seg0 / tile0 is not
// above it, as audio_track_of().  Tracks without frames share their index with the track behind them, so the last one is
// the one that owns it.
AUDIO_HD int cass_track_of_seg(const CassTrackEnt *tab, int n, uint64_t j)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (tab[mid].seg0 <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}
AUDIO_HD int cass_track_of_tile(const CassTrackEnt *tab, int n, uint64_t i)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (tab[mid].tile0 <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The tilt table holds head_tilt_final of every sample count that some track covers, once: the tracks' ranges
// [count, count + frames) merged into disjoint runs in ascending order, the runs back to back in the table.
struct CassTiltRun {
    uint64_t count0, n, at;              // counts [count0, count0 + n) stand at table entries [at, at + n)
};

// Fills tab[t].tilt (0 for a track without frames) and the runs; *total: entries of the table = sines to evaluate.
// false: count + frames of a track overflows 64 bits (nothing is filled in then).
inline bool cass_tilt_layout(CassTrackEnt *tab, int n, std::vector<CassTiltRun> &runs, uint64_t *total)
{
    runs.clear();
    *total = 0;
    std::vector<std::pair<uint64_t, int>> order;                                // (count, track) of the tracks that have frames
    for (int t = 0; t < n; t++) {
        if (tab[t].count + tab[t].frames < tab[t].count) return false;
        if (tab[t].frames) order.push_back({tab[t].count, t});
    }
    std::sort(order.begin(), order.end());
    for (const std::pair<uint64_t, int> &o : order) {
        const int t = o.second;
        const uint64_t a = tab[t].count, b = a + tab[t].frames;
        if (runs.empty() || a > runs.back().count0 + runs.back().n) runs.push_back(CassTiltRun{a, b - a, *total});
        else if (b > runs.back().count0 + runs.back().n) runs.back().n = b - runs.back().count0;
        *total = runs.back().at + runs.back().n;
        tab[t].tilt = runs.back().at + (a - runs.back().count0);
    }
    for (int t = 0; t < n; t++)
        if (!tab[t].frames) tab[t].tilt = 0;
    return true;
}

// entries [at, at + n) of the table: what one thread of the fill evaluates
inline void cass_fill_tilt_part(const CassCfg &c, const CassTiltRun *runs, size_t nruns, uint64_t at, uint64_t n, double *tf)
{
    for (size_t r = 0; r < nruns && n; r++) {
        if (runs[r].at + runs[r].n <= at) continue;
        const uint64_t skip = at - runs[r].at, m = runs[r].n - skip < n ? runs[r].n - skip : n;
        cass_fill_tilt(c, runs[r].count0 + skip, m, tf + at);
        at += m;
        n -= m;
    }
}

inline CassState cass_track_carried(const CassTrackEnt &e)
{
    CassState z;
    if (e.state) z = *e.state;
    else std::memset(&z, 0, sizeof(z));
    z.front.count = e.count;                                                    // the state's own count is not read
    return z;
}

struct CassTrackIO {                     // host: one track of cass_run_tracks_planned()
    const int16_t *src;
    int16_t *dst;                        // must not overlap any src
    const int32_t *hiss;                 // numerators of the track (NULL: no hiss)
    uint64_t frames, count;
    CassState *state;                    // as CassTrackEnt's
};

// Run, verify, repair over a set of tracks: what k_cass_track_front (every call-wide segment, found through
// cass_track_of_seg), k_cass_track_front_verify (each track's records walked from its own true state, its history laid
// in front of its section), k_cass_track_conv (every call-wide tile, found through cass_track_of_tile, the tilt through
// the track's table offset; the track's new history), k_cass_track_back and k_cass_track_back_verify do, in their
// order.  stats[t]: of track t.  tilt_frames (may be NULL): the sines evaluated.  false: a count overflows; nothing ran.
inline bool cass_run_tracks_planned(const CassCfg &c, const CassTrackIO *tracks, int n, uint32_t L, uint32_t Wf, uint32_t Wb, CassPlanStats *stats,
                                    uint64_t *tilt_frames = nullptr)
{
    for (int t = 0; t < n; t++) stats[t].segments = stats[t].repaired_front = stats[t].repaired_back = 0;
    if (L == 0) L = 1;
    const uint64_t h = (uint64_t)(c.taps - 1);
    std::vector<CassTrackEnt> tab((size_t)n);
    for (int t = 0; t < n; t++) {
        std::memset(&tab[(size_t)t], 0, sizeof(CassTrackEnt));
        tab[(size_t)t].frames = tracks[t].frames;
        tab[(size_t)t].count = tracks[t].count;
        tab[(size_t)t].state = tracks[t].state;
        tab[(size_t)t].block0 = t;                                              // the host has one block per track
        tab[(size_t)t].nblocks = 1;
    }
    std::vector<CassTiltRun> runs;
    uint64_t tilt_total = 0;
    if (!cass_tilt_layout(tab.data(), n, runs, &tilt_total)) return false;
    if (tilt_frames) *tilt_frames = tilt_total;
    const CassTracksTotals z = cass_tracks_layout(tab.data(), n, L, c.taps);
    std::vector<double> tf((size_t)tilt_total + 1), xs((size_t)z.xs_frames * 2 + 2, 0.0), rs((size_t)z.frames * 2 + 2);
    cass_fill_tilt_part(c, runs.data(), runs.size(), 0, tilt_total, tf.data());
    {
        std::vector<CassFront> at_start((size_t)z.segments), at_end((size_t)z.segments);
        for (uint64_t j = 0; j < z.segments; j++) {                             // the speculative front
            const int t = cass_track_of_seg(tab.data(), n, j);
            const CassTrackEnt &e = tab[(size_t)t];
            const AudioSeg g = audio_seg(e.frames, L, Wf, j - e.seg0);
            const CassFront carried = cass_track_carried(e).front;
            CassFront s = g.run_start == 0 ? carried : cass_front_spec(c, carried, g.run_start);
            cass_front_span(c, s, tracks[t].src, nullptr, tracks[t].hiss, g.run_start, g.start - g.run_start);
            at_start[(size_t)j] = s;
            cass_front_span(c, s, tracks[t].src, xs.data() + e.xs * 2, tracks[t].hiss, g.start, g.len);
            at_end[(size_t)j] = s;
        }
        for (int t = 0; t < n; t++) {                                           // verify, repair: per track
            const CassTrackEnt &e = tab[(size_t)t];
            if (!e.frames) continue;
            const CassState carried = cass_track_carried(e);
            for (uint64_t k = 0; k < h; k++)
                for (int ch = 0; ch < CASS_CHANNELS; ch++) xs[(size_t)(e.xs + k) * 2 + ch] = carried.hist[k][ch];
            const uint64_t nt = audio_seg_count(e.frames, L);
            CassFront truth = carried.front;
            for (uint64_t j = 0; j < nt; j++) {
                const AudioSeg g = audio_seg(e.frames, L, Wf, j);
                if (!cass_front_same(at_start[(size_t)(e.seg0 + j)], truth)) {
                    cass_front_span(c, truth, tracks[t].src, xs.data() + e.xs * 2, tracks[t].hiss, g.start, g.len);
                    stats[t].repaired_front++;
                } else {
                    truth = at_end[(size_t)(e.seg0 + j)];
                }
            }
            if (e.state) e.state->front = truth;                               // count: e.count + e.frames by now
            stats[t].segments = nt;
        }
    }
    for (uint64_t i = 0; i < z.tiles; i++) {                                    // the FIR by tile
        const CassTrackEnt &e = tab[(size_t)cass_track_of_tile(tab.data(), n, i)];
        const uint64_t first = (i - e.tile0) * CASS_TILE_FRAMES, own = e.frames - first < CASS_TILE_FRAMES ? e.frames - first : CASS_TILE_FRAMES;
        cass_conv_span<true>(c, xs.data() + e.xs * 2, tf.data() + e.tilt, rs.data() + e.plane * 2, first, own);
    }
    if (!c.post) {
        for (int t = 0; t < n; t++) {
            CassBack none = cass_track_carried(tab[(size_t)t]).back;
            cass_back_span(c, none, rs.data() + tab[(size_t)t].plane * 2, tracks[t].dst, 0, tab[(size_t)t].frames);
        }
    } else {
        std::vector<CassBack> at_start((size_t)z.segments), at_end((size_t)z.segments);
        for (uint64_t j = 0; j < z.segments; j++) {                             // the speculative back
            const int t = cass_track_of_seg(tab.data(), n, j);
            const CassTrackEnt &e = tab[(size_t)t];
            const AudioSeg g = audio_seg(e.frames, L, Wb, j - e.seg0);
            CassBack s = cass_track_carried(e).back;
            if (g.run_start != 0) s.post[0] = s.post[1] = 0;
            cass_back_span(c, s, rs.data() + e.plane * 2, nullptr, g.run_start, g.start - g.run_start);
            at_start[(size_t)j] = s;
            cass_back_span(c, s, rs.data() + e.plane * 2, tracks[t].dst, g.start, g.len);
            at_end[(size_t)j] = s;
        }
        for (int t = 0; t < n; t++) {
            const CassTrackEnt &e = tab[(size_t)t];
            if (!e.frames) continue;
            const uint64_t nt = audio_seg_count(e.frames, L);
            CassBack truth = cass_track_carried(e).back;
            for (uint64_t j = 0; j < nt; j++) {
                const AudioSeg g = audio_seg(e.frames, L, Wb, j);
                if (!cass_back_same(at_start[(size_t)(e.seg0 + j)], truth)) {
                    cass_back_span(c, truth, rs.data() + e.plane * 2, tracks[t].dst, g.start, g.len);
                    stats[t].repaired_back++;
                } else {
                    truth = at_end[(size_t)(e.seg0 + j)];
                }
            }
            if (e.state) e.state->back = truth;
        }
    }
    for (int t = 0; t < n; t++) {                                               // the history, the count, the taps
        const CassTrackEnt &e = tab[(size_t)t];
        if (!e.frames || !e.state) continue;
        for (uint64_t k = 0; k < h; k++)
            for (int ch = 0; ch < CASS_CHANNELS; ch++) e.state->hist[k][ch] = xs[(size_t)(e.xs + e.frames + k) * 2 + ch];
        e.state->front.count = e.count + e.frames;
        e.state->taps = (uint32_t)c.taps;
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ parameters per track
// A mixed tracks call (ntscsim_cass_mixed_tracks_device) is a tracks call whose tracks each name a CassCfg of a SET
// TABLE: one cfg per distinct set that some track names, in order of first use.  What was the call's and is now the
// track's: the taps (so the size of its section of the x plane, the halo of its tiles and the length of its history),
// the front's warm-up, pre-emphasis, de-emphasis (tracks without it are packed and closed by the FIR; the back skips
// them), mono, the hiss level, tilt and waver.  The segment length and the back's warm-up stay the call's.
// The table that the FIR reads holds the SINES s = sin(cass_sin_arg(count, rate)), not head_tilt_final: s depends on the
// count and the rate alone, so tracks on different tilt and waver share it, and cass_tilt_of_sin() of the track's cfg --
// one product and one sum, rounded one by one -- makes head_tilt_final of it where it is used.

struct CassMixedEnt {
    uint64_t frames, plane, seg0, tile0, xs, tilt, count;   // as CassTrackEnt's; xs counts taps_t - 1 history frames per
                                         // track, tilt is an offset in the table of sines
    CassState *state;
    int32_t block0, nblocks;
    int32_t set;                         // the track's cfg in the set table
    uint32_t warm;                       // the front's warm-up of this track
};

// set_of[t] in -1 .. n_sets - 1 (checked by the caller).  order: the sets of the table, in order of first use;
// cfg_of[t]: track t's place in it.
inline void cass_mixed_set_table(const int32_t *set_of, int n, int n_sets, std::vector<int32_t> &order, std::vector<int32_t> &cfg_of)
{
    std::vector<int32_t> at((size_t)n_sets + 1, -1);                            // at[set + 1]: its place in the table
    order.clear();
    cfg_of.assign((size_t)n, 0);
    for (int t = 0; t < n; t++) {
        int32_t &a = at[(size_t)(set_of[t] + 1)];
        if (a < 0) {
            a = (int32_t)order.size();
            order.push_back(set_of[t]);
        }
        cfg_of[(size_t)t] = a;
    }
}

// fills plane, seg0, tile0, xs and warm of tab[0..n) from frames and set.  warm_all (may be NULL): a debug plan's
// warm-up for every track; otherwise each track has its own cfg's default, as a lone call of its frames would.
inline CassTracksTotals cass_mixed_layout(CassMixedEnt *tab, int n, const CassCfg *cfgs, uint32_t L, const uint32_t *warm_all)
{
    CassTracksTotals z{0, 0, 0, 0};
    for (int t = 0; t < n; t++) {
        const CassCfg &c = cfgs[tab[t].set];
        tab[t].plane = z.frames;
        tab[t].seg0 = z.segments;
        tab[t].tile0 = z.tiles;
        tab[t].xs = z.xs_frames;
        tab[t].warm = warm_all ? *warm_all : cass_default_front_warmup(c);
        z.frames += tab[t].frames;
        z.segments += audio_seg_count(tab[t].frames, L);
        z.tiles += audio_seg_count(tab[t].frames, CASS_TILE_FRAMES);
        z.xs_frames += (uint64_t)(c.taps - 1) + tab[t].frames;
    }
    return z;
}

AUDIO_HD int cass_track_of_seg(const CassMixedEnt *tab, int n, uint64_t j)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (tab[mid].seg0 <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}
AUDIO_HD int cass_track_of_tile(const CassMixedEnt *tab, int n, uint64_t i)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (tab[mid].tile0 <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The table of sines: per distinct rate (in order of first use by a track that has frames) the union of the ranges
// [count, count + frames) of the tracks on that rate, as cass_tilt_layout() makes it; the unions back to back.
struct CassSineRun {
    uint64_t count0, n, at;              // counts [count0, count0 + n) stand at table entries [at, at + n)
    double rate;
};

// Fills tab[t].tilt (0 for a track without frames) and the runs; *total: entries of the table = sines to evaluate.
// false: count + frames of a track overflows 64 bits.
inline bool cass_sine_layout(CassMixedEnt *tab, int n, const CassCfg *cfgs, std::vector<CassSineRun> &runs, uint64_t *total)
{
    runs.clear();
    *total = 0;
    std::vector<double> rates;
    for (int t = 0; t < n; t++) {
        if (tab[t].count + tab[t].frames < tab[t].count) return false;
        const double r = cfgs[tab[t].set].rate;
        if (tab[t].frames && std::find(rates.begin(), rates.end(), r) == rates.end()) rates.push_back(r);
    }
    for (const double rate : rates) {
        std::vector<std::pair<uint64_t, int>> order;
        for (int t = 0; t < n; t++)
            if (tab[t].frames && cfgs[tab[t].set].rate == rate) order.push_back({tab[t].count, t});
        std::sort(order.begin(), order.end());
        const size_t first_run = runs.size();
        for (const std::pair<uint64_t, int> &o : order) {
            const int t = o.second;
            const uint64_t a = tab[t].count, b = a + tab[t].frames;
            if (runs.size() == first_run || a > runs.back().count0 + runs.back().n) runs.push_back(CassSineRun{a, b - a, *total, rate});
            else if (b > runs.back().count0 + runs.back().n) runs.back().n = b - runs.back().count0;
            *total = runs.back().at + runs.back().n;
            tab[t].tilt = runs.back().at + (a - runs.back().count0);
        }
    }
    for (int t = 0; t < n; t++)
        if (!tab[t].frames) tab[t].tilt = 0;
    return true;
}

// entries [at, at + n) of the table of sines: what one thread of the fill evaluates
inline void cass_fill_sines_part(const CassSineRun *runs, size_t nruns, uint64_t at, uint64_t n, double *s)
{
    CassCfg c;
    std::memset(&c, 0, sizeof(c));
    for (size_t r = 0; r < nruns && n; r++) {
        if (runs[r].at + runs[r].n <= at) continue;
        const uint64_t skip = at - runs[r].at, m = runs[r].n - skip < n ? runs[r].n - skip : n;
        c.rate = runs[r].rate;
        for (uint64_t i = 0; i < m; i++) s[at + i] = std::sin(cass_sin_arg(c, runs[r].count0 + skip + i));
        at += m;
        n -= m;
    }
}

struct CassMixedIO {                     // host: one track of cass_run_mixed_tracks_planned()
    CassTrackIO io;
    int32_t set;                         // in the set table
};

// Run, verify, repair over tracks that each have a cfg of the set table: what k_cass_mixed_front,
// k_cass_mixed_front_verify, k_cass_mixed_conv, k_cass_mixed_back and k_cass_mixed_back_verify do, in their order.
// warm_all: as cass_mixed_layout()'s.  stats[t]: of track t.  tilt_frames (may be NULL): the sines evaluated.
// false: a count overflows; nothing ran.
inline bool cass_run_mixed_tracks_planned(const CassCfg *cfgs, const CassMixedIO *tracks, int n, uint32_t L, const uint32_t *warm_all, uint32_t Wb,
                                          CassPlanStats *stats, uint64_t *tilt_frames = nullptr)
{
    for (int t = 0; t < n; t++) stats[t].segments = stats[t].repaired_front = stats[t].repaired_back = 0;
    if (L == 0) L = 1;
    std::vector<CassMixedEnt> tab((size_t)n);
    for (int t = 0; t < n; t++) {
        CassMixedEnt &e = tab[(size_t)t];
        std::memset(&e, 0, sizeof(e));
        e.frames = tracks[t].io.frames;
        e.count = tracks[t].io.count;
        e.state = tracks[t].io.state;
        e.block0 = t;
        e.nblocks = 1;
        e.set = tracks[t].set;
    }
    std::vector<CassSineRun> runs;
    uint64_t sines_total = 0;
    if (!cass_sine_layout(tab.data(), n, cfgs, runs, &sines_total)) return false;
    if (tilt_frames) *tilt_frames = sines_total;
    const CassTracksTotals z = cass_mixed_layout(tab.data(), n, cfgs, L, warm_all);
    std::vector<double> sines((size_t)sines_total + 1), xs((size_t)z.xs_frames * 2 + 2, 0.0), rs((size_t)z.frames * 2 + 2);
    cass_fill_sines_part(runs.data(), runs.size(), 0, sines_total, sines.data());
    const auto carried_of = [](const CassMixedEnt &e) {
        CassTrackEnt u;
        std::memset(&u, 0, sizeof(u));
        u.count = e.count;
        u.state = e.state;
        return cass_track_carried(u);
    };
    {
        std::vector<CassFront> at_start((size_t)z.segments), at_end((size_t)z.segments);
        for (uint64_t j = 0; j < z.segments; j++) {                             // the speculative front
            const int t = cass_track_of_seg(tab.data(), n, j);
            const CassMixedEnt &e = tab[(size_t)t];
            const CassCfg &c = cfgs[e.set];
            const CassTrackIO &io = tracks[t].io;
            const AudioSeg g = audio_seg(e.frames, L, e.warm, j - e.seg0);
            const CassFront carried = carried_of(e).front;
            CassFront s = g.run_start == 0 ? carried : cass_front_spec(c, carried, g.run_start);
            cass_front_span(c, s, io.src, nullptr, io.hiss, g.run_start, g.start - g.run_start);
            at_start[(size_t)j] = s;
            cass_front_span(c, s, io.src, xs.data() + e.xs * 2, io.hiss, g.start, g.len);
            at_end[(size_t)j] = s;
        }
        for (int t = 0; t < n; t++) {                                           // verify, repair: per track
            const CassMixedEnt &e = tab[(size_t)t];
            if (!e.frames) continue;
            const CassCfg &c = cfgs[e.set];
            const CassTrackIO &io = tracks[t].io;
            const CassState carried = carried_of(e);
            for (uint64_t k = 0; k < (uint64_t)(c.taps - 1); k++)
                for (int ch = 0; ch < CASS_CHANNELS; ch++) xs[(size_t)(e.xs + k) * 2 + ch] = carried.hist[k][ch];
            const uint64_t nt = audio_seg_count(e.frames, L);
            CassFront truth = carried.front;
            for (uint64_t j = 0; j < nt; j++) {
                const AudioSeg g = audio_seg(e.frames, L, e.warm, j);
                if (!cass_front_same(at_start[(size_t)(e.seg0 + j)], truth)) {
                    cass_front_span(c, truth, io.src, xs.data() + e.xs * 2, io.hiss, g.start, g.len);
                    stats[t].repaired_front++;
                } else {
                    truth = at_end[(size_t)(e.seg0 + j)];
                }
            }
            if (e.state) e.state->front = truth;
            stats[t].segments = nt;
        }
    }
    bool any_post = false;
    for (uint64_t i = 0; i < z.tiles; i++) {                                    // the FIR by tile; tracks without de-emphasis end here
        const int t = cass_track_of_tile(tab.data(), n, i);
        const CassMixedEnt &e = tab[(size_t)t];
        const CassCfg &c = cfgs[e.set];
        const uint64_t first = (i - e.tile0) * CASS_TILE_FRAMES, own = e.frames - first < CASS_TILE_FRAMES ? e.frames - first : CASS_TILE_FRAMES;
        const double *x = xs.data() + e.xs * 2;
        double *r = rs.data() + e.plane * 2;
        for (uint64_t f = first; f < first + own; f++) {
            const double tf = cass_tilt_of_sin(c, sines[(size_t)(e.tilt + f)]);
            for (int ch = 0; ch < CASS_CHANNELS; ch++) r[f * 2 + ch] = cass_conv<true>(c.taps, tf, ch, x + f * 2 + ch, 2);
        }
        if (c.post) {
            any_post = true;
        } else {
            CassBack none = carried_of(e).back;
            cass_back_span(c, none, r, tracks[t].io.dst, first, own);
        }
    }
    if (any_post) {
        std::vector<CassBack> at_start((size_t)z.segments), at_end((size_t)z.segments);
        for (uint64_t j = 0; j < z.segments; j++) {                             // the speculative back
            const int t = cass_track_of_seg(tab.data(), n, j);
            const CassMixedEnt &e = tab[(size_t)t];
            const CassCfg &c = cfgs[e.set];
            if (!c.post) continue;
            const AudioSeg g = audio_seg(e.frames, L, Wb, j - e.seg0);
            CassBack s = carried_of(e).back;
            if (g.run_start != 0) s.post[0] = s.post[1] = 0;
            cass_back_span(c, s, rs.data() + e.plane * 2, nullptr, g.run_start, g.start - g.run_start);
            at_start[(size_t)j] = s;
            cass_back_span(c, s, rs.data() + e.plane * 2, tracks[t].io.dst, g.start, g.len);
            at_end[(size_t)j] = s;
        }
        for (int t = 0; t < n; t++) {
            const CassMixedEnt &e = tab[(size_t)t];
            const CassCfg &c = cfgs[e.set];
            if (!e.frames || !c.post) continue;
            const uint64_t nt = audio_seg_count(e.frames, L);
            CassBack truth = carried_of(e).back;
            for (uint64_t j = 0; j < nt; j++) {
                const AudioSeg g = audio_seg(e.frames, L, Wb, j);
                if (!cass_back_same(at_start[(size_t)(e.seg0 + j)], truth)) {
                    cass_back_span(c, truth, rs.data() + e.plane * 2, tracks[t].io.dst, g.start, g.len);
                    stats[t].repaired_back++;
                } else {
                    truth = at_end[(size_t)(e.seg0 + j)];
                }
            }
            if (e.state) e.state->back = truth;
        }
    }
    for (int t = 0; t < n; t++) {                                               // the history of the track's own length, the count, the taps
        const CassMixedEnt &e = tab[(size_t)t];
        if (!e.frames || !e.state) continue;
        const CassCfg &c = cfgs[e.set];
        for (uint64_t k = 0; k < (uint64_t)(c.taps - 1); k++)
            for (int ch = 0; ch < CASS_CHANNELS; ch++) e.state->hist[k][ch] = xs[(size_t)(e.xs + e.frames + k) * 2 + ch];
        e.state->front.count = e.count + e.frames;
        e.state->taps = (uint32_t)c.taps;
    }
    return true;
}

} // namespace ntscsim
