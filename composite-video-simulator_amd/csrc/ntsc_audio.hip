// ntsc_audio.hip -- the VHS audio chain of ffmpeg_ntsc / ffmpeg_to_composite as a device stage (include/ntscsim.h:
// ntscsim_audio_*).  The arithmetic is audio_chain.hpp; this file is its lane-parallel form.
//
// The chain is a serial recurrence (17 one-pole fp64 filters per channel-sample, a clip in the middle), so a call is cut
// into segments that start one warm-up early from a zero state (the plan of audio_chain.hpp) and each segment is run by
// a GROUP OF 21 ADJACENT LANES, one lane per stage of the chain: lane r works on channel-sample t - r at step t and
// hands its result to lane r + 1 (__shfl_up, two dwords).  Three groups share a wavefront.  Stages with per-channel
// state keep two values and alternate; the pre-/de-emphasis stages keep one, which IS the reference's cross-channel
// coupling (:920, :960).  k_audio_verify_repair then makes the result independent of the speculation.
// ntscsim_audio_tracks_device() runs many such streams side by side through a track table (k_audio_track_*).
// ntscsim_audio_mixed_tracks_device() does so with parameters per track: a set table in the call's records and a per-lane
// view of the track's cfg (k_audio_mixed_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "audio_chain.hpp"
#include "audio_hiss.hpp"
#include "glibc_rand.hpp"
#include "ntsc_frames.hpp"
#include "ntsc_stage.hpp"
#include "ntscsim.h"

namespace ntscsim {

#include "lane_rand.hpp"

constexpr int AUDIO_LANES = 21;          // stages of the chain = lanes of a group
constexpr int AUDIO_GROUPS = 3;          // groups of a wavefront
constexpr int AUDIO_RING = 3 * AUDIO_LANES;

struct AudioBlock {                      // one descriptor; first: its first frame in the call
    const int16_t *src;
    int16_t *dst;
    uint64_t first, frames;
};
struct AudioSegRec {
    AudioState at_start, at_end;         // at the segment's first own frame, behind its last
};

// ---------------------------------------------------------------------------------------- the draws
// Lane k of block b: the window at the block's position advanced by k chunks (the set bits of k pick the polynomials),
// then HISS_CHUNK draws kept in registers, 31 to a round.
__global__ __launch_bounds__(64) void k_audio_hiss(const AudioHissBlock *__restrict__ hb, int nblocks, const uint32_t *__restrict__ polys, int32_t *__restrict__ out)
{
    for (int b = (int)blockIdx.y; b < nblocks; b += (int)gridDim.y) {
        const uint64_t items = hb[b].items, first = hb[b].first;
        const int level = hb[b].level;                                          // per block: a mixed call's tracks differ in it
        const uint64_t nchunks = (items + HISS_CHUNK - 1) / HISS_CHUNK;
        for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nchunks; k += (uint64_t)gridDim.x * blockDim.x) {
            uint32_t w[61];
#pragma unroll
            for (int j = 0; j < 31; j++) w[j] = hb[b].w[j];
            for (int bit = 0; bit < HISS_POLYS && (k >> bit) != 0; bit++) {
                if (!((k >> bit) & 1)) continue;
#pragma unroll
                for (int i = 31; i < 61; i++) w[i] = w[i - 31] + w[i - 3];
                uint32_t o[31];
                jump61(polys + bit * 31, w, o);
#pragma unroll
                for (int j = 0; j < 31; j++) w[j] = o[j];
            }
            const uint64_t base = k * HISS_CHUNK;
            const uint64_t left = items - base;
            int32_t *dst = out + first + base;
            for (int round = 0; round < HISS_ROUNDS; round++) {
#pragma unroll
                for (int i = 0; i < 31; i++) {
                    const uint32_t v = w[i] + w[(i + 28) % 31];
                    w[i] = v;
                    const uint64_t idx = (uint64_t)(round * 31 + i);
                    if (idx < left) dst[idx] = audio_hiss_num(v >> 1, level);
                }
            }
        }
    }
}

void audio_hiss_launch(const AudioHissBlock *blocks, int m, uint64_t max_items, const uint32_t *polys, int32_t *out, hipStream_t st)
{
    const uint64_t chunks = (max_items + HISS_CHUNK - 1) / HISS_CHUNK;
    const unsigned gx = (unsigned)std::min<uint64_t>((chunks + 63) / 64, 65535), gy = (unsigned)std::min(m, 1024);
    hipLaunchKernelGGL(k_audio_hiss, dim3(gx, gy), dim3(64), 0, st, blocks, m, polys, out);
}

int audio_hiss_polys(const CtxStageView &v, uint32_t **polys)
{
    std::vector<uint32_t> host((size_t)HISS_POLYS * 31);
    for (int j = 0; j < HISS_POLYS; j++) {
        const RandPoly q = rand_poly_pow((uint64_t)HISS_CHUNK << j);
        std::memcpy(&host[(size_t)j * 31], q.c, sizeof(q.c));
    }
    STAGECHK(v, hipMalloc((void **)polys, host.size() * sizeof(uint32_t)));
    STAGECHK(v, hipMemcpy(*polys, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return NTSCSIM_OK;
}

// st != NULL: counts run from the ctx's sample count
__global__ __launch_bounds__(256) void k_audio_pulses(AudioCfg c, const AudioState *__restrict__ st, uint64_t count0, uint64_t n, uint8_t *__restrict__ out)
{
    const uint64_t base = count0 + (st ? st->count : 0);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = (uint8_t)audio_pulse_count(c, base + i);
}

// ---------------------------------------------------------------------------------------- the stage lanes
// every filter stage is ONE role -- the same four fp64 operations with a per-lane alpha and a per-lane output rule (prev,
// x - prev, x + (x - prev) * g) -- because the lanes of a wavefront that differ in role run one after the other
enum AudioRole { AR_LOAD, AR_FILTER, AR_PASS, AR_BUZZ_A, AR_BUZZ_B, AR_STORE, AR_IDLE };
enum AudioRule { AO_PREV, AO_HIGH, AO_EMPH };

struct AudioLane {
    int role, rule;
    int slot0, slot1;                    // values of the state this lane owns (-1: none)
    bool on;                             // false: the stage is switched off, the lane passes its input on
    double alpha, gain;
};

__device__ __forceinline__ AudioLane audio_idle_lane()
{
    AudioLane l;
    l.role = AR_IDLE;
    l.rule = AO_PREV;
    l.slot0 = l.slot1 = -1;
    l.on = true;
    l.alpha = 0;
    l.gain = 1.0;
    return l;
}

__device__ __forceinline__ AudioLane audio_lane(const AudioCfg &c, int r)
{
    AudioLane l = audio_idle_lane();
    const bool two = c.channels == 2;
    if (r == 0) l.role = AR_LOAD;
    else if (r <= 6) { l.role = AR_FILTER; l.slot0 = r - 1; l.slot1 = two ? 12 + r - 1 : -1; l.alpha = c.a_lo; }
    else if (r <= 12) { l.role = AR_FILTER; l.rule = AO_HIGH; l.slot0 = r - 1; l.slot1 = two ? 12 + r - 1 : -1; l.alpha = c.a_hi; }
    else if (r <= 14) { l.on = c.pre && r - 13 < c.channels; l.role = l.on ? AR_FILTER : AR_PASS; l.rule = AO_EMPH; l.slot0 = l.on ? 24 + r - 13 : -1; l.alpha = c.a_pre; }
    else if (r == 15) { l.role = AR_BUZZ_A; l.on = audio_buzz_on(c); }
    else if (r == 16) l.role = AR_BUZZ_B;
    else if (r == 17) { l.on = audio_boost_on(c); l.role = l.on ? AR_FILTER : AR_PASS; l.rule = AO_EMPH; l.slot0 = l.on ? 28 : -1; l.slot1 = l.on && two ? 29 : -1; l.alpha = c.a_boost; l.gain = c.boost_gain; }
    else if (r <= 19) { l.on = c.post && r - 18 < c.channels; l.role = l.on ? AR_FILTER : AR_PASS; l.slot0 = l.on ? 26 + r - 18 : -1; l.alpha = c.a_post; }
    else if (r == 20) l.role = AR_STORE;
    return l;
}

// What audio_run_lanes reads of a call, in two forms.  AudioCall: one cfg for every lane, a kernel argument, so all of it
// is wave-uniform.  AudioMixedView (below): the groups of a wavefront serve tracks with different cfgs, so a lane keeps
// what the steps read of its track's cfg -- and no more -- in registers.
struct AudioCall {
    AudioCfg c;
    const AudioBlock *blocks;
    const int32_t *hiss;                 // per channel-sample of the call, NULL without hiss
    const uint8_t *pulses;               // per frame of the call, NULL without buzz
    uint64_t total;                      // frames of the call
    int nblocks;

    __device__ __forceinline__ int channels() const { return c.channels; }
    __device__ __forceinline__ AudioLane lane(int r) const { return audio_lane(c, r); }
    __device__ __forceinline__ double buzz_step() const { return c.buzz / AUDIO_OVERSAMPLE / 2; }
    __device__ __forceinline__ bool hiss_on() const { return c.hiss_level != 0; }
    __device__ __forceinline__ bool buzz_on() const { return pulses != nullptr; }
    __device__ __forceinline__ int32_t hiss_at(uint64_t f, int ch, int cc) const { return hiss[f * ch + cc]; }
};

struct AudioMixedView {
    const AudioBlock *blocks;            // of all tracks, `first` in the plane: wave-uniform, as the two planes are
    const int32_t *hiss;
    const uint8_t *pulses;               // per frame of the plane
    uint64_t hiss_off;                   // channel-sample (plane frame f, channel cc) of the track is hiss[f * ch + cc + hiss_off]: the
                                         // track's hiss0 minus its plane frames in its own channels, modulo 2^64
    AudioLane L;                         // of this lane at its place in the group, from the track's cfg; the two buzz lanes own no
                                         // filter, so their alpha holds the track's buzz step
    int nblocks;
    int ch;
    bool hissing, buzzing;               // of the track

    __device__ __forceinline__ int channels() const { return ch; }
    __device__ __forceinline__ AudioLane lane(int) const { return L; }
    __device__ __forceinline__ double buzz_step() const { return L.alpha; }
    __device__ __forceinline__ bool hiss_on() const { return hissing; }
    __device__ __forceinline__ bool buzz_on() const { return buzzing; }
    __device__ __forceinline__ int32_t hiss_at(uint64_t f, int chn, int cc) const { return hiss[f * chn + cc + hiss_off]; }
};

// the block that holds frame f (f < total); b only moves forward
template <class K>
__device__ __forceinline__ void audio_seek(const K &k, int &b, uint64_t f)
{
    while (b + 1 < k.nblocks && f >= k.blocks[b].first + k.blocks[b].frames) b++;
}

// Frames [first, first + warm + own) of the call through the 21 lanes of one group; r: this lane's place in its group
// (>= AUDIO_LANES or !live: the lane only takes part in the hand-offs).  init[]: the state the run starts from; b0: a
// block at or in front of frame `first`, where the lane's block cursors start (a tracks call: the track's first).  The
// outputs of the last `own` frames are stored.  at_start (may be NULL) / at_end receive the values this lane owns, at
// the first own frame and behind the last; their other values and their counts are the caller's.
// ring: AUDIO_RING entries of the group for each of the three prefetched inputs -- every lane fetches, one period of 21
// steps ahead, what channel-sample (period * 21 + r) needs (input, hiss numerator, pulse count), so that no stage waits
// for memory inside a step.
template <class K>
__device__ void audio_run_lanes(const K &k, int r, bool live, uint64_t first, uint64_t warm, uint64_t own, const double *init,
                                AudioState *at_start, AudioState *at_end, int32_t *ring_in, int32_t *ring_hiss, int32_t *ring_pulses, int b0 = 0)
{
    const int ch = k.channels();
    const AudioLane L = k.lane(live ? r : 99);
    const uint64_t N = live ? (warm + own) * (uint64_t)ch : 0;                  // channel-samples of the run
    const uint64_t warm_items = warm * (uint64_t)ch;
    double st0 = L.slot0 >= 0 ? init[L.slot0] : 0.0, st1 = L.slot1 >= 0 ? init[L.slot1] : 0.0;
    const double q = k.buzz_step();
    const bool hiss_on = k.hiss_on();

    // prefetch cursor: channel-sample pf of the run, period by period
    uint64_t pf = (uint64_t)r;
    int pf_block = b0, st_block = b0;                                          // b0: a block at or in front of frame `first`
    int32_t pf_in = 0, pf_hiss = 0, pf_pulses = 0;
    uint64_t st_first = 0, st_end = 0;                                         // the block the store lane writes
    int16_t *st_dst = nullptr;
    const auto fetch = [&]() {
        pf_in = pf_hiss = pf_pulses = 0;
        if (r < AUDIO_LANES && pf < N) {
            const uint64_t f = first + (ch == 2 ? pf >> 1 : pf);
            const int cc = ch == 2 ? (int)(pf & 1) : 0;
            audio_seek(k, pf_block, f);
            pf_in = k.blocks[pf_block].src[(f - k.blocks[pf_block].first) * ch + cc];
            if (hiss_on) pf_hiss = k.hiss_at(f, ch, cc);
            if (k.buzz_on()) pf_pulses = k.pulses[f];
        }
    };
    int pslot = r;                                                             // ring entry of the period being fetched
    fetch();
    if (r < AUDIO_LANES) { ring_in[pslot] = pf_in; ring_hiss[pslot] = pf_hiss; ring_pulses[pslot] = pf_pulses; }
    pf += AUDIO_LANES;
    pslot += AUDIO_LANES;
    fetch();

    double y = 0.0;
    int64_t n = -(int64_t)r;                                                   // channel-sample of this lane at step t
    int slot = 0;                                                              // n % AUDIO_RING while n >= 0
    int chn = 0;
    uint64_t frame = first;
    int tp = 0;                                                                // t % AUDIO_LANES
    const uint64_t steps = N ? N + AUDIO_LANES : 0;
    __syncthreads();
    for (uint64_t t = 0; __any(t < steps); t++) {
        const double x = __shfl_up(y, 1);
        if (n >= 0 && (uint64_t)n < N) {
            if ((uint64_t)n == warm_items && at_start) {
                if (L.slot0 >= 0) at_start->v[L.slot0] = st0;
                if (L.slot1 >= 0) at_start->v[L.slot1] = st1;
            }
            double *prev = (chn && L.slot1 >= 0) ? &st1 : &st0;
            switch (L.role) {
            case AR_LOAD: y = (double)ring_in[slot] / 32768; break;
            case AR_FILTER: {
                const double t = audio_pole(*prev, x, L.alpha);
                const double d = x - t;
                y = L.rule == AO_PREV ? t : (L.rule == AO_HIGH ? d : x + d * L.gain);   // * 1.0 (pre-emphasis) changes no bit
                break;
            }
            case AR_PASS: y = x; break;
            case AR_BUZZ_A: {
                double s = x;
                if (L.on) {
                    const int p = min(ring_pulses[slot], 8);
                    for (int i = 0; i < p; i++) s -= q;
                }
                y = s;
                break;
            }
            case AR_BUZZ_B: {
                double s = x;
                if (k.buzz_on()) {
                    const int p = ring_pulses[slot] - 8;
                    for (int i = 0; i < p; i++) s -= q;
                }
                if (s > 1.0) s = 1.0;
                else if (s < -1.0) s = -1.0;
                if (hiss_on) s += ((double)ring_hiss[slot]) / 20000;
                y = s;
                break;
            }
            case AR_STORE:
                if ((uint64_t)n >= warm_items) {
                    if (frame >= st_end) {                                      // the block's bounds stay in registers: no load in a step
                        audio_seek(k, st_block, frame);
                        st_first = k.blocks[st_block].first;
                        st_end = st_first + k.blocks[st_block].frames;
                        st_dst = k.blocks[st_block].dst;
                    }
                    st_dst[(frame - st_first) * ch + chn] = audio_pack(x);
                }
                break;
            default: break;
            }
        }
        if (n >= 0) {
            slot = slot == AUDIO_RING - 1 ? 0 : slot + 1;
            if (++chn == ch) { chn = 0; frame++; }
        }
        n++;
        if (++tp == AUDIO_LANES) {                                             // a period ends: publish the next, fetch the one after
            tp = 0;
            __syncthreads();
            if (r < AUDIO_LANES) { ring_in[pslot] = pf_in; ring_hiss[pslot] = pf_hiss; ring_pulses[pslot] = pf_pulses; }
            pf += AUDIO_LANES;
            pslot = pslot >= 2 * AUDIO_LANES ? pslot - 2 * AUDIO_LANES : pslot + AUDIO_LANES;
            fetch();
            __syncthreads();
        }
    }
    if (N) {
        if (L.slot0 >= 0) at_end->v[L.slot0] = st0;
        if (L.slot1 >= 0) at_end->v[L.slot1] = st1;
    }
}

// One wavefront per workgroup, three segments per wavefront.
__global__ __launch_bounds__(64) void k_audio_segments(AudioCall k, const AudioState *__restrict__ carried, AudioSegRec *__restrict__ recs, uint32_t seg_len,
                                                       uint32_t warmup)
{
    __shared__ int32_t ring[AUDIO_GROUPS + 1][3][AUDIO_RING];
    __shared__ double init[AUDIO_GROUPS + 1][AUDIO_STATE_VALUES];
    const int lane = (int)threadIdx.x, g = lane / AUDIO_LANES, r = lane - g * AUDIO_LANES;
    const uint64_t nseg = audio_seg_count(k.total, seg_len);
    const uint64_t j = (uint64_t)blockIdx.x * AUDIO_GROUPS + (uint64_t)g;
    const bool live = g < AUDIO_GROUPS && j < nseg;
    AudioSeg s{0, 0, 0};
    if (live) {
        s = audio_seg(k.total, seg_len, warmup, j);
        const bool spec = s.run_start != 0;
        for (int i = r; i < AUDIO_STATE_VALUES; i += AUDIO_LANES) {
            const double v = spec && audio_value_live(k.c, i) ? 0.0 : carried->v[i];
            init[g][i] = v;
            recs[j].at_start.v[i] = v;
            recs[j].at_end.v[i] = v;
        }
        if (r == 0) {
            recs[j].at_start.count = carried->count + s.start;
            recs[j].at_end.count = carried->count + s.start + s.len;
        }
    }
    __syncthreads();
    audio_run_lanes(k, r, live, s.run_start, s.start - s.run_start, s.len, init[g], live ? &recs[j].at_start : nullptr, live ? &recs[j].at_end : nullptr,
                    ring[g][0], ring[g][1], ring[g][2]);
}

// One wavefront.  truth: the state behind the last verified segment.
__global__ __launch_bounds__(64) void k_audio_verify_repair(AudioCall k, AudioState *__restrict__ carried, const AudioSegRec *__restrict__ recs, uint32_t seg_len,
                                                            uint32_t warmup, uint64_t *__restrict__ stats)
{
    __shared__ int32_t ring[3][AUDIO_RING];
    __shared__ AudioState truth;
    __shared__ double init[AUDIO_STATE_VALUES];
    const int lane = (int)threadIdx.x;
    const uint64_t nseg = audio_seg_count(k.total, seg_len);
    if (lane < AUDIO_STATE_VALUES) truth.v[lane] = carried->v[lane];
    if (lane == AUDIO_STATE_VALUES) truth.count = carried->count;
    __syncthreads();
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        bool same = true;
        if (lane < AUDIO_STATE_VALUES) same = __double_as_longlong(recs[j].at_start.v[lane]) == __double_as_longlong(truth.v[lane]);
        if (lane == AUDIO_STATE_VALUES) same = recs[j].at_start.count == truth.count;
        const bool ok = __all(same);
        __syncthreads();
        if (ok) {
            if (lane < AUDIO_STATE_VALUES) truth.v[lane] = recs[j].at_end.v[lane];
            if (lane == AUDIO_STATE_VALUES) truth.count = recs[j].at_end.count;
        } else {
            const AudioSeg s = audio_seg(k.total, seg_len, warmup, j);
            if (lane < AUDIO_STATE_VALUES) init[lane] = truth.v[lane];
            __syncthreads();
            audio_run_lanes(k, lane, lane < AUDIO_LANES, s.start, 0, s.len, init, nullptr, &truth, ring[0], ring[1], ring[2]);
            if (lane == 0) truth.count += s.len;
            repaired++;
        }
        __syncthreads();
    }
    if (lane < AUDIO_STATE_VALUES) carried->v[lane] = truth.v[lane];
    if (lane == AUDIO_STATE_VALUES) carried->count = truth.count;
    if (lane == 0) { stats[0] = nseg; stats[1] = repaired; }
}

// ---------------------------------------------------------------------------------------- many tracks
// ntscsim_audio_tracks_device(): independent streams side by side (the track table of audio_chain.hpp).  The kernels
// above stay the single stream's; these hand the same audio_run_lanes a track's VIEW.  The three groups of a wavefront
// may serve three tracks, so what differs between tracks lives in VGPRs; to keep that small the tracks are laid into ONE
// frame numbering, the PLANE (track t owns frames [plane_t, plane_t + frames_t) of it): the hiss and pulse planes and the
// blocks' `first` are indexed by it, their base pointers stay wave-uniform, and a view differs from the call only in
// where the run stands in the plane and in the track's range of blocks (b0 .. nblocks).
struct AudioTracksCall {
    AudioCfg c;
    const AudioTrackEnt *tracks;
    const AudioBlock *blocks;            // of all tracks, `first` in the plane
    const int32_t *hiss;                 // per channel-sample / per frame of the plane
    const uint8_t *pulses;
    uint64_t nseg;                       // segments of the call
    int ntracks;
};

__device__ __forceinline__ AudioCall audio_track_view(const AudioTracksCall &k, const AudioTrackEnt &e)
{
    AudioCall v;
    v.c = k.c;
    v.blocks = k.blocks;
    v.hiss = k.hiss;
    v.pulses = k.pulses;
    v.total = e.plane + e.frames;                                               // where the track ends in the plane
    v.nblocks = e.block0 + e.nblocks;                                           // audio_seek stops at the track's last block
    return v;
}

// pulse counts per frame of every track, each from its own sample count
__global__ __launch_bounds__(256) void k_audio_track_pulses(AudioCfg c, const AudioTrackEnt *__restrict__ tracks, int ntracks, uint8_t *__restrict__ out)
{
    for (int t = (int)blockIdx.y; t < ntracks; t += (int)gridDim.y) {
        const AudioTrackEnt e = tracks[t];
        const uint64_t base = e.state ? e.state->count : 0;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e.frames; i += (uint64_t)gridDim.x * blockDim.x)
            out[e.plane + i] = (uint8_t)audio_pulse_count(c, base + i);
    }
}

// One wavefront per workgroup; group g of workgroup b takes call-wide segment 3 b + g, whatever track it belongs to.
__global__ __launch_bounds__(64) void k_audio_track_segments(AudioTracksCall k, AudioSegRec *__restrict__ recs, uint32_t seg_len, uint32_t warmup)
{
    __shared__ int32_t ring[AUDIO_GROUPS + 1][3][AUDIO_RING];
    __shared__ double init[AUDIO_GROUPS + 1][AUDIO_STATE_VALUES];
    const int lane = (int)threadIdx.x, g = lane / AUDIO_LANES, r = lane - g * AUDIO_LANES;
    const uint64_t j = (uint64_t)blockIdx.x * AUDIO_GROUPS + (uint64_t)g;
    const bool live = g < AUDIO_GROUPS && j < k.nseg;
    AudioTrackEnt e{0, 0, 0, nullptr, 0, 0};
    AudioSeg s{0, 0, 0};
    if (live) {
        e = k.tracks[audio_track_of(k.tracks, k.ntracks, j)];
        s = audio_seg(e.frames, seg_len, warmup, j - e.seg0);                    // clamps at frame 0 of this track
        const bool spec = s.run_start != 0;
        for (int i = r; i < AUDIO_STATE_VALUES; i += AUDIO_LANES) {
            const double v = (spec && audio_value_live(k.c, i)) || !e.state ? 0.0 : e.state->v[i];
            init[g][i] = v;
            recs[j].at_start.v[i] = v;
            recs[j].at_end.v[i] = v;
        }
        if (r == 0) {
            const uint64_t count = e.state ? e.state->count : 0;
            recs[j].at_start.count = count + s.start;
            recs[j].at_end.count = count + s.start + s.len;
        }
    }
    __syncthreads();
    const AudioCall view = audio_track_view(k, e);
    audio_run_lanes(view, r, live, e.plane + s.run_start, s.start - s.run_start, s.len, init[g], live ? &recs[j].at_start : nullptr,
                    live ? &recs[j].at_end : nullptr, ring[g][0], ring[g][1], ring[g][2], e.block0);
}

// One workgroup (one wavefront) per track: the walk of k_audio_verify_repair over that track's records, from that
// track's true state.
__global__ __launch_bounds__(64) void k_audio_track_verify(AudioTracksCall k, const AudioSegRec *__restrict__ recs, uint32_t seg_len, uint32_t warmup,
                                                           uint64_t *__restrict__ stats)
{
    __shared__ int32_t ring[3][AUDIO_RING];
    __shared__ AudioState truth;
    __shared__ double init[AUDIO_STATE_VALUES];
    const int lane = (int)threadIdx.x;
    const AudioTrackEnt e = k.tracks[blockIdx.x];
    const AudioCall view = audio_track_view(k, e);
    const uint64_t nseg = audio_seg_count(e.frames, seg_len);
    recs += e.seg0;
    if (lane < AUDIO_STATE_VALUES) truth.v[lane] = e.state ? e.state->v[lane] : 0.0;
    if (lane == AUDIO_STATE_VALUES) truth.count = e.state ? e.state->count : 0;
    __syncthreads();
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        bool same = true;
        if (lane < AUDIO_STATE_VALUES) same = __double_as_longlong(recs[j].at_start.v[lane]) == __double_as_longlong(truth.v[lane]);
        if (lane == AUDIO_STATE_VALUES) same = recs[j].at_start.count == truth.count;
        const bool ok = __all(same);
        __syncthreads();
        if (ok) {
            if (lane < AUDIO_STATE_VALUES) truth.v[lane] = recs[j].at_end.v[lane];
            if (lane == AUDIO_STATE_VALUES) truth.count = recs[j].at_end.count;
        } else {
            const AudioSeg s = audio_seg(e.frames, seg_len, warmup, j);
            if (lane < AUDIO_STATE_VALUES) init[lane] = truth.v[lane];
            __syncthreads();
            audio_run_lanes(view, lane, lane < AUDIO_LANES, e.plane + s.start, 0, s.len, init, nullptr, &truth, ring[0], ring[1], ring[2], e.block0);
            if (lane == 0) truth.count += s.len;
            repaired++;
        }
        __syncthreads();
    }
    if (e.state) {
        if (lane < AUDIO_STATE_VALUES) e.state->v[lane] = truth.v[lane];
        if (lane == AUDIO_STATE_VALUES) e.state->count = truth.count;
    }
    if (lane == 0) { stats[2 * (uint64_t)blockIdx.x] = nseg; stats[2 * (uint64_t)blockIdx.x + 1] = repaired; }
}

// ---------------------------------------------------------------------------------------- mixed tracks
// ntscsim_audio_mixed_tracks_device(): a tracks call whose tracks each name a cfg of a SET TABLE (device records of the
// call).  A lane reads its track's cfg once, in front of the run, and keeps of it what AudioMixedView holds; the 120-byte
// AudioCfg is dead before the first step.  The pulse plane is per frame as before; the hiss plane is per channel-sample
// and tracks differ in channels, so a track finds its part through AudioTrackEnt::hiss0.
struct AudioMixedCall {
    const AudioCfg *cfgs;                // the set table
    const AudioTrackEnt *tracks;
    const AudioBlock *blocks;            // of all tracks, `first` in the plane
    const int32_t *hiss;
    const uint8_t *pulses;
    uint64_t nseg;                       // segments of the call
    int ntracks;
};

// r: the lane's place in its group (>= AUDIO_LANES: it only takes part in the hand-offs)
__device__ __forceinline__ AudioMixedView audio_mixed_view(const AudioMixedCall &k, const AudioTrackEnt &e, const AudioCfg &c, int r)
{
    AudioMixedView v;
    v.blocks = k.blocks;
    v.hiss = k.hiss;
    v.pulses = k.pulses;
    v.hiss_off = e.hiss0 - e.plane * (uint64_t)c.channels;
    v.L = audio_lane(c, r < AUDIO_LANES ? r : 99);
    if (v.L.role == AR_BUZZ_A || v.L.role == AR_BUZZ_B) v.L.alpha = c.buzz / AUDIO_OVERSAMPLE / 2;
    v.hissing = c.hiss_level != 0;
    v.buzzing = audio_buzz_on(c);
    v.nblocks = e.block0 + e.nblocks;                                           // audio_seek stops at the track's last block
    v.ch = c.channels;
    return v;
}

// pulse counts per frame of every track whose buzz is on, each from its own sample count with its own line rates
__global__ __launch_bounds__(256) void k_audio_mixed_pulses(const AudioCfg *__restrict__ cfgs, const AudioTrackEnt *__restrict__ tracks, int ntracks,
                                                            uint8_t *__restrict__ out)
{
    for (int t = (int)blockIdx.y; t < ntracks; t += (int)gridDim.y) {
        const AudioTrackEnt e = tracks[t];
        const AudioCfg c = cfgs[e.set];
        if (!audio_buzz_on(c)) continue;                                        // nobody reads these frames of the plane
        const uint64_t base = e.state ? e.state->count : 0;
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e.frames; i += (uint64_t)gridDim.x * blockDim.x)
            out[e.plane + i] = (uint8_t)audio_pulse_count(c, base + i);
    }
}

// k_audio_track_segments with the cfg, the warm-up and the hiss base of the segment's own track
__global__ __launch_bounds__(64) void k_audio_mixed_segments(AudioMixedCall k, AudioSegRec *__restrict__ recs, uint32_t seg_len)
{
    __shared__ int32_t ring[AUDIO_GROUPS + 1][3][AUDIO_RING];
    __shared__ double init[AUDIO_GROUPS + 1][AUDIO_STATE_VALUES];
    const int lane = (int)threadIdx.x, g = lane / AUDIO_LANES, r = lane - g * AUDIO_LANES;
    const uint64_t j = (uint64_t)blockIdx.x * AUDIO_GROUPS + (uint64_t)g;
    const bool live = g < AUDIO_GROUPS && j < k.nseg;
    AudioSeg s{0, 0, 0};
    uint64_t plane = 0;
    int block0 = 0;
    AudioMixedView view;
    view.blocks = k.blocks;
    view.hiss = k.hiss;
    view.pulses = k.pulses;
    view.hiss_off = 0;
    view.hissing = view.buzzing = false;
    view.L = audio_idle_lane();
    view.nblocks = 0;
    view.ch = 1;
    if (live) {
        const AudioTrackEnt e = k.tracks[audio_track_of(k.tracks, k.ntracks, j)];
        const AudioCfg c = k.cfgs[e.set];
        s = audio_seg(e.frames, seg_len, e.warmup, j - e.seg0);                  // clamps at frame 0 of this track
        const bool spec = s.run_start != 0;
        for (int i = r; i < AUDIO_STATE_VALUES; i += AUDIO_LANES) {
            const double v = (spec && audio_value_live(c, i)) || !e.state ? 0.0 : e.state->v[i];
            init[g][i] = v;
            recs[j].at_start.v[i] = v;
            recs[j].at_end.v[i] = v;
        }
        if (r == 0) {
            const uint64_t count = e.state ? e.state->count : 0;
            recs[j].at_start.count = count + s.start;
            recs[j].at_end.count = count + s.start + s.len;
        }
        view = audio_mixed_view(k, e, c, r);
        plane = e.plane;
        block0 = e.block0;
    }
    __syncthreads();
    audio_run_lanes(view, r, live, plane + s.run_start, s.start - s.run_start, s.len, init[g], live ? &recs[j].at_start : nullptr,
                    live ? &recs[j].at_end : nullptr, ring[g][0], ring[g][1], ring[g][2], block0);
}


// One workgroup (one wavefront) per track, as k_audio_track_verify: the track's cfg is the workgroup's.
__global__ __launch_bounds__(64) void k_audio_mixed_verify(AudioMixedCall k, const AudioSegRec *__restrict__ recs, uint32_t seg_len,
                                                           uint64_t *__restrict__ stats)
{
    __shared__ int32_t ring[3][AUDIO_RING];
    __shared__ AudioState truth;
    __shared__ double init[AUDIO_STATE_VALUES];
    const int lane = (int)threadIdx.x;
    const AudioTrackEnt e = k.tracks[blockIdx.x];
    const AudioMixedView view = audio_mixed_view(k, e, k.cfgs[e.set], lane);
    const uint64_t nseg = audio_seg_count(e.frames, seg_len);
    recs += e.seg0;
    if (lane < AUDIO_STATE_VALUES) truth.v[lane] = e.state ? e.state->v[lane] : 0.0;
    if (lane == AUDIO_STATE_VALUES) truth.count = e.state ? e.state->count : 0;
    __syncthreads();
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        bool same = true;
        if (lane < AUDIO_STATE_VALUES) same = __double_as_longlong(recs[j].at_start.v[lane]) == __double_as_longlong(truth.v[lane]);
        if (lane == AUDIO_STATE_VALUES) same = recs[j].at_start.count == truth.count;
        const bool ok = __all(same);
        __syncthreads();
        if (ok) {
            if (lane < AUDIO_STATE_VALUES) truth.v[lane] = recs[j].at_end.v[lane];
            if (lane == AUDIO_STATE_VALUES) truth.count = recs[j].at_end.count;
        } else {
            const AudioSeg s = audio_seg(e.frames, seg_len, e.warmup, j);
            if (lane < AUDIO_STATE_VALUES) init[lane] = truth.v[lane];
            __syncthreads();
            audio_run_lanes(view, lane, lane < AUDIO_LANES, e.plane + s.start, 0, s.len, init, nullptr, &truth, ring[0], ring[1], ring[2], e.block0);
            if (lane == 0) truth.count += s.len;
            repaired++;
        }
        __syncthreads();
    }
    if (e.state && nseg) {                                                      // a track without frames (or a copied one) keeps its state
        if (lane < AUDIO_STATE_VALUES) e.state->v[lane] = truth.v[lane];
        if (lane == AUDIO_STATE_VALUES) e.state->count = truth.count;
    }
    if (lane == 0) { stats[2 * (uint64_t)blockIdx.x] = nseg; stats[2 * (uint64_t)blockIdx.x + 1] = repaired; }
}

// ---------------------------------------------------------------------------------------- host side
struct AudioStageState {
    ntscsim_audio_params prm;
    AudioCfg cfg;
    AudioState *state = nullptr;         // device: the carried state
    uint32_t *polys = nullptr;           // device: HISS_POLYS polynomials
    uint64_t *stats = nullptr;           // device: segments, repaired of the last call
    int32_t *hiss = nullptr;
    uint8_t *pulses = nullptr;
    AudioSegRec *recs = nullptr;
    size_t hiss_cap = 0, pulses_cap = 0, recs_cap = 0;
    uint64_t *track_stats = nullptr;     // device: segments, repaired per track of the last tracks call
    size_t track_stats_cap = 0;          // in values: two per track
    int last_tracks = 0;
    uint32_t plan_len = 0, plan_warmup = 0;   // 0: the default
    bool plan_warmup_set = false;
    RecordSlots<> slots;
    FrameArena frames;                   // ntscsim_audio_host()
    bool timing = false;
    std::vector<hipEvent_t> marks;       // four per call while timing
};

static void audio_drop_marks(AudioStageState *k)
{
    for (hipEvent_t e : k->marks) (void)hipEventDestroy(e);
    k->marks.clear();
}

void audio_state_destroy(AudioStageState *k)
{
    if (!k) return;
    if (k->state) (void)hipFree(k->state);
    if (k->polys) (void)hipFree(k->polys);
    if (k->stats) (void)hipFree(k->stats);
    if (k->hiss) (void)hipFree(k->hiss);
    if (k->pulses) (void)hipFree(k->pulses);
    if (k->recs) (void)hipFree(k->recs);
    if (k->track_stats) (void)hipFree(k->track_stats);
    audio_drop_marks(k);
    k->slots.release();
    k->frames.release();
    delete k;
}

} // namespace ntscsim

using namespace ntscsim;

namespace {

AudioCfg audio_cfg_of(const ntscsim_audio_params &p)
{
    AudioCfg c;
    std::memset(&c, 0, sizeof(c));
    c.enabled = p.enabled != 0;
    c.channels = p.channels;
    c.hifi = p.hifi != 0;
    c.pre = p.preemphasis != 0;
    c.post = p.deemphasis != 0;
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

int audio_quiet(const CtxStageView &v)
{
    STAGECHK(v, hipSetDevice(v.device));
    STAGECHK(v, hipDeviceSynchronize());
    return NTSCSIM_OK;
}

template <class T>
int audio_grow(const CtxStageView &v, T *&p, size_t &cap, size_t want)
{
    if (want <= cap) return NTSCSIM_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    const size_t n = want + want / 4 + 1024;
    STAGECHK(v, hipMalloc((void **)&p, n * sizeof(T)));
    cap = n;
    return NTSCSIM_OK;
}

int audio_mark(const CtxStageView &v, AudioStageState *k, hipStream_t st)
{
    if (!k->timing) return NTSCSIM_OK;
    hipEvent_t e = nullptr;
    STAGECHK(v, hipEventCreate(&e));
    k->marks.push_back(e);
    STAGECHK(v, hipEventRecord(e, st));
    return NTSCSIM_OK;
}

int audio_blocks(ntscsim_ctx *c, const ntscsim_audio_desc *descs, int n, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    AudioStageState *k = *v.audio;
    const AudioCfg &cfg = k->cfg;
    const size_t fbytes = (size_t)cfg.channels * sizeof(int16_t);
    // every descriptor checked before anything is enqueued or the rand() position moves
    std::vector<Span> srcs;
    uint64_t total = 0;
    for (int i = 0; i < n; i++) {
        const ntscsim_audio_desc &d = descs[i];
        if (d.samples == 0) continue;
        if (!d.src || !d.dst || (((uintptr_t)d.src | (uintptr_t)d.dst) & 1)) return NTSCSIM_E_ARG;
        srcs.push_back(Span{(uintptr_t)d.src, (uintptr_t)d.src + (size_t)d.samples * fbytes});
        total += d.samples;
    }
    std::sort(srcs.begin(), srcs.end(), [](const Span &x, const Span &y) { return x.a < y.a; });
    std::vector<uintptr_t> reach(srcs.size());                                  // the furthest end among srcs[0..i]
    for (size_t i = 0; i < srcs.size(); i++) reach[i] = std::max(srcs[i].b, i ? reach[i - 1] : 0);
    for (int i = 0; i < n; i++) {
        const ntscsim_audio_desc &d = descs[i];
        if (d.samples == 0) continue;
        const uintptr_t a = (uintptr_t)d.dst, b = a + (size_t)d.samples * fbytes;
        const size_t m = (size_t)(std::lower_bound(srcs.begin(), srcs.end(), b, [](const Span &x, uintptr_t e) { return x.a < e; }) - srcs.begin());
        if (m > 0 && reach[m - 1] > a) return NTSCSIM_E_ARG;                    // a warm-up reads input again
    }
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    audio_drop_marks(k);
    if (!cfg.enabled) {                                                         // -nocomp: the tool does not call the chain
        for (int i = 0; i < n; i++)
            if (descs[i].samples) STAGECHK(v, hipMemcpyAsync(descs[i].dst, descs[i].src, (size_t)descs[i].samples * fbytes, hipMemcpyDeviceToDevice, st));
        STAGECHK(v, hipMemsetAsync(k->stats, 0, 2 * sizeof(uint64_t), st));
        return NTSCSIM_OK;
    }
    const bool hiss = cfg.hiss_level != 0, buzz = audio_buzz_on(cfg);
    const uint32_t L = k->plan_len ? k->plan_len : AUDIO_DEFAULT_SEG;
    const uint32_t W = k->plan_warmup_set ? k->plan_warmup : audio_default_warmup(cfg);
    const uint64_t nseg = audio_seg_count(total, L);
    // the rand() position moves at call time, whatever becomes of the launch
    uint64_t pos = ntscsim_get_rng_pos(c);
    std::vector<uint64_t> block_pos((size_t)n);
    for (int i = 0; i < n; i++) {
        if (descs[i].rng_pos != NTSCSIM_RNG_AUTO) pos = descs[i].rng_pos;
        block_pos[(size_t)i] = pos;
        if (hiss) pos += (uint64_t)descs[i].samples * (uint64_t)cfg.channels;
    }
    ntscsim_set_rng_pos(c, pos);
    if (total == 0) {
        STAGECHK(v, hipMemsetAsync(k->stats, 0, 2 * sizeof(uint64_t), st));
        return NTSCSIM_OK;
    }
    if ((hiss && total * cfg.channels > k->hiss_cap) || (buzz && total > k->pulses_cap) || nseg > k->recs_cap) {
        int rc = k->slots.wait_all(v);                                          // launches in flight use what is replaced
        if (rc == NTSCSIM_OK && hiss) rc = audio_grow(v, k->hiss, k->hiss_cap, (size_t)total * cfg.channels);
        if (rc == NTSCSIM_OK && buzz) rc = audio_grow(v, k->pulses, k->pulses_cap, (size_t)total);
        if (rc == NTSCSIM_OK) rc = audio_grow(v, k->recs, k->recs_cap, (size_t)nseg);
        if (rc != NTSCSIM_OK) return rc;
    }
    // records: the blocks that have frames, then their rand() windows
    int m = 0;
    for (int i = 0; i < n; i++) m += descs[i].samples != 0;
    const size_t blocks_bytes = (size_t)m * sizeof(AudioBlock), hb_bytes = hiss ? (size_t)m * sizeof(AudioHissBlock) : 0;
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, blocks_bytes + hb_bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    AudioBlock *blocks = reinterpret_cast<AudioBlock *>(slot->host);
    AudioHissBlock *hb = reinterpret_cast<AudioHissBlock *>(slot->host + blocks_bytes);
    uint64_t first = 0, max_items = 0;
    RandSeq seq(rand_state_origin());
    uint64_t seq_pos = UINT64_MAX;                                              // where seq stands; UINT64_MAX: nowhere
    for (int i = 0, o = 0; i < n; i++) {
        const ntscsim_audio_desc &d = descs[i];
        if (d.samples == 0) continue;
        blocks[o] = AudioBlock{d.src, d.dst, first, d.samples};
        if (hiss) {
            audio_hiss_window(hb[o], seq, seq_pos, block_pos[(size_t)i], first * cfg.channels, (uint64_t)d.samples * cfg.channels, cfg.hiss_level);
            max_items = std::max(max_items, hb[o].items);
        }
        first += d.samples;
        o++;
    }
    STAGECHK(v, hipMemcpyAsync(slot->dev, slot->host, blocks_bytes + hb_bytes, hipMemcpyHostToDevice, st));
    AudioCall call;
    call.c = cfg;
    call.blocks = reinterpret_cast<const AudioBlock *>(slot->dev);
    call.hiss = hiss ? k->hiss : nullptr;
    call.pulses = buzz ? k->pulses : nullptr;
    call.total = total;
    call.nblocks = m;
    int lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    if (hiss) {
        audio_hiss_launch(reinterpret_cast<const AudioHissBlock *>(slot->dev + blocks_bytes), m, max_items, k->polys, k->hiss, st);
        lrc = stage_launched(v, nullptr, st, "k_audio_hiss");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    if (buzz) {
        hipLaunchKernelGGL(k_audio_pulses, dim3((unsigned)std::min<uint64_t>((total + 255) / 256, 65535)), dim3(256), 0, st, cfg, k->state, (uint64_t)0, total,
                           k->pulses);
        lrc = stage_launched(v, nullptr, st, "k_audio_pulses");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_audio_segments, dim3((unsigned)((nseg + AUDIO_GROUPS - 1) / AUDIO_GROUPS)), dim3(64), 0, st, call, k->state, k->recs, L, W);
    lrc = stage_launched(v, nullptr, st, "k_audio_segments");
    if (lrc == NTSCSIM_OK) lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_audio_verify_repair, dim3(1), dim3(64), 0, st, call, k->state, k->recs, L, W, k->stats);
    lrc = stage_launched(v, slot, st, "k_audio_verify_repair");
    return lrc == NTSCSIM_OK ? audio_mark(v, k, st) : lrc;
}

// ntscsim_audio_tracks_device(): n independent streams in one launch of each kernel
int audio_tracks(ntscsim_ctx *c, const ntscsim_audio_track *tracks, int n, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    AudioStageState *k = *v.audio;
    const AudioCfg &cfg = k->cfg;
    const size_t fbytes = (size_t)cfg.channels * sizeof(int16_t);
    // every track and descriptor checked before anything is enqueued or the rand() position moves
    std::vector<Span> srcs;
    std::vector<uintptr_t> states;
    uint64_t total = 0;
    size_t m = 0;                                                               // blocks that have frames
    for (int t = 0; t < n; t++) {
        const ntscsim_audio_track &tr = tracks[t];
        if (tr.n_blocks < 0 || (tr.n_blocks > 0 && !tr.blocks) || ((uintptr_t)tr.state & 7)) return NTSCSIM_E_ARG;
        if (tr.state) states.push_back((uintptr_t)tr.state);
        for (int i = 0; i < tr.n_blocks; i++) {
            const ntscsim_audio_desc &d = tr.blocks[i];
            if (d.samples == 0) continue;
            if (!d.src || !d.dst || (((uintptr_t)d.src | (uintptr_t)d.dst) & 1)) return NTSCSIM_E_ARG;
            srcs.push_back(Span{(uintptr_t)d.src, (uintptr_t)d.src + (size_t)d.samples * fbytes});
            total += d.samples;
            m++;
        }
    }
    if (m > (size_t)INT32_MAX) return NTSCSIM_E_ARG;
    std::sort(states.begin(), states.end());
    for (size_t i = 1; i < states.size(); i++)
        if (states[i] - states[i - 1] < sizeof(AudioState)) return NTSCSIM_E_ARG;   // two tracks would share a state
    std::sort(srcs.begin(), srcs.end(), [](const Span &x, const Span &y) { return x.a < y.a; });
    std::vector<uintptr_t> reach(srcs.size());                                  // the furthest end among srcs[0..i]
    for (size_t i = 0; i < srcs.size(); i++) reach[i] = std::max(srcs[i].b, i ? reach[i - 1] : 0);
    for (int t = 0; t < n; t++)
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_audio_desc &d = tracks[t].blocks[i];
            if (d.samples == 0) continue;
            const uintptr_t a = (uintptr_t)d.dst, b = a + (size_t)d.samples * fbytes;
            const size_t at = (size_t)(std::lower_bound(srcs.begin(), srcs.end(), b, [](const Span &x, uintptr_t e) { return x.a < e; }) - srcs.begin());
            if (at > 0 && reach[at - 1] > a) return NTSCSIM_E_ARG;              // a warm-up reads input again, in any track
        }
    STAGECHK(v, hipSetDevice(v.device));
    if (2 * (size_t)n > k->track_stats_cap) {
        int rc = k->slots.wait_all(v);                                          // launches in flight use what is replaced
        if (rc == NTSCSIM_OK) rc = audio_grow(v, k->track_stats, k->track_stats_cap, 2 * (size_t)n);
        if (rc != NTSCSIM_OK) return rc;
    }
    v.kernels->clear();
    audio_drop_marks(k);
    k->last_tracks = n;
    const size_t stats_bytes = (size_t)n * 2 * sizeof(uint64_t);
    if (!cfg.enabled) {                                                         // -nocomp: the tool does not call the chain
        for (int t = 0; t < n; t++)
            for (int i = 0; i < tracks[t].n_blocks; i++) {
                const ntscsim_audio_desc &d = tracks[t].blocks[i];
                if (d.samples) STAGECHK(v, hipMemcpyAsync(d.dst, d.src, (size_t)d.samples * fbytes, hipMemcpyDeviceToDevice, st));
            }
        if (n) STAGECHK(v, hipMemsetAsync(k->track_stats, 0, stats_bytes, st));
        return NTSCSIM_OK;
    }
    const bool hiss = cfg.hiss_level != 0, buzz = audio_buzz_on(cfg);
    const uint32_t L = k->plan_len ? k->plan_len : AUDIO_DEFAULT_SEG;
    const uint32_t W = k->plan_warmup_set ? k->plan_warmup : audio_default_warmup(cfg);
    // the rand() position moves at call time, whatever becomes of the launch: tracks in order, blocks in order
    uint64_t pos = ntscsim_get_rng_pos(c);
    std::vector<uint64_t> block_pos;
    block_pos.reserve(m);
    for (int t = 0; t < n; t++)
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_audio_desc &d = tracks[t].blocks[i];
            if (d.rng_pos != NTSCSIM_RNG_AUTO) pos = d.rng_pos;
            if (d.samples) block_pos.push_back(pos);
            if (hiss) pos += (uint64_t)d.samples * (uint64_t)cfg.channels;
        }
    ntscsim_set_rng_pos(c, pos);
    if (total == 0) {
        if (n) STAGECHK(v, hipMemsetAsync(k->track_stats, 0, stats_bytes, st));
        return NTSCSIM_OK;
    }
    // records: the track table, the blocks that have frames, their rand() windows
    const size_t tab_bytes = (size_t)n * sizeof(AudioTrackEnt), blocks_bytes = m * sizeof(AudioBlock), hb_bytes = hiss ? m * sizeof(AudioHissBlock) : 0;
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, tab_bytes + blocks_bytes + hb_bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    AudioTrackEnt *tab = reinterpret_cast<AudioTrackEnt *>(slot->host);
    AudioBlock *blocks = reinterpret_cast<AudioBlock *>(slot->host + tab_bytes);
    AudioHissBlock *hb = reinterpret_cast<AudioHissBlock *>(slot->host + tab_bytes + blocks_bytes);
    int o = 0;
    uint64_t total_before = 0;                                                  // = the plane of the track, as audio_tracks_layout() sets it
    for (int t = 0; t < n; t++) {
        AudioTrackEnt &e = tab[t];
        e.frames = 0;
        e.state = reinterpret_cast<AudioState *>(tracks[t].state);
        e.block0 = o;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_audio_desc &d = tracks[t].blocks[i];
            if (d.samples == 0) continue;
            blocks[o++] = AudioBlock{d.src, d.dst, total_before + e.frames, d.samples};   // first: in the plane
            e.frames += d.samples;
        }
        e.nblocks = o - e.block0;
        total_before += e.frames;
    }
    const uint64_t nseg = audio_tracks_layout(tab, n, L);
    uint64_t max_items = 0, max_frames = 0;
    if (hiss) {
        RandSeq seq(rand_state_origin());
        uint64_t seq_pos = UINT64_MAX;                                          // where seq stands; UINT64_MAX: nowhere
        for (int t = 0; t < n; t++)
            for (int b = tab[t].block0; b < tab[t].block0 + tab[t].nblocks; b++) {
                audio_hiss_window(hb[b], seq, seq_pos, block_pos[(size_t)b], blocks[b].first * cfg.channels, blocks[b].frames * cfg.channels, cfg.hiss_level);
                max_items = std::max(max_items, hb[b].items);
            }
    }
    for (int t = 0; t < n; t++) max_frames = std::max(max_frames, tab[t].frames);
    if ((hiss && total * cfg.channels > k->hiss_cap) || (buzz && total > k->pulses_cap) || nseg > k->recs_cap) {
        int grc = k->slots.wait_all(v);                                         // launches in flight use what is replaced
        if (grc == NTSCSIM_OK && hiss) grc = audio_grow(v, k->hiss, k->hiss_cap, (size_t)total * cfg.channels);
        if (grc == NTSCSIM_OK && buzz) grc = audio_grow(v, k->pulses, k->pulses_cap, (size_t)total);
        if (grc == NTSCSIM_OK) grc = audio_grow(v, k->recs, k->recs_cap, (size_t)nseg);
        if (grc != NTSCSIM_OK) return grc;
    }
    STAGECHK(v, hipMemcpyAsync(slot->dev, slot->host, tab_bytes + blocks_bytes + hb_bytes, hipMemcpyHostToDevice, st));
    AudioTracksCall call;
    call.c = cfg;
    call.tracks = reinterpret_cast<const AudioTrackEnt *>(slot->dev);
    call.blocks = reinterpret_cast<const AudioBlock *>(slot->dev + tab_bytes);
    call.hiss = hiss ? k->hiss : nullptr;
    call.pulses = buzz ? k->pulses : nullptr;
    call.nseg = nseg;
    call.ntracks = n;
    int lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    if (hiss) {
        audio_hiss_launch(reinterpret_cast<const AudioHissBlock *>(slot->dev + tab_bytes + blocks_bytes), (int)m, max_items, k->polys, k->hiss, st);
        lrc = stage_launched(v, nullptr, st, "k_audio_hiss");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    if (buzz) {
        const dim3 grid((unsigned)std::min<uint64_t>((max_frames + 255) / 256, 65535), (unsigned)std::min(n, 1024));
        hipLaunchKernelGGL(k_audio_track_pulses, grid, dim3(256), 0, st, cfg, call.tracks, n, k->pulses);
        lrc = stage_launched(v, nullptr, st, "k_audio_track_pulses");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_audio_track_segments, dim3((unsigned)((nseg + AUDIO_GROUPS - 1) / AUDIO_GROUPS)), dim3(64), 0, st, call, k->recs, L, W);
    lrc = stage_launched(v, nullptr, st, "k_audio_track_segments");
    if (lrc == NTSCSIM_OK) lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_audio_track_verify, dim3((unsigned)n), dim3(64), 0, st, call, k->recs, L, W, k->track_stats);
    lrc = stage_launched(v, slot, st, "k_audio_track_verify");
    return lrc == NTSCSIM_OK ? audio_mark(v, k, st) : lrc;
}

// what ntscsim_audio_bind() accepts
bool audio_params_ok(const ntscsim_audio_params &p)
{
    return !(p.channels < 1 || p.channels > 2 || p.passes != AUDIO_PASSES || p.rate <= 0 || !(p.lowpass_hz > 0) || !(p.highpass_hz > 0) ||
             p.vsync_lines <= 0 || p.hiss_level < 0 || p.hiss_level > 0x3FFFFFFF);
}

// What a mixed call checks before it looks at a sample pointer: the shape of the arguments and the sets that tracks
// name.  cfgs: the set table, one AudioCfg per distinct set in use, in order of first use; cfg_of_track[t]: track t's.
int audio_mixed_sets(const AudioStageState *k, const ntscsim_audio_params *sets, int n_sets, const ntscsim_audio_mixed_track *tracks, int n,
                     std::vector<AudioCfg> &cfgs, std::vector<int32_t> &cfg_of_track)
{
    if (n_sets < 0 || n < 0 || (n_sets > 0 && !sets) || (n > 0 && !tracks)) return NTSCSIM_E_ARG;
    for (int t = 0; t < n; t++) {
        const ntscsim_audio_mixed_track &tr = tracks[t];
        if (tr.set < -1 || tr.set >= n_sets || tr.n_blocks < 0 || (tr.n_blocks > 0 && !tr.blocks)) return NTSCSIM_E_ARG;
        if (tr.set >= 0 && sets[tr.set].struct_size != sizeof(ntscsim_audio_params)) return NTSCSIM_E_ARG;
    }
    std::vector<int32_t> at((size_t)n_sets + 1, -1);                            // at[set + 1]: its place in the table
    cfg_of_track.assign((size_t)n, 0);
    for (int t = 0; t < n; t++) {
        const int set = tracks[t].set;
        if (at[(size_t)set + 1] < 0) {
            if (set >= 0 && !audio_params_ok(sets[set])) return NTSCSIM_E_PARAM;
            at[(size_t)set + 1] = (int32_t)cfgs.size();
            cfgs.push_back(set < 0 ? k->cfg : audio_cfg_of(sets[set]));
        }
        cfg_of_track[(size_t)t] = at[(size_t)set + 1];
    }
    return NTSCSIM_OK;
}

// ntscsim_audio_mixed_tracks_device(): n independent streams, each with the cfg of its set, in one launch of each kernel
int audio_mixed(ntscsim_ctx *c, const std::vector<AudioCfg> &cfgs, const std::vector<int32_t> &cfg_of_track, const ntscsim_audio_mixed_track *tracks,
                int n, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    AudioStageState *k = *v.audio;
    // every track and descriptor checked before anything is enqueued or the rand() position moves
    std::vector<Span> srcs;
    std::vector<uintptr_t> states;
    size_t m = 0, mh = 0;                                                       // blocks that run the chain; those of them that draw
    for (int t = 0; t < n; t++) {
        const ntscsim_audio_mixed_track &tr = tracks[t];
        const AudioCfg &cfg = cfgs[(size_t)cfg_of_track[(size_t)t]];
        const size_t fbytes = (size_t)cfg.channels * sizeof(int16_t);
        if ((uintptr_t)tr.state & 7) return NTSCSIM_E_ARG;
        if (tr.state) states.push_back((uintptr_t)tr.state);
        for (int i = 0; i < tr.n_blocks; i++) {
            const ntscsim_audio_desc &d = tr.blocks[i];
            if (d.samples == 0) continue;
            if (!d.src || !d.dst || (((uintptr_t)d.src | (uintptr_t)d.dst) & 1)) return NTSCSIM_E_ARG;
            srcs.push_back(Span{(uintptr_t)d.src, (uintptr_t)d.src + (size_t)d.samples * fbytes});
            if (cfg.enabled) m++;
            if (audio_track_draws(cfg)) mh++;
        }
    }
    if (m > (size_t)INT32_MAX) return NTSCSIM_E_ARG;
    std::sort(states.begin(), states.end());
    for (size_t i = 1; i < states.size(); i++)
        if (states[i] - states[i - 1] < sizeof(AudioState)) return NTSCSIM_E_ARG;   // two tracks would share a state
    std::sort(srcs.begin(), srcs.end(), [](const Span &x, const Span &y) { return x.a < y.a; });
    std::vector<uintptr_t> reach(srcs.size());                                  // the furthest end among srcs[0..i]
    for (size_t i = 0; i < srcs.size(); i++) reach[i] = std::max(srcs[i].b, i ? reach[i - 1] : 0);
    for (int t = 0; t < n; t++) {
        const size_t fbytes = (size_t)cfgs[(size_t)cfg_of_track[(size_t)t]].channels * sizeof(int16_t);
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_audio_desc &d = tracks[t].blocks[i];
            if (d.samples == 0) continue;
            const uintptr_t a = (uintptr_t)d.dst, b = a + (size_t)d.samples * fbytes;
            const size_t at = (size_t)(std::lower_bound(srcs.begin(), srcs.end(), b, [](const Span &x, uintptr_t e) { return x.a < e; }) - srcs.begin());
            if (at > 0 && reach[at - 1] > a) return NTSCSIM_E_ARG;              // a warm-up reads input again, in any track
        }
    }
    STAGECHK(v, hipSetDevice(v.device));
    if (2 * (size_t)n > k->track_stats_cap) {
        int rc = k->slots.wait_all(v);                                          // launches in flight use what is replaced
        if (rc == NTSCSIM_OK) rc = audio_grow(v, k->track_stats, k->track_stats_cap, 2 * (size_t)n);
        if (rc != NTSCSIM_OK) return rc;
    }
    v.kernels->clear();
    audio_drop_marks(k);
    k->last_tracks = n;
    const size_t stats_bytes = (size_t)n * 2 * sizeof(uint64_t);
    const uint32_t L = k->plan_len ? k->plan_len : AUDIO_DEFAULT_SEG;
    // the rand() position moves at call time, whatever becomes of the launch: tracks in order, blocks in order; a copied
    // track is no call of the chain and leaves the position alone
    uint64_t pos = ntscsim_get_rng_pos(c);
    std::vector<uint64_t> block_pos;                                            // of the blocks that draw
    block_pos.reserve(mh);
    for (int t = 0; t < n; t++) {
        const AudioCfg &cfg = cfgs[(size_t)cfg_of_track[(size_t)t]];
        if (!cfg.enabled) continue;
        const bool draws = audio_track_draws(cfg);
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_audio_desc &d = tracks[t].blocks[i];
            if (d.rng_pos != NTSCSIM_RNG_AUTO) pos = d.rng_pos;
            if (d.samples && draws) block_pos.push_back(pos);
            if (draws) pos += (uint64_t)d.samples * (uint64_t)cfg.channels;
        }
    }
    ntscsim_set_rng_pos(c, pos);
    for (int t = 0; t < n; t++) {                                               // -nocomp tracks: the tool does not call the chain
        const AudioCfg &cfg = cfgs[(size_t)cfg_of_track[(size_t)t]];
        if (cfg.enabled) continue;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_audio_desc &d = tracks[t].blocks[i];
            if (d.samples)
                STAGECHK(v, hipMemcpyAsync(d.dst, d.src, (size_t)d.samples * (size_t)cfg.channels * sizeof(int16_t), hipMemcpyDeviceToDevice, st));
        }
    }
    if (m == 0) {
        if (n) STAGECHK(v, hipMemsetAsync(k->track_stats, 0, stats_bytes, st));
        return NTSCSIM_OK;
    }
    // records: the set table, the track table, the blocks that run the chain, the rand() windows of those that draw
    const size_t cfg_bytes = cfgs.size() * sizeof(AudioCfg), tab_bytes = (size_t)n * sizeof(AudioTrackEnt), blocks_bytes = m * sizeof(AudioBlock),
                 hb_bytes = mh * sizeof(AudioHissBlock);
    static_assert(sizeof(AudioCfg) % 8 == 0 && sizeof(AudioTrackEnt) % 8 == 0 && sizeof(AudioBlock) % 8 == 0, "the records follow each other");
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, cfg_bytes + tab_bytes + blocks_bytes + hb_bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    std::memcpy(slot->host, cfgs.data(), cfg_bytes);
    AudioTrackEnt *tab = reinterpret_cast<AudioTrackEnt *>(slot->host + cfg_bytes);
    AudioBlock *blocks = reinterpret_cast<AudioBlock *>(slot->host + cfg_bytes + tab_bytes);
    AudioHissBlock *hb = reinterpret_cast<AudioHissBlock *>(slot->host + cfg_bytes + tab_bytes + blocks_bytes);
    int o = 0;
    uint64_t total_before = 0;                                                  // = the plane of the track, as audio_mixed_layout() sets it
    for (int t = 0; t < n; t++) {
        AudioTrackEnt &e = tab[t];
        std::memset(&e, 0, sizeof(e));
        e.state = reinterpret_cast<AudioState *>(tracks[t].state);
        e.block0 = o;
        e.set = cfg_of_track[(size_t)t];
        if (cfgs[(size_t)e.set].enabled)
            for (int i = 0; i < tracks[t].n_blocks; i++) {
                const ntscsim_audio_desc &d = tracks[t].blocks[i];
                if (d.samples == 0) continue;
                blocks[o++] = AudioBlock{d.src, d.dst, total_before + e.frames, d.samples};   // first: in the plane
                e.frames += d.samples;
            }
        e.nblocks = o - e.block0;
        total_before += e.frames;
    }
    uint64_t hiss_items = 0, plane_frames = 0;
    const uint64_t nseg = audio_mixed_layout(tab, n, cfgs.data(), L, k->plan_warmup_set ? &k->plan_warmup : nullptr, &hiss_items, &plane_frames);
    uint64_t max_items = 0, max_frames = 0;
    bool buzz = false;
    {
        RandSeq seq(rand_state_origin());
        uint64_t seq_pos = UINT64_MAX;                                          // where seq stands; UINT64_MAX: nowhere
        size_t h = 0;
        for (int t = 0; t < n; t++) {
            const AudioTrackEnt &e = tab[t];
            const AudioCfg &cfg = cfgs[(size_t)e.set];
            if (audio_buzz_on(cfg) && e.frames) {
                buzz = true;
                max_frames = std::max(max_frames, e.frames);
            }
            if (!audio_track_draws(cfg)) continue;
            for (int b = e.block0; b < e.block0 + e.nblocks; b++, h++) {
                audio_hiss_window(hb[h], seq, seq_pos, block_pos[h], e.hiss0 + (blocks[b].first - e.plane) * cfg.channels, blocks[b].frames * cfg.channels,
                                  cfg.hiss_level);
                max_items = std::max(max_items, hb[h].items);
            }
        }
    }
    const bool hiss = hiss_items != 0;
    if ((hiss && hiss_items > k->hiss_cap) || (buzz && plane_frames > k->pulses_cap) || nseg > k->recs_cap) {
        int grc = k->slots.wait_all(v);                                         // launches in flight use what is replaced
        if (grc == NTSCSIM_OK && hiss) grc = audio_grow(v, k->hiss, k->hiss_cap, (size_t)hiss_items);
        if (grc == NTSCSIM_OK && buzz) grc = audio_grow(v, k->pulses, k->pulses_cap, (size_t)plane_frames);
        if (grc == NTSCSIM_OK) grc = audio_grow(v, k->recs, k->recs_cap, (size_t)nseg);
        if (grc != NTSCSIM_OK) return grc;
    }
    STAGECHK(v, hipMemcpyAsync(slot->dev, slot->host, cfg_bytes + tab_bytes + blocks_bytes + hb_bytes, hipMemcpyHostToDevice, st));
    AudioMixedCall call;
    call.cfgs = reinterpret_cast<const AudioCfg *>(slot->dev);
    call.tracks = reinterpret_cast<const AudioTrackEnt *>(slot->dev + cfg_bytes);
    call.blocks = reinterpret_cast<const AudioBlock *>(slot->dev + cfg_bytes + tab_bytes);
    call.hiss = hiss ? k->hiss : nullptr;
    call.pulses = buzz ? k->pulses : nullptr;
    call.nseg = nseg;
    call.ntracks = n;
    int lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    if (hiss) {
        audio_hiss_launch(reinterpret_cast<const AudioHissBlock *>(slot->dev + cfg_bytes + tab_bytes + blocks_bytes), (int)mh, max_items, k->polys, k->hiss, st);
        lrc = stage_launched(v, nullptr, st, "k_audio_hiss");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    if (buzz) {
        const dim3 grid((unsigned)std::min<uint64_t>((max_frames + 255) / 256, 65535), (unsigned)std::min(n, 1024));
        hipLaunchKernelGGL(k_audio_mixed_pulses, grid, dim3(256), 0, st, call.cfgs, call.tracks, n, k->pulses);
        lrc = stage_launched(v, nullptr, st, "k_audio_mixed_pulses");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_audio_mixed_segments, dim3((unsigned)((nseg + AUDIO_GROUPS - 1) / AUDIO_GROUPS)), dim3(64), 0, st, call, k->recs, L);
    lrc = stage_launched(v, nullptr, st, "k_audio_mixed_segments");
    if (lrc == NTSCSIM_OK) lrc = audio_mark(v, k, st);
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_audio_mixed_verify, dim3((unsigned)n), dim3(64), 0, st, call, k->recs, L, k->track_stats);
    lrc = stage_launched(v, slot, st, "k_audio_mixed_verify");
    return lrc == NTSCSIM_OK ? audio_mark(v, k, st) : lrc;
}

AudioStageState *audio_of(ntscsim_ctx *c) { return c ? *ctx_stage_view(c).audio : nullptr; }

} // namespace

extern "C" int ntscsim_audio_bind(ntscsim_ctx *c, const ntscsim_audio_params *p)
{
    if (!c || !p || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    if (!audio_params_ok(*p)) return NTSCSIM_E_PARAM;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    AudioStageState *k = *v.audio;
    if (!k) {
        k = new (std::nothrow) AudioStageState();
        if (!k) return NTSCSIM_E_NOMEM;
        *v.audio = k;
    }
    const int rc = k->slots.wait_all(v);                                        // launches in flight use the state
    if (rc != NTSCSIM_OK) return rc;
    if (!k->state) STAGECHK(v, hipMalloc((void **)&k->state, sizeof(AudioState)));
    if (!k->stats) STAGECHK(v, hipMalloc((void **)&k->stats, 2 * sizeof(uint64_t)));
    if (!k->polys) {
        const int prc = audio_hiss_polys(v, &k->polys);
        if (prc != NTSCSIM_OK) return prc;
    }
    STAGECHK(v, hipMemset(k->state, 0, sizeof(AudioState)));
    STAGECHK(v, hipMemset(k->stats, 0, 2 * sizeof(uint64_t)));
    k->prm = *p;
    k->cfg = audio_cfg_of(*p);
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_device(ntscsim_ctx *c, const ntscsim_audio_desc *descs, int n, void *hip_stream)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    if (!*v.audio) return NTSCSIM_E_ARG;                                        // ntscsim_audio_bind() first
    return audio_blocks(c, descs, n, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

extern "C" int ntscsim_audio_tracks_device(ntscsim_ctx *c, const ntscsim_audio_track *tracks, int n_tracks, void *hip_stream)
{
    if (!c || n_tracks < 0 || (n_tracks > 0 && !tracks)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    if (!*v.audio) return NTSCSIM_E_ARG;                                        // ntscsim_audio_bind() first
    return audio_tracks(c, tracks, n_tracks, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

extern "C" int ntscsim_audio_mixed_tracks_device(ntscsim_ctx *c, const ntscsim_audio_params *sets, int n_sets, const ntscsim_audio_mixed_track *tracks,
                                                 int n_tracks, void *hip_stream)
{
    AudioStageState *k = audio_of(c);
    if (!k) return NTSCSIM_E_ARG;                                               // ntscsim_audio_bind() first
    std::vector<AudioCfg> cfgs;
    std::vector<int32_t> cfg_of_track;
    const int rc = audio_mixed_sets(k, sets, n_sets, tracks, n_tracks, cfgs, cfg_of_track);
    if (rc != NTSCSIM_OK) return rc;
    return audio_mixed(c, cfgs, cfg_of_track, tracks, n_tracks, hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx_stage_view(c).stream);
}

// The host form: every block's samples and every state through the ctx's staging -- [sources | states | results] on
// both sides, so that one copy goes up and one comes down around ONE device call.
extern "C" int ntscsim_audio_mixed_tracks_host(ntscsim_ctx *c, const ntscsim_audio_params *sets, int n_sets, const ntscsim_audio_mixed_track *tracks,
                                               int n_tracks)
{
    AudioStageState *k = audio_of(c);
    if (!k) return NTSCSIM_E_ARG;
    std::vector<AudioCfg> cfgs;
    std::vector<int32_t> cfg_of_track;
    int rc = audio_mixed_sets(k, sets, n_sets, tracks, n_tracks, cfgs, cfg_of_track);
    if (rc != NTSCSIM_OK) return rc;
    size_t samples_bytes = 0, n_descs = 0, n_states = 0;
    for (int t = 0; t < n_tracks; t++) {
        const size_t fbytes = (size_t)cfgs[(size_t)cfg_of_track[(size_t)t]].channels * sizeof(int16_t);
        n_states += tracks[t].state != nullptr;
        n_descs += (size_t)tracks[t].n_blocks;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_audio_desc &d = tracks[t].blocks[i];
            if (d.samples && (!d.src || !d.dst)) return NTSCSIM_E_ARG;
            samples_bytes += (size_t)d.samples * fbytes;
        }
    }
    std::vector<uintptr_t> states;
    for (int t = 0; t < n_tracks; t++)
        if (tracks[t].state) states.push_back((uintptr_t)tracks[t].state);
    std::sort(states.begin(), states.end());
    for (size_t i = 1; i < states.size(); i++)
        if (states[i] - states[i - 1] < sizeof(AudioState)) return NTSCSIM_E_ARG;   // two tracks would share a state
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    const size_t src_bytes = (samples_bytes + 255) & ~(size_t)255, states_bytes = (n_states * sizeof(AudioState) + 255) & ~(size_t)255;
    const size_t whole = 2 * src_bytes + states_bytes;
    if (whole > k->frames.arena_cap || whole > k->frames.staging_cap) {
        rc = k->slots.wait_all(v);                                              // launches in flight may use the arena
        if (rc == NTSCSIM_OK) rc = k->frames.reserve(v, whole, whole);
        if (rc != NTSCSIM_OK) return rc;
    }
    unsigned char *stage = k->frames.staging, *arena = k->frames.arena;
    std::vector<ntscsim_audio_desc> descs(n_descs);
    std::vector<ntscsim_audio_mixed_track> dev((size_t)n_tracks);
    size_t at = 0, s_at = 0, d_at = 0;
    for (int t = 0; t < n_tracks; t++) {
        const size_t fbytes = (size_t)cfgs[(size_t)cfg_of_track[(size_t)t]].channels * sizeof(int16_t);
        dev[(size_t)t] = tracks[t];
        dev[(size_t)t].blocks = descs.data() + d_at;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            ntscsim_audio_desc &d = descs[d_at++];
            d = tracks[t].blocks[i];
            const size_t bytes = (size_t)d.samples * fbytes;
            if (!bytes) continue;
            std::memcpy(stage + at, tracks[t].blocks[i].src, bytes);
            d.src = reinterpret_cast<const int16_t *>(arena + at);
            d.dst = reinterpret_cast<int16_t *>(arena + src_bytes + states_bytes + at);
            at += bytes;
        }
        if (tracks[t].state) {
            std::memcpy(stage + src_bytes + s_at, tracks[t].state, sizeof(AudioState));
            dev[(size_t)t].state = reinterpret_cast<ntscsim_audio_state *>(arena + src_bytes + s_at);
            s_at += sizeof(AudioState);
        }
    }
    if (src_bytes + states_bytes) STAGECHK(v, hipMemcpyAsync(arena, stage, src_bytes + states_bytes, hipMemcpyHostToDevice, v.stream));
    rc = audio_mixed(c, cfgs, cfg_of_track, dev.data(), n_tracks, v.stream);
    if (rc != NTSCSIM_OK) return rc;
    if (src_bytes + states_bytes)
        STAGECHK(v, hipMemcpyAsync(stage + src_bytes, arena + src_bytes, states_bytes + src_bytes, hipMemcpyDeviceToHost, v.stream));
    STAGECHK(v, hipStreamSynchronize(v.stream));
    at = s_at = 0;
    for (int t = 0; t < n_tracks; t++) {
        const size_t fbytes = (size_t)cfgs[(size_t)cfg_of_track[(size_t)t]].channels * sizeof(int16_t);
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const size_t bytes = (size_t)tracks[t].blocks[i].samples * fbytes;
            if (!bytes) continue;
            std::memcpy(tracks[t].blocks[i].dst, stage + src_bytes + states_bytes + at, bytes);
            at += bytes;
        }
        if (tracks[t].state) {
            std::memcpy(tracks[t].state, stage + src_bytes + s_at, sizeof(AudioState));
            s_at += sizeof(AudioState);
        }
    }
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_host(ntscsim_ctx *c, int16_t *audio, uint32_t samples)
{
    AudioStageState *k = audio_of(c);
    if (!k || (samples && !audio)) return NTSCSIM_E_ARG;
    if (samples == 0) return NTSCSIM_OK;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    const size_t bytes = (size_t)samples * (size_t)k->cfg.channels * sizeof(int16_t), half = (bytes + 255) & ~(size_t)255;
    const int arc = k->frames.reserve(v, 2 * half, half);
    if (arc != NTSCSIM_OK) return arc;
    std::memcpy(k->frames.staging, audio, bytes);
    STAGECHK(v, hipMemcpyAsync(k->frames.arena, k->frames.staging, bytes, hipMemcpyHostToDevice, v.stream));
    ntscsim_audio_desc d;
    std::memset(&d, 0, sizeof(d));
    d.src = reinterpret_cast<const int16_t *>(k->frames.arena);
    d.dst = reinterpret_cast<int16_t *>(k->frames.arena + half);
    d.samples = samples;
    d.rng_pos = NTSCSIM_RNG_AUTO;
    const int rc = audio_blocks(c, &d, 1, v.stream);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpyAsync(k->frames.staging, k->frames.arena + half, bytes, hipMemcpyDeviceToHost, v.stream));
    STAGECHK(v, hipStreamSynchronize(v.stream));
    std::memcpy(audio, k->frames.staging, bytes);
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_reset(ntscsim_ctx *c)
{
    ntscsim_audio_state s;
    std::memset(&s, 0, sizeof(s));
    return ntscsim_audio_set_state(c, &s);
}

static_assert(sizeof(ntscsim_audio_state) == sizeof(AudioState), "ntscsim_audio_state is AudioState");

extern "C" int ntscsim_audio_get_state(ntscsim_ctx *c, ntscsim_audio_state *out)
{
    AudioStageState *k = audio_of(c);
    if (!k || !out) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = audio_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpy(out, k->state, sizeof(AudioState), hipMemcpyDeviceToHost));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_set_state(ntscsim_ctx *c, const ntscsim_audio_state *in)
{
    AudioStageState *k = audio_of(c);
    if (!k || !in) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = audio_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpy(k->state, in, sizeof(AudioState), hipMemcpyHostToDevice));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_debug_set_plan(ntscsim_ctx *c, uint32_t seg_len, uint32_t warmup)
{
    AudioStageState *k = audio_of(c);
    if (!k) return NTSCSIM_E_ARG;
    k->plan_len = seg_len;
    k->plan_warmup = warmup;
    k->plan_warmup_set = seg_len != 0 || warmup != 0;                           // (0, 0) restores both defaults; (L, 0) is W = 0
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_debug_stats(ntscsim_ctx *c, ntscsim_audio_stats *out)
{
    AudioStageState *k = audio_of(c);
    if (!k || !out) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = audio_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    uint64_t s[2];
    STAGECHK(v, hipMemcpy(s, k->stats, sizeof(s), hipMemcpyDeviceToHost));
    out->segments = s[0];
    out->repaired = s[1];
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_debug_track_stats(ntscsim_ctx *c, ntscsim_audio_stats *out, int n_tracks)
{
    AudioStageState *k = audio_of(c);
    if (!k || n_tracks < 0 || n_tracks > k->last_tracks || (n_tracks && !out)) return NTSCSIM_E_ARG;
    if (n_tracks == 0) return NTSCSIM_OK;
    CtxStageView v = ctx_stage_view(c);
    const int rc = audio_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    static_assert(sizeof(ntscsim_audio_stats) == 2 * sizeof(uint64_t), "k_audio_track_verify writes ntscsim_audio_stats");
    STAGECHK(v, hipMemcpy(out, k->track_stats, (size_t)n_tracks * sizeof(ntscsim_audio_stats), hipMemcpyDeviceToHost));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_debug_pulses(ntscsim_ctx *c, uint64_t count0, uint32_t n, uint8_t *out)
{
    AudioStageState *k = audio_of(c);
    if (!k || (n && !out)) return NTSCSIM_E_ARG;
    if (n == 0) return NTSCSIM_OK;
    CtxStageView v = ctx_stage_view(c);
    const int rc = audio_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    uint8_t *dev = nullptr;
    STAGECHK(v, hipMalloc((void **)&dev, n));
    hipLaunchKernelGGL(k_audio_pulses, dim3((n + 255u) / 256u), dim3(256), 0, v.stream, k->cfg, (const AudioState *)nullptr, count0, (uint64_t)n, dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, dev, n, hipMemcpyDeviceToHost, v.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(v.stream);
    (void)hipFree(dev);
    STAGECHK(v, e);
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_debug_time_kernels(ntscsim_ctx *c, int on)
{
    AudioStageState *k = audio_of(c);
    if (!k) return NTSCSIM_E_ARG;
    k->timing = on != 0;
    if (!k->timing) audio_drop_marks(k);
    return NTSCSIM_OK;
}

extern "C" int ntscsim_audio_debug_kernel_ms(ntscsim_ctx *c, float out_ms[3])
{
    AudioStageState *k = audio_of(c);
    if (!k || !out_ms || k->marks.size() != 4) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = audio_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    for (int i = 0; i < 3; i++) STAGECHK(v, hipEventElapsedTime(&out_ms[i], k->marks[(size_t)i], k->marks[(size_t)i + 1]));
    return NTSCSIM_OK;
}
