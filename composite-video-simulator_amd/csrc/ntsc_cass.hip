// ntsc_cass.hip -- ffmpeg_cassette's tape chain as a device stage (include/ntscsim.h: ntscsim_cass_*).
// The arithmetic is cass_chain.hpp; this file is its device form.
//
// FRONT (band-pass, pre-emphasis, clip, hiss) is a serial recurrence and runs as ntsc_audio.hip's chain does: segments
// that start one warm-up early from a zero state, each run by a GROUP OF 17 ADJACENT LANES, one lane per stage, three
// groups to a wavefront; k_cass_front_verify makes the result independent of the speculation.  It leaves DOUBLES in a
// scratch plane x.  The FIR has no feedback: k_cass_conv runs it over all frames at once from LDS tiles of x and never
// sits on the beat of the lane pipeline.  BACK (the two shared de-emphasis poles, pack, downmix) is a recurrence of two
// values: one lane per segment, a short warm-up, k_cass_back_verify behind it.  head_tilt_final of every frame comes
// from the host (libm sin), never from the device.
// ntscsim_cass_tracks_device() runs many such streams side by side through a track table (k_cass_track_*);
// ntscsim_cass_mixed_tracks_device() does so with parameters per track: a set table in the call's records, sections of
// the x plane of every track's own taps, and a table of sines in place of head_tilt_final (k_cass_mixed_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "audio_hiss.hpp"
#include "cass_chain.hpp"
#include "glibc_rand.hpp"
#include "ntsc_frames.hpp"
#include "ntsc_stage.hpp"
#include "ntscsim.h"

namespace ntscsim {

constexpr int CASS_LANES = 17;           // stages of the front = lanes of a group
constexpr int CASS_GROUPS = 3;           // groups of a wavefront
constexpr int CASS_RING = 3 * CASS_LANES;
constexpr int CASS_TILE = 256;           // frames of a workgroup of k_cass_conv
constexpr int CASS_STAT_VALUES = 3;

struct CassBlock {                       // one descriptor; first: its first frame in the call
    const int16_t *src;
    int16_t *dst;
    uint64_t first, frames;
};
struct CassFrontRec {
    CassFront at_start, at_end;          // at the segment's first own frame, behind its last
};
struct CassBackRec {
    CassBack at_start, at_end;
};

struct CassCall {                        // what every lane of a call reads
    CassCfg c;
    const CassBlock *blocks;
    const int32_t *hiss;                 // per channel-sample of the call, NULL without hiss
    double *xs;                          // taps - 1 frames of history, then x of the call's frames: [frame][channel]
    uint64_t total;                      // frames of the call
    int nblocks;
};

// the block that holds frame f (f < total); b only moves forward
__device__ __forceinline__ void cass_seek(const CassCall &k, int &b, uint64_t f)
{
    while (b + 1 < k.nblocks && f >= k.blocks[b].first + k.blocks[b].frames) b++;
}
// the same from nowhere: the last block whose first frame is <= f (blocks are in order and none is empty)
__device__ __forceinline__ int cass_find(const CassCall &k, uint64_t f)
{
    int lo = 0, hi = k.nblocks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (k.blocks[mid].first <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------- the front's lanes
enum CassRole { CR_LOAD, CR_FILTER, CR_PASS, CR_CLIP, CR_STORE, CR_IDLE };
enum CassRule { CO_PREV, CO_HIGH, CO_EMPH };

struct CassLane {
    int role, rule;
    int slot0, slot1;                    // values of the front state this lane owns (-1: none)
    double alpha;
};

__device__ __forceinline__ CassLane cass_lane(const CassCfg &c, int r)
{
    CassLane l;
    l.role = CR_IDLE;
    l.rule = CO_PREV;
    l.slot0 = l.slot1 = -1;
    l.alpha = 0;
    if (r == 0) l.role = CR_LOAD;
    else if (r <= 6) { l.role = CR_FILTER; l.slot0 = r - 1; l.slot1 = 12 + r - 1; l.alpha = c.a_lo; }
    else if (r <= 12) { l.role = CR_FILTER; l.rule = CO_HIGH; l.slot0 = r - 1; l.slot1 = 12 + r - 1; l.alpha = c.a_hi; }
    else if (r <= 14) { l.role = c.pre ? CR_FILTER : CR_PASS; l.rule = CO_EMPH; l.slot0 = c.pre ? 24 + r - 13 : -1; l.alpha = c.a_pre; }
    else if (r == 15) l.role = CR_CLIP;
    else if (r == 16) l.role = CR_STORE;
    return l;
}

// Frames [first, first + warm + own) of the call through the 17 lanes of one group; r: this lane's place in its group
// (>= CASS_LANES or !live: the lane only takes part in the hand-offs).  init[]: the state the run starts from.  x of the
// last `own` frames is stored.  at_start (may be NULL) / at_end receive the values this lane owns, at the first own
// frame and behind the last; their other values and their counts are the caller's.
// ring: CASS_RING entries of the group for each of the two prefetched inputs -- every lane fetches, one period of 17
// steps ahead, what channel-sample (period * 17 + r) needs (input, hiss numerator), so that no stage waits for memory
// inside a step.
__device__ void cass_run_lanes(const CassCall &k, int r, bool live, uint64_t first, uint64_t warm, uint64_t own, const double *init, CassFront *at_start,
                               CassFront *at_end, int32_t *ring_in, int32_t *ring_hiss)
{
    const CassCfg &c = k.c;
    const CassLane L = cass_lane(c, live ? r : 99);
    const uint64_t N = live ? (warm + own) * 2 : 0;                             // channel-samples of the run
    const uint64_t warm_items = warm * 2;
    double st0 = L.slot0 >= 0 ? init[L.slot0] : 0.0, st1 = L.slot1 >= 0 ? init[L.slot1] : 0.0;
    const bool hiss_on = c.hiss_level != 0;
    double *const xs = k.xs + (uint64_t)(c.taps - 1) * 2;                       // x of frame 0

    // prefetch cursor: channel-sample pf of the run, period by period
    uint64_t pf = (uint64_t)r;
    int pf_block = 0;
    int32_t pf_in = 0, pf_hiss = 0;
    const auto fetch = [&]() {
        pf_in = pf_hiss = 0;
        if (r < CASS_LANES && pf < N) {
            const uint64_t f = first + (pf >> 1);
            const int cc = (int)(pf & 1);
            cass_seek(k, pf_block, f);
            pf_in = k.blocks[pf_block].src[(f - k.blocks[pf_block].first) * 2 + cc];
            if (hiss_on) pf_hiss = k.hiss[f * 2 + cc];
        }
    };
    int pslot = r;                                                             // ring entry of the period being fetched
    fetch();
    if (r < CASS_LANES) { ring_in[pslot] = pf_in; ring_hiss[pslot] = pf_hiss; }
    pf += CASS_LANES;
    pslot += CASS_LANES;
    fetch();

    double y = 0.0;
    int64_t n = -(int64_t)r;                                                   // channel-sample of this lane at step t
    int slot = 0;                                                              // n % CASS_RING while n >= 0
    int chn = 0;
    uint64_t frame = first;
    int tp = 0;                                                                // t % CASS_LANES
    const uint64_t steps = N ? N + CASS_LANES : 0;
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
            case CR_LOAD: y = (double)ring_in[slot] / 32768; break;
            case CR_FILTER: {
                const double p = audio_pole(*prev, x, L.alpha);
                const double d = x - p;
                y = L.rule == CO_PREV ? p : (L.rule == CO_HIGH ? d : x + d);
                break;
            }
            case CR_PASS: y = x; break;
            case CR_CLIP: {
                double s = x;
                if (s > 1.0) s = 1.0;
                else if (s < -1.0) s = -1.0;
                if (hiss_on) s += ((double)ring_hiss[slot]) / 20000;
                y = s;
                break;
            }
            case CR_STORE:
                if ((uint64_t)n >= warm_items) xs[frame * 2 + chn] = x;        // frame < total: inside the plane
                break;
            default: break;
            }
        }
        if (n >= 0) {
            slot = slot == CASS_RING - 1 ? 0 : slot + 1;
            if (++chn == 2) { chn = 0; frame++; }
        }
        n++;
        if (++tp == CASS_LANES) {                                              // a period ends: publish the next, fetch the one after
            tp = 0;
            __syncthreads();
            if (r < CASS_LANES) { ring_in[pslot] = pf_in; ring_hiss[pslot] = pf_hiss; }
            pf += CASS_LANES;
            pslot = pslot >= 2 * CASS_LANES ? pslot - 2 * CASS_LANES : pslot + CASS_LANES;
            fetch();
            __syncthreads();
        }
    }
    if (N) {
        if (L.slot0 >= 0) at_end->v[L.slot0] = st0;
        if (L.slot1 >= 0) at_end->v[L.slot1] = st1;
    }
}

__device__ __forceinline__ bool cass_front_live(const CassCfg &c, int i) { return i < 24 || c.pre; }

// One wavefront per workgroup, three segments per wavefront.
__global__ __launch_bounds__(64) void k_cass_front(CassCall k, const CassState *__restrict__ carried, CassFrontRec *__restrict__ recs, uint32_t seg_len,
                                                   uint32_t warmup)
{
    __shared__ int32_t ring[CASS_GROUPS + 1][2][CASS_RING];
    __shared__ double init[CASS_GROUPS + 1][CASS_FRONT_VALUES];
    const int lane = (int)threadIdx.x, g = lane / CASS_LANES, r = lane - g * CASS_LANES;
    const uint64_t nseg = audio_seg_count(k.total, seg_len);
    const uint64_t j = (uint64_t)blockIdx.x * CASS_GROUPS + (uint64_t)g;
    const bool live = g < CASS_GROUPS && j < nseg;
    AudioSeg s{0, 0, 0};
    if (live) {
        s = audio_seg(k.total, seg_len, warmup, j);
        const bool spec = s.run_start != 0;
        for (int i = r; i < CASS_FRONT_VALUES; i += CASS_LANES) {
            const double v = spec && cass_front_live(k.c, i) ? 0.0 : carried->front.v[i];
            init[g][i] = v;
            recs[j].at_start.v[i] = v;
            recs[j].at_end.v[i] = v;
        }
        if (r == 0) {
            recs[j].at_start.count = carried->front.count + s.start;
            recs[j].at_end.count = carried->front.count + s.start + s.len;
        }
    }
    __syncthreads();
    cass_run_lanes(k, r, live, s.run_start, s.start - s.run_start, s.len, init[g], live ? &recs[j].at_start : nullptr, live ? &recs[j].at_end : nullptr,
                   ring[g][0], ring[g][1]);
}

// One wavefront.  truth: the state behind the last verified segment.  It also lays the carried history in front of the
// plane, where k_cass_conv reads it as the frames before the call's first.
__global__ __launch_bounds__(64) void k_cass_front_verify(CassCall k, CassState *__restrict__ carried, const CassFrontRec *__restrict__ recs, uint32_t seg_len,
                                                          uint32_t warmup, uint64_t *__restrict__ stats)
{
    __shared__ int32_t ring[2][CASS_RING];
    __shared__ CassFront truth;
    __shared__ double init[CASS_FRONT_VALUES];
    const int lane = (int)threadIdx.x;
    const uint64_t nseg = audio_seg_count(k.total, seg_len);
    for (int i = lane; i < (k.c.taps - 1) * 2; i += 64) k.xs[i] = carried->hist[i >> 1][i & 1];
    if (lane < CASS_FRONT_VALUES) truth.v[lane] = carried->front.v[lane];
    if (lane == CASS_FRONT_VALUES) truth.count = carried->front.count;
    __syncthreads();
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        bool same = true;
        if (lane < CASS_FRONT_VALUES) same = __double_as_longlong(recs[j].at_start.v[lane]) == __double_as_longlong(truth.v[lane]);
        if (lane == CASS_FRONT_VALUES) same = recs[j].at_start.count == truth.count;
        const bool ok = __all(same);
        __syncthreads();
        if (ok) {
            if (lane < CASS_FRONT_VALUES) truth.v[lane] = recs[j].at_end.v[lane];
            if (lane == CASS_FRONT_VALUES) truth.count = recs[j].at_end.count;
        } else {
            const AudioSeg s = audio_seg(k.total, seg_len, warmup, j);
            if (lane < CASS_FRONT_VALUES) init[lane] = truth.v[lane];
            __syncthreads();
            cass_run_lanes(k, lane, lane < CASS_LANES, s.start, 0, s.len, init, nullptr, &truth, ring[0], ring[1]);
            if (lane == 0) truth.count += s.len;
            repaired++;
        }
        __syncthreads();
    }
    if (lane < CASS_FRONT_VALUES) carried->front.v[lane] = truth.v[lane];
    if (lane == CASS_FRONT_VALUES) carried->front.count = truth.count;
    if (lane == 0) { stats[0] = nseg; stats[1] = repaired; }
}

// ---------------------------------------------------------------------------------------- the FIR
// A workgroup: CASS_TILE frames.  Their x and the taps - 1 frames in front of them go to LDS, a plane per channel; lane t
// computes the taps of its frame from tf[] and sums in ascending order (cass_conv<true>: the taps that are +0 are left
// out, which changes no bit).  rs == NULL (no de-emphasis): pack, downmix, store the samples; otherwise store r.
// Workgroup 0 also makes the call's last taps - 1 values of x the carried history: nothing in this kernel reads that.
__global__ __launch_bounds__(CASS_TILE) void k_cass_conv(CassCall k, const double *__restrict__ tf, CassState *__restrict__ carried, double *__restrict__ rs)
{
    __shared__ double tile[2][CASS_TILE + CASS_HIST];
    const int t = (int)threadIdx.x, taps = k.c.taps;
    const uint64_t tile0 = (uint64_t)blockIdx.x * CASS_TILE;
    const int own = (int)(k.total - tile0 < CASS_TILE ? k.total - tile0 : CASS_TILE);
    const double *src = k.xs + tile0 * 2;                                       // plane entry tile0 is frame tile0 - (taps - 1)
    for (int i = t; i < (own + taps - 1) * 2; i += CASS_TILE) tile[i & 1][i >> 1] = src[i];
    __syncthreads();
    if (t < own) {
        const uint64_t f = tile0 + (uint64_t)t;
        const double h = tf[f];
        const double r0 = cass_conv<true>(taps, h, 0, &tile[0][t], 1);
        const double r1 = cass_conv<true>(taps, h, 1, &tile[1][t], 1);
        if (rs) {
            rs[f * 2] = r0;
            rs[f * 2 + 1] = r1;
        } else {
            int16_t o0 = audio_pack(r0), o1 = audio_pack(r1);
            cass_downmix(k.c, o0, o1);
            const CassBlock &b = k.blocks[cass_find(k, f)];
            int16_t *d = b.dst + (f - b.first) * 2;
            d[0] = o0;
            d[1] = o1;
        }
    }
    if (blockIdx.x == 0)
        for (int i = t; i < (taps - 1) * 2; i += CASS_TILE) carried->hist[i >> 1][i & 1] = k.xs[k.total * 2 + (uint64_t)i];
}

// ---------------------------------------------------------------------------------------- the back
// frames [first, first + n) from b; store: write the samples
__device__ void cass_back_run(const CassCall &k, CassBack &b, const double *__restrict__ rs, uint64_t first, uint64_t n, bool store)
{
    if (n == 0) return;
    int blk = store ? cass_find(k, first) : 0;
    double a0 = rs[first * 2], a1 = rs[first * 2 + 1];
    for (uint64_t f = first; f < first + n; f++) {
        const double r0 = a0, r1 = a1;
        if (f + 1 < first + n) { a0 = rs[(f + 1) * 2]; a1 = rs[(f + 1) * 2 + 1]; }   // the next frame's load is under way
        int16_t o0 = cass_back_sample(k.c, b, r0);
        int16_t o1 = cass_back_sample(k.c, b, r1);
        if (store) {
            cass_downmix(k.c, o0, o1);
            cass_seek(k, blk, f);
            int16_t *d = k.blocks[blk].dst + (f - k.blocks[blk].first) * 2;
            d[0] = o0;
            d[1] = o1;
        }
    }
}

// one lane per segment
__global__ __launch_bounds__(64) void k_cass_back(CassCall k, const double *__restrict__ rs, const CassState *__restrict__ carried, CassBackRec *__restrict__ recs,
                                                  uint32_t seg_len, uint32_t warmup)
{
    const uint64_t nseg = audio_seg_count(k.total, seg_len);
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nseg) return;
    const AudioSeg s = audio_seg(k.total, seg_len, warmup, j);
    CassBack b = carried->back;
    if (s.run_start != 0) b.post[0] = b.post[1] = 0;
    cass_back_run(k, b, rs, s.run_start, s.start - s.run_start, false);
    recs[j].at_start = b;
    cass_back_run(k, b, rs, s.start, s.len, true);
    recs[j].at_end = b;
}

// one lane: the ordered walk
__global__ __launch_bounds__(64) void k_cass_back_verify(CassCall k, const double *__restrict__ rs, CassState *__restrict__ carried,
                                                         const CassBackRec *__restrict__ recs, uint32_t seg_len, uint32_t warmup, uint64_t *__restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t nseg = audio_seg_count(k.total, seg_len);
    CassBack truth = carried->back;
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        const CassBackRec rec = recs[j];
        if (cass_back_same(rec.at_start, truth)) {
            truth = rec.at_end;
        } else {
            const AudioSeg s = audio_seg(k.total, seg_len, warmup, j);
            cass_back_run(k, truth, rs, s.start, s.len, true);
            repaired++;
        }
    }
    carried->back = truth;
    stats[2] = repaired;
}

// ---------------------------------------------------------------------------------------- many tracks
// ntscsim_cass_tracks_device(): independent streams side by side (the track table of cass_chain.hpp).  The kernels above
// stay the single stream's; these hand the same cass_run_lanes / cass_back_run a track's VIEW.  The tracks are laid into
// one frame numbering, the PLANE (track t owns frames [plane_t, plane_t + frames_t) of it): the hiss and r scratch and
// the blocks' `first` are indexed by it.  The x plane is not: every track has a section of its own there, its taps - 1
// history frames in front of its frames, so a view's xs is shifted until the plane's numbering lands in that section.
static_assert(CASS_TILE == (int)CASS_TILE_FRAMES, "the tiles of the track table are k_cass_track_conv's");

struct CassTracksCall {
    CassCfg c;
    const CassTrackEnt *tracks;
    const CassBlock *blocks;             // of all tracks, `first` in the plane
    const int32_t *hiss;                 // per channel-sample of the plane, NULL without hiss
    double *xs;                          // the tracks' sections
    uint64_t nseg;                       // segments of the call
    int ntracks;
};

__device__ __forceinline__ CassCall cass_track_view(const CassTracksCall &k, const CassTrackEnt &e)
{
    CassCall v;
    v.c = k.c;
    v.blocks = k.blocks + e.block0;                                             // cass_seek and cass_find stay inside the track
    v.hiss = k.hiss;
    v.xs = k.xs + ((int64_t)e.xs - (int64_t)e.plane) * 2;                       // plane frame plane_t + f: entry taps - 1 + f of the section
    v.total = e.plane + e.frames;                                               // where the track ends in the plane
    v.nblocks = e.nblocks;
    return v;
}

// One wavefront per workgroup; group g of workgroup b takes call-wide segment 3 b + g, whatever track it belongs to.
__global__ __launch_bounds__(64) void k_cass_track_front(CassTracksCall k, CassFrontRec *__restrict__ recs, uint32_t seg_len, uint32_t warmup)
{
    __shared__ int32_t ring[CASS_GROUPS + 1][2][CASS_RING];
    __shared__ double init[CASS_GROUPS + 1][CASS_FRONT_VALUES];
    const int lane = (int)threadIdx.x, g = lane / CASS_LANES, r = lane - g * CASS_LANES;
    const uint64_t j = (uint64_t)blockIdx.x * CASS_GROUPS + (uint64_t)g;
    const bool live = g < CASS_GROUPS && j < k.nseg;
    CassTrackEnt e{0, 0, 0, 0, 0, 0, 0, nullptr, 0, 0};
    AudioSeg s{0, 0, 0};
    if (live) {
        e = k.tracks[cass_track_of_seg(k.tracks, k.ntracks, j)];
        s = audio_seg(e.frames, seg_len, warmup, j - e.seg0);                    // clamps at frame 0 of this track
        const bool spec = s.run_start != 0;
        for (int i = r; i < CASS_FRONT_VALUES; i += CASS_LANES) {
            const double v = (spec && cass_front_live(k.c, i)) || !e.state ? 0.0 : e.state->front.v[i];
            init[g][i] = v;
            recs[j].at_start.v[i] = v;
            recs[j].at_end.v[i] = v;
        }
        if (r == 0) {
            recs[j].at_start.count = e.count + s.start;                         // the table's count, not the state's
            recs[j].at_end.count = e.count + s.start + s.len;
        }
    }
    __syncthreads();
    const CassCall view = cass_track_view(k, e);
    cass_run_lanes(view, r, live, e.plane + s.run_start, s.start - s.run_start, s.len, init[g], live ? &recs[j].at_start : nullptr,
                   live ? &recs[j].at_end : nullptr, ring[g][0], ring[g][1]);
}

// One workgroup (one wavefront) per track: the walk of k_cass_front_verify over that track's records, from that track's
// true state, behind laying that track's carried history in front of its section.  A track without frames is left alone.
__global__ __launch_bounds__(64) void k_cass_track_front_verify(CassTracksCall k, const CassFrontRec *__restrict__ recs, uint32_t seg_len, uint32_t warmup,
                                                                uint64_t *__restrict__ stats)
{
    __shared__ int32_t ring[2][CASS_RING];
    __shared__ CassFront truth;
    __shared__ double init[CASS_FRONT_VALUES];
    const int lane = (int)threadIdx.x;
    const CassTrackEnt e = k.tracks[blockIdx.x];
    if (e.frames == 0) return;
    const CassCall view = cass_track_view(k, e);
    const uint64_t nseg = audio_seg_count(e.frames, seg_len);
    recs += e.seg0;
    double *const sec = k.xs + e.xs * 2;
    for (int i = lane; i < (k.c.taps - 1) * 2; i += 64) sec[i] = e.state ? e.state->hist[i >> 1][i & 1] : 0.0;
    if (lane < CASS_FRONT_VALUES) truth.v[lane] = e.state ? e.state->front.v[lane] : 0.0;
    if (lane == CASS_FRONT_VALUES) truth.count = e.count;
    __syncthreads();
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        bool same = true;
        if (lane < CASS_FRONT_VALUES) same = __double_as_longlong(recs[j].at_start.v[lane]) == __double_as_longlong(truth.v[lane]);
        if (lane == CASS_FRONT_VALUES) same = recs[j].at_start.count == truth.count;
        const bool ok = __all(same);
        __syncthreads();
        if (ok) {
            if (lane < CASS_FRONT_VALUES) truth.v[lane] = recs[j].at_end.v[lane];
            if (lane == CASS_FRONT_VALUES) truth.count = recs[j].at_end.count;
        } else {
            const AudioSeg s = audio_seg(e.frames, seg_len, warmup, j);
            if (lane < CASS_FRONT_VALUES) init[lane] = truth.v[lane];
            __syncthreads();
            cass_run_lanes(view, lane, lane < CASS_LANES, e.plane + s.start, 0, s.len, init, nullptr, &truth, ring[0], ring[1]);
            if (lane == 0) truth.count += s.len;
            repaired++;
        }
        __syncthreads();
    }
    if (e.state && lane < CASS_FRONT_VALUES) e.state->front.v[lane] = truth.v[lane];
    if (lane == 0) stats[CASS_STAT_VALUES * (uint64_t)blockIdx.x + 1] = repaired;
}

// what the last kernel of a track leaves behind the filter values: the count, the taps, the segments
__device__ __forceinline__ void cass_track_close(const CassCfg &c, const CassTrackEnt &e, uint32_t seg_len, uint64_t *__restrict__ stats, uint64_t t)
{
    if (e.state) {
        e.state->front.count = e.count + e.frames;
        e.state->taps = (uint32_t)c.taps;
    }
    stats[CASS_STAT_VALUES * t] = audio_seg_count(e.frames, seg_len);
}

// One workgroup per call-wide tile, found through the track table: a tile never crosses a track, and the taps - 1
// frames in front of a track's first tile are that track's history.  The tilt is read through the track's offset in the
// table.  The first tile of a track also makes the last taps - 1 entries of the section the track's history -- for a track
// shorter than that, part of them are the old history that k_cass_track_front_verify laid there -- and, when no back
// follows, closes the track.
__global__ __launch_bounds__(CASS_TILE) void k_cass_track_conv(CassTracksCall k, const double *__restrict__ tf, double *__restrict__ rs, uint32_t seg_len,
                                                               uint64_t *__restrict__ stats)
{
    __shared__ double tile[2][CASS_TILE + CASS_HIST];
    const int t = (int)threadIdx.x, taps = k.c.taps;
    const int tr = cass_track_of_tile(k.tracks, k.ntracks, (uint64_t)blockIdx.x);
    const CassTrackEnt e = k.tracks[tr];
    const uint64_t tile0 = ((uint64_t)blockIdx.x - e.tile0) * CASS_TILE;        // in the track
    const int own = (int)(e.frames - tile0 < CASS_TILE ? e.frames - tile0 : CASS_TILE);
    const double *sec = k.xs + e.xs * 2;
    const double *src = sec + tile0 * 2;                                        // section entry tile0 is frame tile0 - (taps - 1)
    for (int i = t; i < (own + taps - 1) * 2; i += CASS_TILE) tile[i & 1][i >> 1] = src[i];
    __syncthreads();
    if (t < own) {
        const uint64_t f = tile0 + (uint64_t)t;
        const double h = tf[e.tilt + f];
        const double r0 = cass_conv<true>(taps, h, 0, &tile[0][t], 1);
        const double r1 = cass_conv<true>(taps, h, 1, &tile[1][t], 1);
        if (rs) {
            rs[(e.plane + f) * 2] = r0;
            rs[(e.plane + f) * 2 + 1] = r1;
        } else {
            int16_t o0 = audio_pack(r0), o1 = audio_pack(r1);
            cass_downmix(k.c, o0, o1);
            const CassCall view = cass_track_view(k, e);
            const CassBlock &b = view.blocks[cass_find(view, e.plane + f)];
            int16_t *d = b.dst + (e.plane + f - b.first) * 2;
            d[0] = o0;
            d[1] = o1;
        }
    }
    if (tile0 == 0) {
        if (e.state)
            for (int i = t; i < (taps - 1) * 2; i += CASS_TILE) e.state->hist[i >> 1][i & 1] = sec[e.frames * 2 + (uint64_t)i];
        if (!rs && t == 0) cass_track_close(k.c, e, seg_len, stats, (uint64_t)tr);
    }
}

// one lane per call-wide segment
__global__ __launch_bounds__(64) void k_cass_track_back(CassTracksCall k, const double *__restrict__ rs, CassBackRec *__restrict__ recs, uint32_t seg_len,
                                                        uint32_t warmup)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k.nseg) return;
    const CassTrackEnt e = k.tracks[cass_track_of_seg(k.tracks, k.ntracks, j)];
    const CassCall view = cass_track_view(k, e);
    const AudioSeg s = audio_seg(e.frames, seg_len, warmup, j - e.seg0);
    CassBack b{{0.0, 0.0}};
    if (e.state && s.run_start == 0) b = e.state->back;
    cass_back_run(view, b, rs, e.plane + s.run_start, s.start - s.run_start, false);
    recs[j].at_start = b;
    cass_back_run(view, b, rs, e.plane + s.start, s.len, true);
    recs[j].at_end = b;
}

// one lane per track: the ordered walk of k_cass_back_verify over that track's records; it closes the track
__global__ __launch_bounds__(64) void k_cass_track_back_verify(CassTracksCall k, const double *__restrict__ rs, const CassBackRec *__restrict__ recs,
                                                               uint32_t seg_len, uint32_t warmup, uint64_t *__restrict__ stats)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)k.ntracks) return;
    const CassTrackEnt e = k.tracks[t];
    if (e.frames == 0) return;
    const CassCall view = cass_track_view(k, e);
    const uint64_t nseg = audio_seg_count(e.frames, seg_len);
    recs += e.seg0;
    CassBack truth{{0.0, 0.0}};
    if (e.state) truth = e.state->back;
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        const CassBackRec rec = recs[j];
        if (cass_back_same(rec.at_start, truth)) {
            truth = rec.at_end;
        } else {
            const AudioSeg s = audio_seg(e.frames, seg_len, warmup, j);
            cass_back_run(view, truth, rs, e.plane + s.start, s.len, true);
            repaired++;
        }
    }
    if (e.state) e.state->back = truth;
    stats[CASS_STAT_VALUES * t + 2] = repaired;
    cass_track_close(k.c, e, seg_len, stats, t);
}

// ---------------------------------------------------------------------------------------- parameters per track
// ntscsim_cass_mixed_tracks_device(): a tracks call whose tracks each name a cfg of a SET TABLE (device records of the
// call, cass_chain.hpp).  The kernels above stay the uniform calls'; these hand the same cass_run_lanes / cass_back_run
// a view whose cfg is the TRACK's.  A lane of the front loads its track's cfg once, in front of the run, and keeps of
// it what its stage reads -- its alpha, whether its stage filters, the hiss flag, the offset of frame 0 in its track's
// section -- so the three groups of a wavefront may serve three tracks on three sets and no step loads from the table.
// The FIR's table holds sines, not head_tilt_final: cass_tilt_of_sin() of the track's cfg makes the tilt per frame.
struct CassMixedCall {
    const CassCfg *cfgs;                 // the set table
    const CassMixedEnt *tracks;
    const CassBlock *blocks;             // of all tracks, `first` in the plane
    const int32_t *hiss;                 // per channel-sample of the plane (written for the tracks that draw), NULL if none does
    double *xs;                          // the tracks' sections: taps_t - 1 history frames, then the frames of track t
    uint64_t nseg;                       // segments of the call
    int ntracks;
};

__device__ __forceinline__ CassCall cass_mixed_view(const CassMixedCall &k, const CassMixedEnt &e, const CassCfg &c)
{
    CassCall v;
    v.c = c;
    v.blocks = k.blocks + e.block0;
    v.hiss = k.hiss;
    v.xs = k.xs + ((int64_t)e.xs - (int64_t)e.plane) * 2;                       // plane frame plane_t + f: entry taps_t - 1 + f of the section
    v.total = e.plane + e.frames;
    v.nblocks = e.nblocks;
    return v;
}

__device__ __forceinline__ CassMixedEnt cass_mixed_none()
{
    CassMixedEnt e;
    e.frames = e.plane = e.seg0 = e.tile0 = e.xs = e.tilt = e.count = 0;
    e.state = nullptr;
    e.block0 = e.nblocks = e.set = 0;
    e.warm = 0;
    return e;
}

// k_cass_track_front with the cfg and the warm-up of the segment's track
__global__ __launch_bounds__(64) void k_cass_mixed_front(CassMixedCall k, CassFrontRec *__restrict__ recs, uint32_t seg_len)
{
    __shared__ int32_t ring[CASS_GROUPS + 1][2][CASS_RING];
    __shared__ double init[CASS_GROUPS + 1][CASS_FRONT_VALUES];
    const int lane = (int)threadIdx.x, g = lane / CASS_LANES, r = lane - g * CASS_LANES;
    const uint64_t j = (uint64_t)blockIdx.x * CASS_GROUPS + (uint64_t)g;
    const bool live = g < CASS_GROUPS && j < k.nseg;
    CassMixedEnt e = cass_mixed_none();
    AudioSeg s{0, 0, 0};
    if (live) {
        e = k.tracks[cass_track_of_seg(k.tracks, k.ntracks, j)];
        s = audio_seg(e.frames, seg_len, e.warm, j - e.seg0);                    // clamps at frame 0 of this track
    }
    const CassCfg c = k.cfgs[e.set];                                            // entry 0 exists whenever a track has frames
    if (live) {
        const bool spec = s.run_start != 0;
        for (int i = r; i < CASS_FRONT_VALUES; i += CASS_LANES) {
            const double v = (spec && cass_front_live(c, i)) || !e.state ? 0.0 : e.state->front.v[i];
            init[g][i] = v;
            recs[j].at_start.v[i] = v;
            recs[j].at_end.v[i] = v;
        }
        if (r == 0) {
            recs[j].at_start.count = e.count + s.start;
            recs[j].at_end.count = e.count + s.start + s.len;
        }
    }
    __syncthreads();
    const CassCall view = cass_mixed_view(k, e, c);
    cass_run_lanes(view, r, live, e.plane + s.run_start, s.start - s.run_start, s.len, init[g], live ? &recs[j].at_start : nullptr,
                   live ? &recs[j].at_end : nullptr, ring[g][0], ring[g][1]);
}

// One workgroup (one wavefront) per track, as k_cass_track_front_verify: the cfg is the workgroup's.
__global__ __launch_bounds__(64) void k_cass_mixed_front_verify(CassMixedCall k, const CassFrontRec *__restrict__ recs, uint32_t seg_len,
                                                                uint64_t *__restrict__ stats)
{
    __shared__ int32_t ring[2][CASS_RING];
    __shared__ CassFront truth;
    __shared__ double init[CASS_FRONT_VALUES];
    const int lane = (int)threadIdx.x;
    const CassMixedEnt e = k.tracks[blockIdx.x];
    if (e.frames == 0) return;
    const CassCfg c = k.cfgs[e.set];
    const CassCall view = cass_mixed_view(k, e, c);
    const uint64_t nseg = audio_seg_count(e.frames, seg_len);
    recs += e.seg0;
    double *const sec = k.xs + e.xs * 2;
    for (int i = lane; i < (c.taps - 1) * 2; i += 64) sec[i] = e.state ? e.state->hist[i >> 1][i & 1] : 0.0;
    if (lane < CASS_FRONT_VALUES) truth.v[lane] = e.state ? e.state->front.v[lane] : 0.0;
    if (lane == CASS_FRONT_VALUES) truth.count = e.count;
    __syncthreads();
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        bool same = true;
        if (lane < CASS_FRONT_VALUES) same = __double_as_longlong(recs[j].at_start.v[lane]) == __double_as_longlong(truth.v[lane]);
        if (lane == CASS_FRONT_VALUES) same = recs[j].at_start.count == truth.count;
        const bool ok = __all(same);
        __syncthreads();
        if (ok) {
            if (lane < CASS_FRONT_VALUES) truth.v[lane] = recs[j].at_end.v[lane];
            if (lane == CASS_FRONT_VALUES) truth.count = recs[j].at_end.count;
        } else {
            const AudioSeg s = audio_seg(e.frames, seg_len, e.warm, j);
            if (lane < CASS_FRONT_VALUES) init[lane] = truth.v[lane];
            __syncthreads();
            cass_run_lanes(view, lane, lane < CASS_LANES, e.plane + s.start, 0, s.len, init, nullptr, &truth, ring[0], ring[1]);
            if (lane == 0) truth.count += s.len;
            repaired++;
        }
        __syncthreads();
    }
    if (e.state && lane < CASS_FRONT_VALUES) e.state->front.v[lane] = truth.v[lane];
    if (lane == 0) stats[CASS_STAT_VALUES * (uint64_t)blockIdx.x + 1] = repaired;
}

__device__ __forceinline__ void cass_mixed_close(int taps, const CassMixedEnt &e, uint32_t seg_len, uint64_t *__restrict__ stats, uint64_t t)
{
    if (e.state) {
        e.state->front.count = e.count + e.frames;
        e.state->taps = (uint32_t)taps;
    }
    stats[CASS_STAT_VALUES * t] = audio_seg_count(e.frames, seg_len);
}

// One workgroup per call-wide tile.  The halo in front of a tile is its TRACK's taps - 1 frames (the LDS tile has room
// for CASS_HIST); head_tilt_final is made from the sine of the frame's count and the track's tilt and waver.  A track
// with de-emphasis leaves r in the plane for the back; one without is packed, downmixed, stored and closed here.
__global__ __launch_bounds__(CASS_TILE) void k_cass_mixed_conv(CassMixedCall k, const double *__restrict__ sines, double *__restrict__ rs, uint32_t seg_len,
                                                               uint64_t *__restrict__ stats)
{
    __shared__ double tile[2][CASS_TILE + CASS_HIST];
    const int t = (int)threadIdx.x;
    const int tr = cass_track_of_tile(k.tracks, k.ntracks, (uint64_t)blockIdx.x);
    const CassMixedEnt e = k.tracks[tr];
    const CassCfg c = k.cfgs[e.set];
    const int taps = c.taps;
    const uint64_t tile0 = ((uint64_t)blockIdx.x - e.tile0) * CASS_TILE;        // in the track
    const int own = (int)(e.frames - tile0 < CASS_TILE ? e.frames - tile0 : CASS_TILE);
    const double *sec = k.xs + e.xs * 2;
    const double *src = sec + tile0 * 2;                                        // section entry tile0 is frame tile0 - (taps - 1)
    for (int i = t; i < (own + taps - 1) * 2; i += CASS_TILE) tile[i & 1][i >> 1] = src[i];
    __syncthreads();
    if (t < own) {
        const uint64_t f = tile0 + (uint64_t)t;
        const double h = cass_tilt_of_sin(c, sines[e.tilt + f]);
        const double r0 = cass_conv<true>(taps, h, 0, &tile[0][t], 1);
        const double r1 = cass_conv<true>(taps, h, 1, &tile[1][t], 1);
        if (c.post) {
            rs[(e.plane + f) * 2] = r0;
            rs[(e.plane + f) * 2 + 1] = r1;
        } else {
            int16_t o0 = audio_pack(r0), o1 = audio_pack(r1);
            cass_downmix(c, o0, o1);
            const CassCall view = cass_mixed_view(k, e, c);
            const CassBlock &b = view.blocks[cass_find(view, e.plane + f)];
            int16_t *d = b.dst + (e.plane + f - b.first) * 2;
            d[0] = o0;
            d[1] = o1;
        }
    }
    if (tile0 == 0) {
        if (e.state)
            for (int i = t; i < (taps - 1) * 2; i += CASS_TILE) e.state->hist[i >> 1][i & 1] = sec[e.frames * 2 + (uint64_t)i];
        if (!c.post && t == 0) cass_mixed_close(taps, e, seg_len, stats, (uint64_t)tr);
    }
}

// one lane per call-wide segment; the segments of tracks without de-emphasis are skipped
__global__ __launch_bounds__(64) void k_cass_mixed_back(CassMixedCall k, const double *__restrict__ rs, CassBackRec *__restrict__ recs, uint32_t seg_len,
                                                        uint32_t warmup)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k.nseg) return;
    const CassMixedEnt e = k.tracks[cass_track_of_seg(k.tracks, k.ntracks, j)];
    const CassCfg c = k.cfgs[e.set];
    if (!c.post) return;
    const CassCall view = cass_mixed_view(k, e, c);
    const AudioSeg s = audio_seg(e.frames, seg_len, warmup, j - e.seg0);
    CassBack b{{0.0, 0.0}};
    if (e.state && s.run_start == 0) b = e.state->back;
    cass_back_run(view, b, rs, e.plane + s.run_start, s.start - s.run_start, false);
    recs[j].at_start = b;
    cass_back_run(view, b, rs, e.plane + s.start, s.len, true);
    recs[j].at_end = b;
}

// one lane per track that has de-emphasis: the ordered walk over its records; it closes the track
__global__ __launch_bounds__(64) void k_cass_mixed_back_verify(CassMixedCall k, const double *__restrict__ rs, const CassBackRec *__restrict__ recs,
                                                               uint32_t seg_len, uint32_t warmup, uint64_t *__restrict__ stats)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)k.ntracks) return;
    const CassMixedEnt e = k.tracks[t];
    if (e.frames == 0) return;
    const CassCfg c = k.cfgs[e.set];
    if (!c.post) return;
    const CassCall view = cass_mixed_view(k, e, c);
    const uint64_t nseg = audio_seg_count(e.frames, seg_len);
    recs += e.seg0;
    CassBack truth{{0.0, 0.0}};
    if (e.state) truth = e.state->back;
    uint64_t repaired = 0;
    for (uint64_t j = 0; j < nseg; j++) {
        const CassBackRec rec = recs[j];
        if (cass_back_same(rec.at_start, truth)) {
            truth = rec.at_end;
        } else {
            const AudioSeg s = audio_seg(e.frames, seg_len, warmup, j);
            cass_back_run(view, truth, rs, e.plane + s.start, s.len, true);
            repaired++;
        }
    }
    if (e.state) e.state->back = truth;
    stats[CASS_STAT_VALUES * t + 2] = repaired;
    cass_mixed_close(c.taps, e, seg_len, stats, t);
}

// ---------------------------------------------------------------------------------------- host side
constexpr int CASS_MARKS = 9;
constexpr int CASS_FILL_THREADS = 4;     // of the sin() fill of a long call; fixed, whatever the host has
constexpr uint64_t CASS_FILL_SPLIT = 1u << 18;   // frames from which the fill is split

struct CassStageState {
    ntscsim_cass_params prm;
    CassCfg cfg;
    CassState *state = nullptr;          // device: the carried state
    uint64_t count = 0;                  // the host's copy of its sample count: the sines are made here
    uint32_t *polys = nullptr;           // device: HISS_POLYS polynomials
    uint64_t *stats = nullptr;           // device: segments, repaired front, repaired back of the last call
    uint64_t *track_stats = nullptr;     // device: the same three per track of the last tracks call
    size_t track_stats_cap = 0;          // in values
    int last_tracks = 0;
    uint64_t tilt_frames = 0;            // sines the last call's fill evaluated
    int32_t *hiss = nullptr;
    double *xs = nullptr, *rs = nullptr, *tf = nullptr;
    CassFrontRec *frecs = nullptr;
    CassBackRec *brecs = nullptr;
    size_t hiss_cap = 0, xs_cap = 0, rs_cap = 0, tf_cap = 0, frecs_cap = 0, brecs_cap = 0;
    double *tf_host = nullptr;           // pinned: head_tilt_final of the call's frames
    size_t tf_host_cap = 0;
    hipEvent_t tf_done = nullptr;        // its last upload has finished
    bool tf_used = false;
    uint32_t plan_len = 0, plan_front = 0, plan_back = 0;
    bool plan_set = false;
    RecordSlots<> slots;
    FrameArena frames;                   // ntscsim_cass_host()
    bool timing = false;
    float fill_ms = 0;
    std::vector<hipEvent_t> marks;       // CASS_MARKS per call while timing
};

static void cass_drop_marks(CassStageState *k)
{
    for (hipEvent_t e : k->marks) (void)hipEventDestroy(e);
    k->marks.clear();
}

void cass_state_destroy(CassStageState *k)
{
    if (!k) return;
    if (k->state) (void)hipFree(k->state);
    if (k->polys) (void)hipFree(k->polys);
    if (k->stats) (void)hipFree(k->stats);
    if (k->track_stats) (void)hipFree(k->track_stats);
    if (k->hiss) (void)hipFree(k->hiss);
    if (k->xs) (void)hipFree(k->xs);
    if (k->rs) (void)hipFree(k->rs);
    if (k->tf) (void)hipFree(k->tf);
    if (k->frecs) (void)hipFree(k->frecs);
    if (k->brecs) (void)hipFree(k->brecs);
    if (k->tf_host) (void)hipHostFree(k->tf_host);
    if (k->tf_done) (void)hipEventDestroy(k->tf_done);
    cass_drop_marks(k);
    k->slots.release();
    k->frames.release();
    delete k;
}

} // namespace ntscsim

using namespace ntscsim;

namespace {

CassCfg cass_cfg_of(const ntscsim_cass_params &p)
{
    CassCfg c;
    std::memset(&c, 0, sizeof(c));
    c.pre = p.preemphasis != 0;
    c.post = p.deemphasis != 0;
    c.mono = p.mono != 0;
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

int cass_quiet(const CtxStageView &v)
{
    STAGECHK(v, hipSetDevice(v.device));
    STAGECHK(v, hipDeviceSynchronize());
    return NTSCSIM_OK;
}

template <class T>
int cass_grow(const CtxStageView &v, T *&p, size_t &cap, size_t want)
{
    if (want <= cap) return NTSCSIM_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    const size_t n = want + want / 4 + 1024;
    STAGECHK(v, hipMalloc((void **)&p, n * sizeof(T)));
    cap = n;
    return NTSCSIM_OK;
}

int cass_mark(const CtxStageView &v, CassStageState *k, hipStream_t st)
{
    if (!k->timing) return NTSCSIM_OK;
    hipEvent_t e = nullptr;
    STAGECHK(v, hipEventCreate(&e));
    k->marks.push_back(e);
    STAGECHK(v, hipEventRecord(e, st));
    return NTSCSIM_OK;
}

// The `total` entries of the FIR's table into the pinned staging -- part(at, n, table) fills entries [at, at + n); they
// are independent: a long table is split over a fixed number of threads -- then up on the call's stream
template <class Part>
int cass_upload_table(const CtxStageView &v, CassStageState *k, uint64_t total, hipStream_t st, Part part)
{
    if (k->tf_used) STAGECHK(v, hipEventSynchronize(k->tf_done));                // the last upload still reads the staging
    if (total > k->tf_host_cap) {
        if (k->tf_host) { (void)hipHostFree(k->tf_host); k->tf_host = nullptr; k->tf_host_cap = 0; }
        const size_t n = (size_t)total + (size_t)total / 4 + 1024;
        STAGECHK(v, hipHostMalloc((void **)&k->tf_host, n * sizeof(double), hipHostMallocPortable));
        k->tf_host_cap = n;
    }
    if (!k->tf_done) STAGECHK(v, hipEventCreateWithFlags(&k->tf_done, hipEventDisableTiming));
    const auto t0 = std::chrono::steady_clock::now();
    if (total < CASS_FILL_SPLIT) {
        part(0, total, k->tf_host);
    } else {
        std::thread helpers[CASS_FILL_THREADS - 1];
        const uint64_t each = (total + CASS_FILL_THREADS - 1) / CASS_FILL_THREADS;
        for (int i = 1; i < CASS_FILL_THREADS; i++) {
            const uint64_t at = std::min<uint64_t>(each * (uint64_t)i, total), n = std::min<uint64_t>(each, total - at);
            helpers[i - 1] = std::thread([k, part, at, n]() { part(at, n, k->tf_host); });
        }
        part(0, std::min<uint64_t>(each, total), k->tf_host);
        for (std::thread &h : helpers) h.join();
    }
    k->tilt_frames = total;
    k->fill_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    int rc = cass_mark(v, k, st);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpyAsync(k->tf, k->tf_host, (size_t)total * sizeof(double), hipMemcpyHostToDevice, st));
    STAGECHK(v, hipEventRecord(k->tf_done, st));
    k->tf_used = true;
    return cass_mark(v, k, st);
}

// head_tilt_final of the bound cfg at the table entries that the runs describe
int cass_upload_tilt_runs(const CtxStageView &v, CassStageState *k, const CassTiltRun *runs, size_t nruns, uint64_t total, hipStream_t st)
{
    const CassCfg cfg = k->cfg;
    return cass_upload_table(v, k, total, st, [cfg, runs, nruns](uint64_t at, uint64_t n, double *tf) { cass_fill_tilt_part(cfg, runs, nruns, at, n, tf); });
}

// a mixed call's table: the sines themselves
int cass_upload_sines(const CtxStageView &v, CassStageState *k, const CassSineRun *runs, size_t nruns, uint64_t total, hipStream_t st)
{
    return cass_upload_table(v, k, total, st, [runs, nruns](uint64_t at, uint64_t n, double *s) { cass_fill_sines_part(runs, nruns, at, n, s); });
}

// the single stream's table: one run from the host's copy of the count
int cass_upload_tilt(const CtxStageView &v, CassStageState *k, uint64_t total, hipStream_t st)
{
    const CassTiltRun one{k->count, total, 0};
    return cass_upload_tilt_runs(v, k, &one, 1, total, st);
}

int cass_blocks(ntscsim_ctx *c, const ntscsim_cass_desc *descs, int n, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    CassStageState *k = *v.cass;
    const CassCfg &cfg = k->cfg;
    const size_t fbytes = 2 * sizeof(int16_t);
    // every descriptor checked before anything is enqueued or the rand() position moves
    std::vector<Span> srcs;
    uint64_t total = 0;
    for (int i = 0; i < n; i++) {
        const ntscsim_cass_desc &d = descs[i];
        if (d.samples == 0) continue;
        if (!d.src || !d.dst || (((uintptr_t)d.src | (uintptr_t)d.dst) & 1)) return NTSCSIM_E_ARG;
        srcs.push_back(Span{(uintptr_t)d.src, (uintptr_t)d.src + (size_t)d.samples * fbytes});
        total += d.samples;
    }
    std::sort(srcs.begin(), srcs.end(), [](const Span &x, const Span &y) { return x.a < y.a; });
    std::vector<uintptr_t> reach(srcs.size());                                  // the furthest end among srcs[0..i]
    for (size_t i = 0; i < srcs.size(); i++) reach[i] = std::max(srcs[i].b, i ? reach[i - 1] : 0);
    for (int i = 0; i < n; i++) {
        const ntscsim_cass_desc &d = descs[i];
        if (d.samples == 0) continue;
        const uintptr_t a = (uintptr_t)d.dst, b = a + (size_t)d.samples * fbytes;
        const size_t m = (size_t)(std::lower_bound(srcs.begin(), srcs.end(), b, [](const Span &x, uintptr_t e) { return x.a < e; }) - srcs.begin());
        if (m > 0 && reach[m - 1] > a) return NTSCSIM_E_ARG;                    // a warm-up reads input again
    }
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    cass_drop_marks(k);
    const bool hiss = cfg.hiss_level != 0, post = cfg.post != 0;
    const uint32_t L = k->plan_len ? k->plan_len : AUDIO_DEFAULT_SEG;
    const uint32_t Wf = k->plan_set ? k->plan_front : cass_default_front_warmup(cfg);
    const uint32_t Wb = k->plan_set ? k->plan_back : CASS_DEFAULT_BACK_WARMUP;
    const uint64_t nseg = audio_seg_count(total, L);
    // the rand() position moves at call time, whatever becomes of the launch
    uint64_t pos = ntscsim_get_rng_pos(c);
    std::vector<uint64_t> block_pos((size_t)n);
    for (int i = 0; i < n; i++) {
        if (descs[i].rng_pos != NTSCSIM_RNG_AUTO) pos = descs[i].rng_pos;
        block_pos[(size_t)i] = pos;
        if (hiss) pos += (uint64_t)descs[i].samples * 2;
    }
    ntscsim_set_rng_pos(c, pos);
    STAGECHK(v, hipMemsetAsync(k->stats, 0, CASS_STAT_VALUES * sizeof(uint64_t), st));
    if (total == 0) return NTSCSIM_OK;
    const size_t plane = ((size_t)total + (size_t)(cfg.taps - 1)) * 2;
    if ((hiss && total * 2 > k->hiss_cap) || plane > k->xs_cap || (post && total * 2 > k->rs_cap) || total > k->tf_cap || nseg > k->frecs_cap ||
        (post && nseg > k->brecs_cap)) {
        int rc = k->slots.wait_all(v);                                          // launches in flight use what is replaced
        if (rc == NTSCSIM_OK && hiss) rc = cass_grow(v, k->hiss, k->hiss_cap, (size_t)total * 2);
        if (rc == NTSCSIM_OK) rc = cass_grow(v, k->xs, k->xs_cap, plane);
        if (rc == NTSCSIM_OK && post) rc = cass_grow(v, k->rs, k->rs_cap, (size_t)total * 2);
        if (rc == NTSCSIM_OK) rc = cass_grow(v, k->tf, k->tf_cap, (size_t)total);
        if (rc == NTSCSIM_OK) rc = cass_grow(v, k->frecs, k->frecs_cap, (size_t)nseg);
        if (rc == NTSCSIM_OK && post) rc = cass_grow(v, k->brecs, k->brecs_cap, (size_t)nseg);
        if (rc != NTSCSIM_OK) return rc;
    }
    // records: the blocks that have frames, then their rand() windows
    int m = 0;
    for (int i = 0; i < n; i++) m += descs[i].samples != 0;
    const size_t blocks_bytes = (size_t)m * sizeof(CassBlock), hb_bytes = hiss ? (size_t)m * sizeof(AudioHissBlock) : 0;
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, blocks_bytes + hb_bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    CassBlock *blocks = reinterpret_cast<CassBlock *>(slot->host);
    AudioHissBlock *hb = reinterpret_cast<AudioHissBlock *>(slot->host + blocks_bytes);
    uint64_t first = 0, max_items = 0;
    RandSeq seq(rand_state_origin());
    uint64_t seq_pos = UINT64_MAX;                                              // where seq stands; UINT64_MAX: nowhere
    for (int i = 0, o = 0; i < n; i++) {
        const ntscsim_cass_desc &d = descs[i];
        if (d.samples == 0) continue;
        blocks[o] = CassBlock{d.src, d.dst, first, d.samples};
        if (hiss) {
            audio_hiss_window(hb[o], seq, seq_pos, block_pos[(size_t)i], first * 2, (uint64_t)d.samples * 2, cfg.hiss_level);
            max_items = std::max(max_items, hb[o].items);
        }
        first += d.samples;
        o++;
    }
    STAGECHK(v, hipMemcpyAsync(slot->dev, slot->host, blocks_bytes + hb_bytes, hipMemcpyHostToDevice, st));
    CassCall call;
    call.c = cfg;
    call.blocks = reinterpret_cast<const CassBlock *>(slot->dev);
    call.hiss = hiss ? k->hiss : nullptr;
    call.xs = k->xs;
    call.total = total;
    call.nblocks = m;
    int lrc = cass_mark(v, k, st);                                              // 0
    if (lrc != NTSCSIM_OK) return lrc;
    if (hiss) {
        audio_hiss_launch(reinterpret_cast<const AudioHissBlock *>(slot->dev + blocks_bytes), m, max_items, k->polys, k->hiss, st);
        lrc = stage_launched(v, nullptr, st, "k_audio_hiss");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    lrc = cass_mark(v, k, st);                                                  // 1
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_cass_front, dim3((unsigned)((nseg + CASS_GROUPS - 1) / CASS_GROUPS)), dim3(64), 0, st, call, k->state, k->frecs, L, Wf);
    lrc = stage_launched(v, nullptr, st, "k_cass_front");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 2
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_cass_front_verify, dim3(1), dim3(64), 0, st, call, k->state, k->frecs, L, Wf, k->stats);
    lrc = stage_launched(v, nullptr, st, "k_cass_front_verify");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 3
    if (lrc != NTSCSIM_OK) return lrc;
    // only the FIR reads the head tilt: the host's sin() fill runs while the front is at work on the device
    lrc = cass_upload_tilt(v, k, total, st);                                    // 4, 5
    if (lrc != NTSCSIM_OK) return lrc;
    k->count += total;
    hipLaunchKernelGGL(k_cass_conv, dim3((unsigned)((total + CASS_TILE - 1) / CASS_TILE)), dim3(CASS_TILE), 0, st, call, k->tf, k->state,
                       post ? k->rs : (double *)nullptr);
    lrc = stage_launched(v, post ? nullptr : slot, st, "k_cass_conv");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 6
    if (lrc != NTSCSIM_OK) return lrc;
    if (post) {
        hipLaunchKernelGGL(k_cass_back, dim3((unsigned)((nseg + 63) / 64)), dim3(64), 0, st, call, k->rs, k->state, k->brecs, L, Wb);
        lrc = stage_launched(v, nullptr, st, "k_cass_back");
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                       // 7
        if (lrc != NTSCSIM_OK) return lrc;
        hipLaunchKernelGGL(k_cass_back_verify, dim3(1), dim3(64), 0, st, call, k->rs, k->state, k->brecs, L, Wb, k->stats);
        lrc = stage_launched(v, slot, st, "k_cass_back_verify");
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                       // 8
    } else {
        lrc = cass_mark(v, k, st);
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);
    }
    return lrc;
}

// ntscsim_cass_tracks_device(): n independent streams in one launch of each kernel
int cass_tracks(ntscsim_ctx *c, const ntscsim_cass_track *tracks, int n, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    CassStageState *k = *v.cass;
    const CassCfg &cfg = k->cfg;
    const size_t fbytes = 2 * sizeof(int16_t);
    // every track and descriptor checked before anything is enqueued or the rand() position moves
    std::vector<Span> srcs;
    std::vector<uintptr_t> states;
    uint64_t total = 0;
    size_t m = 0;                                                               // blocks that have frames
    for (int t = 0; t < n; t++) {
        const ntscsim_cass_track &tr = tracks[t];
        if (tr.n_blocks < 0 || (tr.n_blocks > 0 && !tr.blocks) || ((uintptr_t)tr.state & 7)) return NTSCSIM_E_ARG;
        if (tr.state) states.push_back((uintptr_t)tr.state);
        uint64_t frames = 0;
        for (int i = 0; i < tr.n_blocks; i++) {
            const ntscsim_cass_desc &d = tr.blocks[i];
            if (d.samples == 0) continue;
            if (!d.src || !d.dst || (((uintptr_t)d.src | (uintptr_t)d.dst) & 1)) return NTSCSIM_E_ARG;
            srcs.push_back(Span{(uintptr_t)d.src, (uintptr_t)d.src + (size_t)d.samples * fbytes});
            frames += d.samples;
            m++;
        }
        if (tr.count + frames < tr.count) return NTSCSIM_E_ARG;                 // the count would wrap inside the track
        total += frames;
    }
    if (m > (size_t)INT32_MAX) return NTSCSIM_E_ARG;
    std::sort(states.begin(), states.end());
    for (size_t i = 1; i < states.size(); i++)
        if (states[i] - states[i - 1] < sizeof(CassState)) return NTSCSIM_E_ARG;    // two tracks would share a state
    std::sort(srcs.begin(), srcs.end(), [](const Span &x, const Span &y) { return x.a < y.a; });
    std::vector<uintptr_t> reach(srcs.size());                                  // the furthest end among srcs[0..i]
    for (size_t i = 0; i < srcs.size(); i++) reach[i] = std::max(srcs[i].b, i ? reach[i - 1] : 0);
    for (int t = 0; t < n; t++)
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_cass_desc &d = tracks[t].blocks[i];
            if (d.samples == 0) continue;
            const uintptr_t a = (uintptr_t)d.dst, b = a + (size_t)d.samples * fbytes;
            const size_t at = (size_t)(std::lower_bound(srcs.begin(), srcs.end(), b, [](const Span &x, uintptr_t e) { return x.a < e; }) - srcs.begin());
            if (at > 0 && reach[at - 1] > a) return NTSCSIM_E_ARG;              // a warm-up reads input again, in any track
        }
    STAGECHK(v, hipSetDevice(v.device));
    if ((size_t)CASS_STAT_VALUES * (size_t)n > k->track_stats_cap) {
        int rc = k->slots.wait_all(v);                                          // launches in flight use what is replaced
        if (rc == NTSCSIM_OK) rc = cass_grow(v, k->track_stats, k->track_stats_cap, (size_t)CASS_STAT_VALUES * (size_t)n);
        if (rc != NTSCSIM_OK) return rc;
    }
    v.kernels->clear();
    cass_drop_marks(k);
    k->last_tracks = n;
    k->tilt_frames = 0;
    const bool hiss = cfg.hiss_level != 0, post = cfg.post != 0;
    const uint32_t L = k->plan_len ? k->plan_len : AUDIO_DEFAULT_SEG;
    const uint32_t Wf = k->plan_set ? k->plan_front : cass_default_front_warmup(cfg);
    const uint32_t Wb = k->plan_set ? k->plan_back : CASS_DEFAULT_BACK_WARMUP;
    // the rand() position moves at call time, whatever becomes of the launch: tracks in order, blocks in order
    uint64_t pos = ntscsim_get_rng_pos(c);
    std::vector<uint64_t> block_pos;
    block_pos.reserve(m);
    for (int t = 0; t < n; t++)
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_cass_desc &d = tracks[t].blocks[i];
            if (d.rng_pos != NTSCSIM_RNG_AUTO) pos = d.rng_pos;
            if (d.samples) block_pos.push_back(pos);
            if (hiss) pos += (uint64_t)d.samples * 2;
        }
    ntscsim_set_rng_pos(c, pos);
    if (n) STAGECHK(v, hipMemsetAsync(k->track_stats, 0, (size_t)n * CASS_STAT_VALUES * sizeof(uint64_t), st));
    if (total == 0) return NTSCSIM_OK;
    // records: the track table, the blocks that have frames, their rand() windows
    const size_t tab_bytes = (size_t)n * sizeof(CassTrackEnt), blocks_bytes = m * sizeof(CassBlock), hb_bytes = hiss ? m * sizeof(AudioHissBlock) : 0;
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, tab_bytes + blocks_bytes + hb_bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    CassTrackEnt *tab = reinterpret_cast<CassTrackEnt *>(slot->host);
    CassBlock *blocks = reinterpret_cast<CassBlock *>(slot->host + tab_bytes);
    AudioHissBlock *hb = reinterpret_cast<AudioHissBlock *>(slot->host + tab_bytes + blocks_bytes);
    int o = 0;
    uint64_t total_before = 0;                                                  // = the plane of the track, as cass_tracks_layout() sets it
    for (int t = 0; t < n; t++) {
        CassTrackEnt &e = tab[t];
        std::memset(&e, 0, sizeof(e));
        e.count = tracks[t].count;
        e.state = reinterpret_cast<CassState *>(tracks[t].state);
        e.block0 = o;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_cass_desc &d = tracks[t].blocks[i];
            if (d.samples == 0) continue;
            blocks[o++] = CassBlock{d.src, d.dst, total_before + e.frames, d.samples};   // first: in the plane
            e.frames += d.samples;
        }
        e.nblocks = o - e.block0;
        total_before += e.frames;
    }
    const CassTracksTotals z = cass_tracks_layout(tab, n, L, cfg.taps);
    std::vector<CassTiltRun> runs;
    uint64_t tilt_total = 0;
    if (!cass_tilt_layout(tab, n, runs, &tilt_total)) return NTSCSIM_E_ARG;      // checked above: not reached
    uint64_t max_items = 0;
    if (hiss) {
        RandSeq seq(rand_state_origin());
        uint64_t seq_pos = UINT64_MAX;                                          // where seq stands; UINT64_MAX: nowhere
        for (size_t b = 0; b < m; b++) {
            audio_hiss_window(hb[b], seq, seq_pos, block_pos[b], blocks[b].first * 2, blocks[b].frames * 2, cfg.hiss_level);
            max_items = std::max(max_items, hb[b].items);
        }
    }
    if ((hiss && z.frames * 2 > k->hiss_cap) || z.xs_frames * 2 > k->xs_cap || (post && z.frames * 2 > k->rs_cap) || tilt_total > k->tf_cap ||
        z.segments > k->frecs_cap || (post && z.segments > k->brecs_cap)) {
        int grc = k->slots.wait_all(v);                                         // launches in flight use what is replaced
        if (grc == NTSCSIM_OK && hiss) grc = cass_grow(v, k->hiss, k->hiss_cap, (size_t)z.frames * 2);
        if (grc == NTSCSIM_OK) grc = cass_grow(v, k->xs, k->xs_cap, (size_t)z.xs_frames * 2);
        if (grc == NTSCSIM_OK && post) grc = cass_grow(v, k->rs, k->rs_cap, (size_t)z.frames * 2);
        if (grc == NTSCSIM_OK) grc = cass_grow(v, k->tf, k->tf_cap, (size_t)tilt_total);
        if (grc == NTSCSIM_OK) grc = cass_grow(v, k->frecs, k->frecs_cap, (size_t)z.segments);
        if (grc == NTSCSIM_OK && post) grc = cass_grow(v, k->brecs, k->brecs_cap, (size_t)z.segments);
        if (grc != NTSCSIM_OK) return grc;
    }
    STAGECHK(v, hipMemcpyAsync(slot->dev, slot->host, tab_bytes + blocks_bytes + hb_bytes, hipMemcpyHostToDevice, st));
    CassTracksCall call;
    call.c = cfg;
    call.tracks = reinterpret_cast<const CassTrackEnt *>(slot->dev);
    call.blocks = reinterpret_cast<const CassBlock *>(slot->dev + tab_bytes);
    call.hiss = hiss ? k->hiss : nullptr;
    call.xs = k->xs;
    call.nseg = z.segments;
    call.ntracks = n;
    int lrc = cass_mark(v, k, st);                                              // 0
    if (lrc != NTSCSIM_OK) return lrc;
    if (hiss) {
        audio_hiss_launch(reinterpret_cast<const AudioHissBlock *>(slot->dev + tab_bytes + blocks_bytes), (int)m, max_items, k->polys, k->hiss, st);
        lrc = stage_launched(v, nullptr, st, "k_audio_hiss");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    lrc = cass_mark(v, k, st);                                                  // 1
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_cass_track_front, dim3((unsigned)((z.segments + CASS_GROUPS - 1) / CASS_GROUPS)), dim3(64), 0, st, call, k->frecs, L, Wf);
    lrc = stage_launched(v, nullptr, st, "k_cass_track_front");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 2
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_cass_track_front_verify, dim3((unsigned)n), dim3(64), 0, st, call, k->frecs, L, Wf, k->track_stats);
    lrc = stage_launched(v, nullptr, st, "k_cass_track_front_verify");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 3
    if (lrc != NTSCSIM_OK) return lrc;
    // only the FIR reads the head tilt: the host's sin() fill -- over the union of the tracks' counts, which the host knows
    // without asking the device -- runs while the front is at work there
    lrc = cass_upload_tilt_runs(v, k, runs.data(), runs.size(), tilt_total, st);   // 4, 5
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_cass_track_conv, dim3((unsigned)z.tiles), dim3(CASS_TILE), 0, st, call, k->tf, post ? k->rs : (double *)nullptr, L, k->track_stats);
    lrc = stage_launched(v, post ? nullptr : slot, st, "k_cass_track_conv");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 6
    if (lrc != NTSCSIM_OK) return lrc;
    if (post) {
        hipLaunchKernelGGL(k_cass_track_back, dim3((unsigned)((z.segments + 63) / 64)), dim3(64), 0, st, call, k->rs, k->brecs, L, Wb);
        lrc = stage_launched(v, nullptr, st, "k_cass_track_back");
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                       // 7
        if (lrc != NTSCSIM_OK) return lrc;
        hipLaunchKernelGGL(k_cass_track_back_verify, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, call, k->rs, k->brecs, L, Wb, k->track_stats);
        lrc = stage_launched(v, slot, st, "k_cass_track_back_verify");
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                       // 8
    } else {
        lrc = cass_mark(v, k, st);
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);
    }
    return lrc;
}

// what ntscsim_cass_bind() accepts
bool cass_params_ok(const ntscsim_cass_params &p)
{
    return !(p.channels != CASS_CHANNELS || p.passes != AUDIO_PASSES || p.rate <= 0 || !(p.lowpass_hz > 0) || !(p.highpass_hz > 0) || p.hiss_level < 0 ||
             p.hiss_level > 0x3FFFFFFF || p.taps < 1 || p.taps > CASS_MAX_TAPS || !(std::fabs(p.head_tilt) <= CASS_MAX_TAPS) ||
             p.taps != cass_taps(p.head_tilt));
}

// What a mixed call checks before it looks at a sample pointer: the shape of the arguments and the sets that tracks
// name.  cfgs: the set table (cass_mixed_set_table); cfg_of_track[t]: track t's place in it.
int cass_mixed_sets(const CassStageState *k, const ntscsim_cass_params *sets, int n_sets, const ntscsim_cass_mixed_track *tracks, int n,
                    std::vector<CassCfg> &cfgs, std::vector<int32_t> &cfg_of_track)
{
    if (n_sets < 0 || n < 0 || (n_sets > 0 && !sets) || (n > 0 && !tracks)) return NTSCSIM_E_ARG;
    std::vector<int32_t> set_of((size_t)n);
    for (int t = 0; t < n; t++) {
        const ntscsim_cass_mixed_track &tr = tracks[t];
        if (tr.set < -1 || tr.set >= n_sets || tr.n_blocks < 0 || (tr.n_blocks > 0 && !tr.blocks)) return NTSCSIM_E_ARG;
        if (tr.set >= 0 && sets[tr.set].struct_size != sizeof(ntscsim_cass_params)) return NTSCSIM_E_ARG;
        set_of[(size_t)t] = tr.set;
    }
    std::vector<int32_t> order;
    cass_mixed_set_table(set_of.data(), n, n_sets, order, cfg_of_track);
    cfgs.clear();
    for (const int32_t set : order) {
        if (set >= 0 && !cass_params_ok(sets[set])) return NTSCSIM_E_PARAM;
        cfgs.push_back(set < 0 ? k->cfg : cass_cfg_of(sets[set]));
    }
    return NTSCSIM_OK;
}

// ntscsim_cass_mixed_tracks_device(): n independent streams, each with the cfg of its set, in one launch of each kernel
int cass_mixed(ntscsim_ctx *c, const std::vector<CassCfg> &cfgs, const std::vector<int32_t> &cfg_of_track, const ntscsim_cass_mixed_track *tracks, int n,
               hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    CassStageState *k = *v.cass;
    const size_t fbytes = 2 * sizeof(int16_t);
    // every track and descriptor checked before anything is enqueued or the rand() position moves
    std::vector<Span> srcs;
    std::vector<uintptr_t> states;
    uint64_t total = 0;
    size_t m = 0, mh = 0;                                                       // blocks that have frames; those of them that draw
    bool post = false;                                                          // some track that has frames has de-emphasis
    for (int t = 0; t < n; t++) {
        const ntscsim_cass_mixed_track &tr = tracks[t];
        const CassCfg &cfg = cfgs[(size_t)cfg_of_track[(size_t)t]];
        if ((uintptr_t)tr.state & 7) return NTSCSIM_E_ARG;
        if (tr.state) states.push_back((uintptr_t)tr.state);
        uint64_t frames = 0;
        for (int i = 0; i < tr.n_blocks; i++) {
            const ntscsim_cass_desc &d = tr.blocks[i];
            if (d.samples == 0) continue;
            if (!d.src || !d.dst || (((uintptr_t)d.src | (uintptr_t)d.dst) & 1)) return NTSCSIM_E_ARG;
            srcs.push_back(Span{(uintptr_t)d.src, (uintptr_t)d.src + (size_t)d.samples * fbytes});
            frames += d.samples;
            m++;
            if (cfg.hiss_level != 0) mh++;
        }
        if (tr.count + frames < tr.count) return NTSCSIM_E_ARG;                 // the count would wrap inside the track
        if (frames && cfg.post) post = true;
        total += frames;
    }
    if (m > (size_t)INT32_MAX) return NTSCSIM_E_ARG;
    std::sort(states.begin(), states.end());
    for (size_t i = 1; i < states.size(); i++)
        if (states[i] - states[i - 1] < sizeof(CassState)) return NTSCSIM_E_ARG;    // two tracks would share a state
    std::sort(srcs.begin(), srcs.end(), [](const Span &x, const Span &y) { return x.a < y.a; });
    std::vector<uintptr_t> reach(srcs.size());                                  // the furthest end among srcs[0..i]
    for (size_t i = 0; i < srcs.size(); i++) reach[i] = std::max(srcs[i].b, i ? reach[i - 1] : 0);
    for (int t = 0; t < n; t++)
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_cass_desc &d = tracks[t].blocks[i];
            if (d.samples == 0) continue;
            const uintptr_t a = (uintptr_t)d.dst, b = a + (size_t)d.samples * fbytes;
            const size_t at = (size_t)(std::lower_bound(srcs.begin(), srcs.end(), b, [](const Span &x, uintptr_t e) { return x.a < e; }) - srcs.begin());
            if (at > 0 && reach[at - 1] > a) return NTSCSIM_E_ARG;              // a warm-up reads input again, in any track
        }
    STAGECHK(v, hipSetDevice(v.device));
    if ((size_t)CASS_STAT_VALUES * (size_t)n > k->track_stats_cap) {
        int rc = k->slots.wait_all(v);                                          // launches in flight use what is replaced
        if (rc == NTSCSIM_OK) rc = cass_grow(v, k->track_stats, k->track_stats_cap, (size_t)CASS_STAT_VALUES * (size_t)n);
        if (rc != NTSCSIM_OK) return rc;
    }
    v.kernels->clear();
    cass_drop_marks(k);
    k->last_tracks = n;
    k->tilt_frames = 0;
    const bool hiss = mh != 0;
    const uint32_t L = k->plan_len ? k->plan_len : AUDIO_DEFAULT_SEG;
    const uint32_t Wb = k->plan_set ? k->plan_back : CASS_DEFAULT_BACK_WARMUP;
    // the rand() position moves at call time: tracks in order, blocks in order, by the blocks of the tracks that draw
    uint64_t pos = ntscsim_get_rng_pos(c);
    std::vector<uint64_t> block_pos;
    block_pos.reserve(m);
    for (int t = 0; t < n; t++) {
        const bool draws = cfgs[(size_t)cfg_of_track[(size_t)t]].hiss_level != 0;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_cass_desc &d = tracks[t].blocks[i];
            if (d.rng_pos != NTSCSIM_RNG_AUTO) pos = d.rng_pos;
            if (d.samples) block_pos.push_back(pos);
            if (draws) pos += (uint64_t)d.samples * 2;
        }
    }
    ntscsim_set_rng_pos(c, pos);
    if (n) STAGECHK(v, hipMemsetAsync(k->track_stats, 0, (size_t)n * CASS_STAT_VALUES * sizeof(uint64_t), st));
    if (total == 0) return NTSCSIM_OK;
    // records: the set table, the track table, the blocks that have frames, the rand() windows of those that draw
    const size_t cfg_bytes = (cfgs.size() * sizeof(CassCfg) + 15) & ~(size_t)15, tab_bytes = (size_t)n * sizeof(CassMixedEnt),
                 blocks_bytes = m * sizeof(CassBlock), hb_bytes = mh * sizeof(AudioHissBlock);
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, cfg_bytes + tab_bytes + blocks_bytes + hb_bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    CassCfg *set_table = reinterpret_cast<CassCfg *>(slot->host);
    CassMixedEnt *tab = reinterpret_cast<CassMixedEnt *>(slot->host + cfg_bytes);
    CassBlock *blocks = reinterpret_cast<CassBlock *>(slot->host + cfg_bytes + tab_bytes);
    AudioHissBlock *hb = reinterpret_cast<AudioHissBlock *>(slot->host + cfg_bytes + tab_bytes + blocks_bytes);
    std::memset(slot->host, 0, cfg_bytes);
    std::memcpy(set_table, cfgs.data(), cfgs.size() * sizeof(CassCfg));
    int o = 0;
    uint64_t total_before = 0;                                                  // = the plane of the track, as cass_mixed_layout() sets it
    for (int t = 0; t < n; t++) {
        CassMixedEnt &e = tab[t];
        std::memset(&e, 0, sizeof(e));
        e.count = tracks[t].count;
        e.state = reinterpret_cast<CassState *>(tracks[t].state);
        e.set = cfg_of_track[(size_t)t];
        e.block0 = o;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_cass_desc &d = tracks[t].blocks[i];
            if (d.samples == 0) continue;
            blocks[o++] = CassBlock{d.src, d.dst, total_before + e.frames, d.samples};   // first: in the plane
            e.frames += d.samples;
        }
        e.nblocks = o - e.block0;
        total_before += e.frames;
    }
    const CassTracksTotals z = cass_mixed_layout(tab, n, cfgs.data(), L, k->plan_set ? &k->plan_front : nullptr);
    std::vector<CassSineRun> runs;
    uint64_t sines_total = 0;
    if (!cass_sine_layout(tab, n, cfgs.data(), runs, &sines_total)) return NTSCSIM_E_ARG;   // checked above: not reached
    uint64_t max_items = 0;
    if (hiss) {
        RandSeq seq(rand_state_origin());
        uint64_t seq_pos = UINT64_MAX;                                          // where seq stands; UINT64_MAX: nowhere
        size_t h = 0;
        for (int t = 0; t < n; t++) {
            const int level = cfgs[(size_t)tab[t].set].hiss_level;
            if (level == 0) continue;
            for (int b = tab[t].block0; b < tab[t].block0 + tab[t].nblocks; b++, h++) {
                audio_hiss_window(hb[h], seq, seq_pos, block_pos[(size_t)b], blocks[b].first * 2, blocks[b].frames * 2, level);
                max_items = std::max(max_items, hb[h].items);
            }
        }
    }
    if ((hiss && z.frames * 2 > k->hiss_cap) || z.xs_frames * 2 > k->xs_cap || (post && z.frames * 2 > k->rs_cap) || sines_total > k->tf_cap ||
        z.segments > k->frecs_cap || (post && z.segments > k->brecs_cap)) {
        int grc = k->slots.wait_all(v);                                         // launches in flight use what is replaced
        if (grc == NTSCSIM_OK && hiss) grc = cass_grow(v, k->hiss, k->hiss_cap, (size_t)z.frames * 2);
        if (grc == NTSCSIM_OK) grc = cass_grow(v, k->xs, k->xs_cap, (size_t)z.xs_frames * 2);
        if (grc == NTSCSIM_OK && post) grc = cass_grow(v, k->rs, k->rs_cap, (size_t)z.frames * 2);
        if (grc == NTSCSIM_OK) grc = cass_grow(v, k->tf, k->tf_cap, (size_t)sines_total);
        if (grc == NTSCSIM_OK) grc = cass_grow(v, k->frecs, k->frecs_cap, (size_t)z.segments);
        if (grc == NTSCSIM_OK && post) grc = cass_grow(v, k->brecs, k->brecs_cap, (size_t)z.segments);
        if (grc != NTSCSIM_OK) return grc;
    }
    STAGECHK(v, hipMemcpyAsync(slot->dev, slot->host, cfg_bytes + tab_bytes + blocks_bytes + hb_bytes, hipMemcpyHostToDevice, st));
    CassMixedCall call;
    call.cfgs = reinterpret_cast<const CassCfg *>(slot->dev);
    call.tracks = reinterpret_cast<const CassMixedEnt *>(slot->dev + cfg_bytes);
    call.blocks = reinterpret_cast<const CassBlock *>(slot->dev + cfg_bytes + tab_bytes);
    call.hiss = hiss ? k->hiss : nullptr;
    call.xs = k->xs;
    call.nseg = z.segments;
    call.ntracks = n;
    int lrc = cass_mark(v, k, st);                                              // 0
    if (lrc != NTSCSIM_OK) return lrc;
    if (hiss) {
        audio_hiss_launch(reinterpret_cast<const AudioHissBlock *>(slot->dev + cfg_bytes + tab_bytes + blocks_bytes), (int)mh, max_items, k->polys, k->hiss, st);
        lrc = stage_launched(v, nullptr, st, "k_audio_hiss");
        if (lrc != NTSCSIM_OK) return lrc;
    }
    lrc = cass_mark(v, k, st);                                                  // 1
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_cass_mixed_front, dim3((unsigned)((z.segments + CASS_GROUPS - 1) / CASS_GROUPS)), dim3(64), 0, st, call, k->frecs, L);
    lrc = stage_launched(v, nullptr, st, "k_cass_mixed_front");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 2
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_cass_mixed_front_verify, dim3((unsigned)n), dim3(64), 0, st, call, k->frecs, L, k->track_stats);
    lrc = stage_launched(v, nullptr, st, "k_cass_mixed_front_verify");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 3
    if (lrc != NTSCSIM_OK) return lrc;
    // only the FIR reads the sines: the host's fill runs while the front is at work on the device
    lrc = cass_upload_sines(v, k, runs.data(), runs.size(), sines_total, st);   // 4, 5
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_cass_mixed_conv, dim3((unsigned)z.tiles), dim3(CASS_TILE), 0, st, call, k->tf, post ? k->rs : (double *)nullptr, L, k->track_stats);
    lrc = stage_launched(v, post ? nullptr : slot, st, "k_cass_mixed_conv");
    if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                           // 6
    if (lrc != NTSCSIM_OK) return lrc;
    if (post) {
        hipLaunchKernelGGL(k_cass_mixed_back, dim3((unsigned)((z.segments + 63) / 64)), dim3(64), 0, st, call, k->rs, k->brecs, L, Wb);
        lrc = stage_launched(v, nullptr, st, "k_cass_mixed_back");
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                       // 7
        if (lrc != NTSCSIM_OK) return lrc;
        hipLaunchKernelGGL(k_cass_mixed_back_verify, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, call, k->rs, k->brecs, L, Wb, k->track_stats);
        lrc = stage_launched(v, slot, st, "k_cass_mixed_back_verify");
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);                       // 8
    } else {
        lrc = cass_mark(v, k, st);
        if (lrc == NTSCSIM_OK) lrc = cass_mark(v, k, st);
    }
    return lrc;
}

CassStageState *cass_of(ntscsim_ctx *c) { return c ? *ctx_stage_view(c).cass : nullptr; }

int cass_put_state(const CtxStageView &v, CassStageState *k, const CassState &s)
{
    const int rc = cass_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpy(k->state, &s, sizeof(CassState), hipMemcpyHostToDevice));
    k->count = s.front.count;
    return NTSCSIM_OK;
}

} // namespace

extern "C" int ntscsim_cass_bind(ntscsim_ctx *c, const ntscsim_cass_params *p)
{
    if (!c || !p || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    if (!cass_params_ok(*p)) return NTSCSIM_E_PARAM;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    CassStageState *k = *v.cass;
    if (!k) {
        k = new (std::nothrow) CassStageState();
        if (!k) return NTSCSIM_E_NOMEM;
        *v.cass = k;
    }
    const int rc = k->slots.wait_all(v);                                        // launches in flight use the state
    if (rc != NTSCSIM_OK) return rc;
    if (!k->state) STAGECHK(v, hipMalloc((void **)&k->state, sizeof(CassState)));
    if (!k->stats) STAGECHK(v, hipMalloc((void **)&k->stats, CASS_STAT_VALUES * sizeof(uint64_t)));
    if (!k->polys) {
        const int prc = audio_hiss_polys(v, &k->polys);
        if (prc != NTSCSIM_OK) return prc;
    }
    STAGECHK(v, hipMemset(k->stats, 0, CASS_STAT_VALUES * sizeof(uint64_t)));
    k->prm = *p;
    k->cfg = cass_cfg_of(*p);
    return ntscsim_cass_reset(c);
}

extern "C" int ntscsim_cass_device(ntscsim_ctx *c, const ntscsim_cass_desc *descs, int n, void *hip_stream)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    if (!*v.cass) return NTSCSIM_E_ARG;                                         // ntscsim_cass_bind() first
    return cass_blocks(c, descs, n, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

static_assert(sizeof(ntscsim_cass_track) == 32 && offsetof(ntscsim_cass_track, count) == 16 && offsetof(ntscsim_cass_track, state) == 24,
              "ntscsim_cass_track is what ntscsim/_capi.py mirrors");

extern "C" int ntscsim_cass_tracks_device(ntscsim_ctx *c, const ntscsim_cass_track *tracks, int n_tracks, void *hip_stream)
{
    if (!c || n_tracks < 0 || (n_tracks > 0 && !tracks)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    if (!*v.cass) return NTSCSIM_E_ARG;                                         // ntscsim_cass_bind() first
    return cass_tracks(c, tracks, n_tracks, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

static_assert(sizeof(ntscsim_cass_mixed_track) == 32 && offsetof(ntscsim_cass_mixed_track, set) == 12 && offsetof(ntscsim_cass_mixed_track, count) == 16 &&
                  offsetof(ntscsim_cass_mixed_track, state) == 24,
              "ntscsim_cass_mixed_track is what ntscsim/_capi.py mirrors");

extern "C" int ntscsim_cass_mixed_tracks_device(ntscsim_ctx *c, const ntscsim_cass_params *sets, int n_sets, const ntscsim_cass_mixed_track *tracks,
                                                int n_tracks, void *hip_stream)
{
    CassStageState *k = cass_of(c);
    if (!k) return NTSCSIM_E_ARG;                                               // ntscsim_cass_bind() first
    std::vector<CassCfg> cfgs;
    std::vector<int32_t> cfg_of_track;
    const int rc = cass_mixed_sets(k, sets, n_sets, tracks, n_tracks, cfgs, cfg_of_track);
    if (rc != NTSCSIM_OK) return rc;
    return cass_mixed(c, cfgs, cfg_of_track, tracks, n_tracks, hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx_stage_view(c).stream);
}

// The host form: every block's samples and every state through the ctx's staging -- [sources | states | results] on
// both sides, so that one copy goes up and one comes down around ONE device call.
extern "C" int ntscsim_cass_mixed_tracks_host(ntscsim_ctx *c, const ntscsim_cass_params *sets, int n_sets, const ntscsim_cass_mixed_track *tracks,
                                              int n_tracks)
{
    CassStageState *k = cass_of(c);
    if (!k) return NTSCSIM_E_ARG;
    std::vector<CassCfg> cfgs;
    std::vector<int32_t> cfg_of_track;
    int rc = cass_mixed_sets(k, sets, n_sets, tracks, n_tracks, cfgs, cfg_of_track);
    if (rc != NTSCSIM_OK) return rc;
    const size_t fbytes = 2 * sizeof(int16_t);
    size_t samples_bytes = 0, n_descs = 0, n_states = 0;
    std::vector<uintptr_t> states;
    for (int t = 0; t < n_tracks; t++) {
        if (tracks[t].state) states.push_back((uintptr_t)tracks[t].state);
        n_descs += (size_t)tracks[t].n_blocks;
        uint64_t frames = 0;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const ntscsim_cass_desc &d = tracks[t].blocks[i];
            if (d.samples && (!d.src || !d.dst)) return NTSCSIM_E_ARG;
            samples_bytes += (size_t)d.samples * fbytes;
            frames += d.samples;
        }
        if (tracks[t].count + frames < tracks[t].count) return NTSCSIM_E_ARG;   // refused before the staging is touched
    }
    n_states = states.size();
    std::sort(states.begin(), states.end());
    for (size_t i = 1; i < states.size(); i++)
        if (states[i] - states[i - 1] < sizeof(CassState)) return NTSCSIM_E_ARG;    // two tracks would share a state
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    const size_t src_bytes = (samples_bytes + 255) & ~(size_t)255, states_bytes = (n_states * sizeof(CassState) + 255) & ~(size_t)255;
    const size_t whole = 2 * src_bytes + states_bytes;
    if (whole > k->frames.arena_cap || whole > k->frames.staging_cap) {
        rc = k->slots.wait_all(v);                                              // launches in flight may use the arena
        if (rc == NTSCSIM_OK) rc = k->frames.reserve(v, whole, whole);
        if (rc != NTSCSIM_OK) return rc;
    }
    unsigned char *stage = k->frames.staging, *arena = k->frames.arena;
    std::vector<ntscsim_cass_desc> descs(n_descs);
    std::vector<ntscsim_cass_mixed_track> dev((size_t)n_tracks);
    size_t at = 0, s_at = 0, d_at = 0;
    for (int t = 0; t < n_tracks; t++) {
        dev[(size_t)t] = tracks[t];
        dev[(size_t)t].blocks = descs.data() + d_at;
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            ntscsim_cass_desc &d = descs[d_at++];
            d = tracks[t].blocks[i];
            const size_t bytes = (size_t)d.samples * fbytes;
            if (!bytes) continue;
            std::memcpy(stage + at, tracks[t].blocks[i].src, bytes);
            d.src = reinterpret_cast<const int16_t *>(arena + at);
            d.dst = reinterpret_cast<int16_t *>(arena + src_bytes + states_bytes + at);
            at += bytes;
        }
        if (tracks[t].state) {
            std::memcpy(stage + src_bytes + s_at, tracks[t].state, sizeof(CassState));
            dev[(size_t)t].state = reinterpret_cast<ntscsim_cass_state *>(arena + src_bytes + s_at);
            s_at += sizeof(CassState);
        }
    }
    if (src_bytes + states_bytes) STAGECHK(v, hipMemcpyAsync(arena, stage, src_bytes + states_bytes, hipMemcpyHostToDevice, v.stream));
    rc = cass_mixed(c, cfgs, cfg_of_track, dev.data(), n_tracks, v.stream);
    if (rc != NTSCSIM_OK) return rc;
    if (src_bytes + states_bytes)
        STAGECHK(v, hipMemcpyAsync(stage + src_bytes, arena + src_bytes, states_bytes + src_bytes, hipMemcpyDeviceToHost, v.stream));
    STAGECHK(v, hipStreamSynchronize(v.stream));
    at = s_at = 0;
    for (int t = 0; t < n_tracks; t++) {
        for (int i = 0; i < tracks[t].n_blocks; i++) {
            const size_t bytes = (size_t)tracks[t].blocks[i].samples * fbytes;
            if (!bytes) continue;
            std::memcpy(tracks[t].blocks[i].dst, stage + src_bytes + states_bytes + at, bytes);
            at += bytes;
        }
        if (tracks[t].state) {
            std::memcpy(tracks[t].state, stage + src_bytes + s_at, sizeof(CassState));
            s_at += sizeof(CassState);
        }
    }
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cass_host(ntscsim_ctx *c, int16_t *audio, uint32_t samples)
{
    CassStageState *k = cass_of(c);
    if (!k || (samples && !audio)) return NTSCSIM_E_ARG;
    if (samples == 0) return NTSCSIM_OK;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    const size_t bytes = (size_t)samples * 2 * sizeof(int16_t), half = (bytes + 255) & ~(size_t)255;
    const int arc = k->frames.reserve(v, 2 * half, half);
    if (arc != NTSCSIM_OK) return arc;
    std::memcpy(k->frames.staging, audio, bytes);
    STAGECHK(v, hipMemcpyAsync(k->frames.arena, k->frames.staging, bytes, hipMemcpyHostToDevice, v.stream));
    ntscsim_cass_desc d;
    std::memset(&d, 0, sizeof(d));
    d.src = reinterpret_cast<const int16_t *>(k->frames.arena);
    d.dst = reinterpret_cast<int16_t *>(k->frames.arena + half);
    d.samples = samples;
    d.rng_pos = NTSCSIM_RNG_AUTO;
    const int rc = cass_blocks(c, &d, 1, v.stream);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpyAsync(k->frames.staging, k->frames.arena + half, bytes, hipMemcpyDeviceToHost, v.stream));
    STAGECHK(v, hipStreamSynchronize(v.stream));
    std::memcpy(audio, k->frames.staging, bytes);
    return NTSCSIM_OK;
}

static_assert(sizeof(ntscsim_cass_state) == sizeof(CassState), "ntscsim_cass_state is CassState");
static_assert(offsetof(ntscsim_cass_state, count) == offsetof(CassState, front.count) && offsetof(ntscsim_cass_state, post) == offsetof(CassState, back) &&
                  offsetof(ntscsim_cass_state, taps) == offsetof(CassState, taps) && offsetof(ntscsim_cass_state, history) == offsetof(CassState, hist),
              "ntscsim_cass_state is CassState");

extern "C" int ntscsim_cass_reset(ntscsim_ctx *c)
{
    CassStageState *k = cass_of(c);
    if (!k) return NTSCSIM_E_ARG;
    std::vector<CassState> s(1);
    std::memset(s.data(), 0, sizeof(CassState));
    s[0].taps = (uint32_t)k->cfg.taps;
    return cass_put_state(ctx_stage_view(c), k, s[0]);
}

extern "C" int ntscsim_cass_get_state(ntscsim_ctx *c, ntscsim_cass_state *out)
{
    CassStageState *k = cass_of(c);
    if (!k || !out) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = cass_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpy(out, k->state, sizeof(CassState), hipMemcpyDeviceToHost));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cass_set_state(ntscsim_ctx *c, const ntscsim_cass_state *in)
{
    CassStageState *k = cass_of(c);
    if (!k || !in || in->taps != (uint32_t)k->cfg.taps) return NTSCSIM_E_ARG;
    std::vector<CassState> s(1);
    std::memcpy(s.data(), in, sizeof(CassState));
    return cass_put_state(ctx_stage_view(c), k, s[0]);
}

extern "C" int ntscsim_cass_debug_set_plan(ntscsim_ctx *c, uint32_t seg_len, uint32_t warmup_front, uint32_t warmup_back)
{
    CassStageState *k = cass_of(c);
    if (!k) return NTSCSIM_E_ARG;
    k->plan_len = seg_len;
    k->plan_front = warmup_front;
    k->plan_back = warmup_back;
    k->plan_set = seg_len != 0 || warmup_front != 0 || warmup_back != 0;        // (0, 0, 0) restores the defaults
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cass_debug_stats(ntscsim_ctx *c, ntscsim_cass_stats *out)
{
    CassStageState *k = cass_of(c);
    if (!k || !out) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = cass_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    uint64_t s[CASS_STAT_VALUES];
    STAGECHK(v, hipMemcpy(s, k->stats, sizeof(s), hipMemcpyDeviceToHost));
    out->segments = s[0];
    out->repaired_front = s[1];
    out->repaired_back = s[2];
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cass_debug_track_stats(ntscsim_ctx *c, ntscsim_cass_stats *out, int n_tracks)
{
    CassStageState *k = cass_of(c);
    if (!k || n_tracks < 0 || n_tracks > k->last_tracks || (n_tracks && !out)) return NTSCSIM_E_ARG;
    if (n_tracks == 0) return NTSCSIM_OK;
    CtxStageView v = ctx_stage_view(c);
    const int rc = cass_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    static_assert(sizeof(ntscsim_cass_stats) == CASS_STAT_VALUES * sizeof(uint64_t), "the track kernels write ntscsim_cass_stats");
    STAGECHK(v, hipMemcpy(out, k->track_stats, (size_t)n_tracks * sizeof(ntscsim_cass_stats), hipMemcpyDeviceToHost));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cass_debug_tilt_frames(ntscsim_ctx *c, uint64_t *evaluated)
{
    CassStageState *k = cass_of(c);
    if (!k || !evaluated) return NTSCSIM_E_ARG;
    *evaluated = k->tilt_frames;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cass_debug_time_kernels(ntscsim_ctx *c, int on)
{
    CassStageState *k = cass_of(c);
    if (!k) return NTSCSIM_E_ARG;
    k->timing = on != 0;
    if (!k->timing) cass_drop_marks(k);
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cass_debug_kernel_ms(ntscsim_ctx *c, float out_ms[8])
{
    CassStageState *k = cass_of(c);
    if (!k || !out_ms || k->marks.size() != CASS_MARKS) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = cass_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    // marks: 0 hiss 1 front 2 verify 3 (the host's fill) 4 upload 5 conv 6 back 7 back verify 8
    static const int from[7] = {4, 0, 1, 2, 5, 6, 7};
    out_ms[0] = k->fill_ms;
    for (int i = 0; i < 7; i++) STAGECHK(v, hipEventElapsedTime(&out_ms[i + 1], k->marks[(size_t)from[i]], k->marks[(size_t)from[i] + 1]));
    return NTSCSIM_OK;
}
