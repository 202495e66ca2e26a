// ntsc_avg.hip -- device half of the average_delay stage (include/ntscsim.h: ntscsim_avg_*): composite_layer() of
// ffmpeg_average_delay.cpp:801-837 for all layers of a frame in one pass, and the tool's frame loop over its ring of
// destination frames (:1069-1122) with the destination pixel held in registers.
//
// One lane = 4 pixels = one 16-byte load per present layer, one for the destination and one 16-byte store (frames
// whose pointers and linesizes are all multiples of 16; any other frame, and the last width % 4 pixels of a row,
// move as dwords).  The arithmetic is the tool's unsigned 32-bit arithmetic in one form that holds for every
// newlevel, the wrapping ones included.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ntscsim.h"
#include "ntsc_layer_frames.hpp"
#include "ntsc_px4.hpp"

namespace ntscsim {

#define ADEV __device__ __forceinline__

constexpr int AVG_FAST = NTSCSIM_AVG_FAST_LAYERS;
constexpr int AVG_THREADS = 256;
// the clip forms: one wave per workgroup, so that a small frame (720 x 486 is 1367 waves of quads) spreads over every SIMD
constexpr int AVG_CLIP_THREADS = 64;

struct AvgCfg { uint32_t n[AVG_FAST]; };      // fast forms: (uint32_t)newlevel per layer, a kernel argument

struct AvgLayerDev {                     // general forms: the layer lists, in device memory behind the records
    const uint8_t *src;                  // NULL: absent
    int32_t ls, _pad;
};

struct AvgRec {                          // one output frame
    uint8_t *dst;
    const uint8_t *src[AVG_FAST];        // fast forms
    const AvgLayerDev *layers;           // general forms
    int32_t src_ls[AVG_FAST];
    int32_t dst_ls;
    uint32_t vec;                        // every pointer and linesize of the frame is a multiple of 16
    uint32_t e;                          // efield = field / delay :802; only its low two bits reach a pixel
    uint32_t _pad;
};

struct AvgClip {                         // the clip forms: the ring behind the records, and what all frames share
    uint8_t *const *ring;
    int32_t ring_ls, ri, delay, T;
    int32_t src_ls[AVG_FAST];
    int32_t out_ls;
    uint32_t vec;                        // every pointer and linesize of the clip is a multiple of 16
};

// ((((x ^ y) + efield) & 3) * 255) / 3  :821 -- 0, 85, 170 or 255; xy = x ^ y
ADEV uint32_t avg_dither(uint32_t xy, uint32_t e) { return ((xy + e) & 3u) * 85u; }

// One pixel of one layer, :819-834.  The tool computes s_c * n + d_c * (256 - n) in unsigned int, n = (unsigned)newlevel;
// modulo 2^32 that is n * (s_c - d_c) + (d_c << 8) for EVERY n (a ring identity, no range assumed), which halves the
// 32-bit multiplications.  The channels are summed, not ORed, as :834 does: for n outside 0 .. 256 they carry.
ADEV uint32_t avg_px(uint32_t s, uint32_t d, uint32_t n, uint32_t dth)
{
    const uint32_t sr = (s >> 16) & 0xFF, sg = (s >> 8) & 0xFF, sb = s & 0xFF;
    const uint32_t dr = (d >> 16) & 0xFF, dg = (d >> 8) & 0xFF, db = d & 0xFF;
    const uint32_t r = (n * (sr - dr) + (dr << 8) + dth) >> 8;
    const uint32_t g = (n * (sg - dg) + (dg << 8) + dth) >> 8;
    const uint32_t b = (n * (sb - db) + (db << 8) + dth) >> 8;
    return (r << 16) + (g << 8) + b;
}

ADEV void avg_layer(uint32_t (&d)[4], const uint32_t (&s)[4], int npx, uint32_t n, const uint32_t (&dth)[4])
{
#pragma unroll
    for (int p = 0; p < 4; p++)
        if (p < npx) d[p] = avg_px(s[p], d[p], n, dth[p]);
}

// ---- the frames forms: blockIdx.y is a descriptor ---------------------------------------------------------------

template <bool VEC>
ADEV void avg_item_fast(const AvgRec &r, const AvgCfg &cfg, int nl, int y, int x, int npx)
{
    uint8_t *dp = r.dst + (size_t)y * (size_t)r.dst_ls + (size_t)x * 4u;
    uint32_t d[4], dth[4], s[AVG_FAST][4];
    const uint8_t *row[AVG_FAST];
    // the record's pointers and linesizes are read first, then every vector load is issued: the layers' sources are
    // independent of each other and of the destination
#pragma unroll
    for (int k = 0; k < AVG_FAST; k++) row[k] = k < nl && r.src[k] ? r.src[k] + (size_t)y * (size_t)r.src_ls[k] + (size_t)x * 4u : nullptr;
    px4_load<VEC>(d, dp, npx);
#pragma unroll
    for (int k = 0; k < AVG_FAST; k++)
        if (row[k]) px4_load<VEC>(s[k], row[k], npx);
#pragma unroll
    for (int p = 0; p < 4; p++) dth[p] = avg_dither((uint32_t)(x + p) ^ (uint32_t)y, r.e);
#pragma unroll
    for (int k = 0; k < AVG_FAST; k++)
        if (row[k]) avg_layer(d, s[k], npx, cfg.n[k], dth);
    px4_store<VEC>(dp, d, npx);
}

__global__ __launch_bounds__(AVG_THREADS) void k_avg_fast(const AvgRec *__restrict__ recs, AvgCfg cfg, int W, int H, int nl)
{
    const AvgRec &r = recs[blockIdx.y];
    const int Q = (W + 3) >> 2, total = Q * H;
    for (int item = blockIdx.x * AVG_THREADS + threadIdx.x; item < total; item += gridDim.x * AVG_THREADS) {
        const int y = item / Q, x = (item - y * Q) << 2;
        const int npx = W - x < 4 ? W - x : 4;
        if (r.vec && npx == 4) avg_item_fast<true>(r, cfg, nl, y, x, 4);
        else avg_item_fast<false>(r, cfg, nl, y, x, npx);
    }
}

template <bool VEC>
ADEV void avg_apply_general(uint32_t (&d)[4], const AvgRec &r, const uint32_t *__restrict__ gcfg, int nl, uint32_t e, int y, int x, int npx)
{
    uint32_t dth[4];
#pragma unroll
    for (int p = 0; p < 4; p++) dth[p] = avg_dither((uint32_t)(x + p) ^ (uint32_t)y, e);
    for (int k = 0; k < nl; k++) {
        const AvgLayerDev L = r.layers[k];
        if (!L.src) continue;
        uint32_t s[4];
        px4_load<VEC>(s, L.src + (size_t)y * (size_t)L.ls + (size_t)x * 4u, npx);
        avg_layer(d, s, npx, gcfg[k], dth);
    }
}

template <bool VEC>
ADEV void avg_item_general(const AvgRec &r, const uint32_t *__restrict__ gcfg, int nl, int y, int x, int npx)
{
    uint8_t *dp = r.dst + (size_t)y * (size_t)r.dst_ls + (size_t)x * 4u;
    uint32_t d[4];
    px4_load<VEC>(d, dp, npx);
    avg_apply_general<VEC>(d, r, gcfg, nl, r.e, y, x, npx);
    px4_store<VEC>(dp, d, npx);
}

__global__ __launch_bounds__(AVG_THREADS) void k_avg_general(const AvgRec *__restrict__ recs, const uint32_t *__restrict__ gcfg,
                                                             int W, int H, int nl)
{
    const AvgRec &r = recs[blockIdx.y];
    const int Q = (W + 3) >> 2, total = Q * H;
    for (int item = blockIdx.x * AVG_THREADS + threadIdx.x; item < total; item += gridDim.x * AVG_THREADS) {
        const int y = item / Q, x = (item - y * Q) << 2;
        const int npx = W - x < 4 ? W - x : 4;
        if (r.vec && npx == 4) avg_item_general<true>(r, gcfg, nl, y, x, 4);
        else avg_item_general<false>(r, gcfg, nl, y, x, npx);
    }
}

// ---- the clip forms: blockIdx.y is a chain ----------------------------------------------------------------------
// A chain is the frames t = chain, chain + delay, ... that share ring slot (ri + chain) % delay; efield grows by one
// from each to the next.  The destination quad is read from the ring once, written to recs[t].dst at every step and
// to the ring at the end.  The sources do not depend on the recurrence, so the fast form keeps the loads of the chain's
// next BUFS - 1 frames in flight: BUFS register buffers, the step loop unrolled over them so that no buffer is ever
// copied (a copy would wait for the loads it copies).  A lane has nothing but its own chain to hide latency with --
// a 720 x 486 clip with delay 1 is hardly more than one wave per SIMD -- so the read-ahead is deep: 7 frames of one
// layer, 5 of two, 3 of three or four (32 to 64 VGPRs of buffers).
template <int NL> struct AvgDepth { static constexpr int BUFS = NL == 1 ? 8 : NL == 2 ? 6 : 4; };

// what a step needs of a frame's record; read one step before it is used, so that the scalar load is not waited for
template <int NL> struct AvgPtrs { uint8_t *dst; const uint8_t *src[NL]; bool live; };
template <int NL>
ADEV AvgPtrs<NL> avg_ptrs(const AvgRec *__restrict__ recs, int t, int T, int chain)
{
    const AvgRec &r = recs[t < T ? t : chain];           // past the clip's end: a record that exists, and `live` false
    AvgPtrs<NL> h;
    h.dst = r.dst;
#pragma unroll
    for (int k = 0; k < NL; k++) h.src[k] = r.src[k];
    h.live = t < T;
    return h;
}

// the source loads of one frame into one buffer: NL loads, no branch between them -- an absent layer, and every layer
// of a frame past the clip's end, reads the ring quad instead (valid memory, a cache hit) and is not taken when the
// layers are applied -- so that the number of loads in flight behind a step's sources is the same on every path and
// the wait in front of the step leaves them in flight
template <bool VEC, int NL>
ADEV void avg_issue(uint32_t (&s)[NL][4], uint8_t *&dst, uint32_t &present, const AvgPtrs<NL> &f, const size_t (&soff)[NL],
                    const uint8_t *ringquad)
{
    const uint8_t *p[NL];
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < NL; k++) {
        const bool there = f.live && f.src[k];
        p[k] = there ? f.src[k] + soff[k] : ringquad;
        m |= there ? 1u << k : 0u;
    }
#pragma unroll
    for (int k = 0; k < NL; k++) px4_load<VEC>(s[k], p[k], VEC ? 4 : 1);
    dst = f.dst;
    present = m;
}

template <bool VEC, int NL>
ADEV void avg_chain_fast(const AvgRec *__restrict__ recs, const AvgClip &clip, uint8_t *ring, const AvgCfg &cfg, int chain, int y, int x)
{
    // VEC: the lane's 4 pixels; otherwise ONE pixel per lane (x counts pixels), so that neither form has a per-lane branch
    constexpr int BUFS = AvgDepth<NL>::BUFS, AHEAD = BUFS - 1;
    const int dl = clip.delay, T = clip.T, npx = VEC ? 4 : 1;
    uint8_t *rp = ring + (size_t)y * (size_t)clip.ring_ls + (size_t)x * 4u;
    const size_t ooff = (size_t)y * (size_t)clip.out_ls + (size_t)x * 4u;
    size_t soff[NL];
#pragma unroll
    for (int k = 0; k < NL; k++) soff[k] = (size_t)y * (size_t)clip.src_ls[k] + (size_t)x * 4u;
    uint32_t d[4], xy[4], s[BUFS][NL][4], present[BUFS];
    uint8_t *dst[BUFS];
#pragma unroll
    for (int p = 0; p < 4; p++) xy[p] = (uint32_t)(x + p) ^ (uint32_t)y;
    uint32_t e = recs[chain].e;
    px4_load<VEC>(d, rp, npx);
    // the loads are kept in frame order: the wait in front of a step counts back from the youngest load, and the loop's
    // waits have to hold for the prologue's loads too
#pragma unroll
    for (int j = 0; j < AHEAD; j++) {
        avg_issue<VEC, NL>(s[j], dst[j], present[j], avg_ptrs<NL>(recs, chain + j * dl, T, chain), soff, rp);
        __builtin_amdgcn_sched_barrier(0);
    }
    AvgPtrs<NL> next = avg_ptrs<NL>(recs, chain + AHEAD * dl, T, chain);
    // A round is BUFS whole steps without a branch: the chain's step count is rounded up, and a surplus step (tj >= T)
    // takes no layer and stores the quad where the end of the chain stores it anyway, into the ring.  Within a step the
    // order is fixed -- the loads of the frame AHEAD steps on, the scalar load of the record behind it, then the
    // arithmetic and the store -- and steps do not interleave: the compiler counts its waits from that order, and left
    // to itself it sinks the loads behind the arithmetic.  The first round stands in front of the loop, so that the
    // loop is entered with the same loads and stores in flight as it goes round with, and its waits (2 * AHEAD
    // operations stay in flight in front of every step) are not cut down to the prologue's.
    auto round = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < BUFS; j++) {
            const int tj = t + j * dl;
            avg_issue<VEC, NL>(s[(j + AHEAD) % BUFS], dst[(j + AHEAD) % BUFS], present[(j + AHEAD) % BUFS], next, soff, rp);
            next = avg_ptrs<NL>(recs, tj + BUFS * dl, T, chain);
            __builtin_amdgcn_sched_barrier(0);
            uint32_t dth[4];
#pragma unroll
            for (int p = 0; p < 4; p++) dth[p] = avg_dither(xy[p], e);
            e++;
            // a layer that is not there is computed and not taken: a select, no branch
#pragma unroll
            for (int k = 0; k < NL; k++) {
                uint32_t v[4] = {d[0], d[1], d[2], d[3]};
                avg_layer(v, s[j][k], npx, cfg.n[k], dth);
                const bool take = (present[j] >> k) & 1u;
#pragma unroll
                for (int p = 0; p < 4; p++) d[p] = take ? v[p] : d[p];
            }
            px4_store<VEC>(tj < T ? dst[j] + ooff : rp, d, npx);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    round(chain);
    for (int t = chain + BUFS * dl; t < T; t += BUFS * dl) round(t);
    px4_store<VEC>(rp, d, npx);
}

// <NL>: number of layers, 1 .. NTSCSIM_AVG_FAST_LAYERS
template <int NL>
__global__ __launch_bounds__(AVG_CLIP_THREADS) void k_avg_clip_fast(const AvgRec *__restrict__ recs, AvgClip clip, AvgCfg cfg, int W, int H)
{
    const int chain = blockIdx.y;
    uint8_t *ring = clip.ring[(clip.ri + chain) % clip.delay];
    if (clip.vec != 0) {
        const int Q = W >> 2, total = Q * H;
        for (int item = blockIdx.x * AVG_CLIP_THREADS + threadIdx.x; item < total; item += gridDim.x * AVG_CLIP_THREADS) {
            const int y = item / Q;
            avg_chain_fast<true, NL>(recs, clip, ring, cfg, chain, y, (item - y * Q) << 2);
        }
        const int rest = W & 3, total1 = rest * H;      // the last width % 4 pixels of every row, one per lane
        for (int item = blockIdx.x * AVG_CLIP_THREADS + threadIdx.x; item < total1; item += gridDim.x * AVG_CLIP_THREADS) {
            const int y = item / rest;
            avg_chain_fast<false, NL>(recs, clip, ring, cfg, chain, y, (W & ~3) + (item - y * rest));
        }
    } else {
        const int total = W * H;
        for (int item = blockIdx.x * AVG_CLIP_THREADS + threadIdx.x; item < total; item += gridDim.x * AVG_CLIP_THREADS) {
            const int y = item / W;
            avg_chain_fast<false, NL>(recs, clip, ring, cfg, chain, y, item - y * W);
        }
    }
}

template <bool VEC>
ADEV void avg_chain_general(const AvgRec *__restrict__ recs, const AvgClip &clip, uint8_t *ring, const uint32_t *__restrict__ gcfg,
                            int nl, int chain, int y, int x, int npx)
{
    uint8_t *rp = ring + (size_t)y * (size_t)clip.ring_ls + (size_t)x * 4u;
    const size_t ooff = (size_t)y * (size_t)clip.out_ls + (size_t)x * 4u;
    uint32_t d[4];
    uint32_t e = recs[chain].e;
    px4_load<VEC>(d, rp, npx);
    for (int t = chain; t < clip.T; t += clip.delay, e++) {
        const AvgRec &r = recs[t];
        avg_apply_general<VEC>(d, r, gcfg, nl, e, y, x, npx);
        px4_store<VEC>(r.dst + ooff, d, npx);
    }
    px4_store<VEC>(rp, d, npx);
}

__global__ __launch_bounds__(AVG_CLIP_THREADS) void k_avg_clip_general(const AvgRec *__restrict__ recs, AvgClip clip,
                                                                       const uint32_t *__restrict__ gcfg, int W, int H, int nl)
{
    const int chain = blockIdx.y;
    uint8_t *ring = clip.ring[(clip.ri + chain) % clip.delay];
    const int Q = (W + 3) >> 2, total = Q * H;
    for (int item = blockIdx.x * AVG_CLIP_THREADS + threadIdx.x; item < total; item += gridDim.x * AVG_CLIP_THREADS) {
        const int y = item / Q, x = (item - y * Q) << 2;
        const int npx = W - x < 4 ? W - x : 4;
        if (clip.vec != 0 && npx == 4) avg_chain_general<true>(recs, clip, ring, gcfg, nl, chain, y, x, 4);
        else avg_chain_general<false>(recs, clip, ring, gcfg, nl, chain, y, x, npx);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------

struct AvgState {
    ntscsim_avg_params prm;
    std::vector<uint32_t> cfg;           // (uint32_t)newlevel per layer
    uint32_t *cfg_dev = nullptr;         // general forms
    RecordSlots<> slots;
    FrameArena frames;                   // ntscsim_avg_frames_host()
    LayerGeom geom() const { return LayerGeom{prm.width, prm.height, prm.n_layers}; }
};

void avg_state_destroy(AvgState *k)
{
    if (!k) return;
    if (k->cfg_dev) (void)hipFree(k->cfg_dev);
    k->slots.release();
    k->frames.release();
    delete k;
}

} // namespace ntscsim

using namespace ntscsim;

extern "C" int ntscsim_avg_bind(ntscsim_ctx *c, const ntscsim_avg_params *p)
{
    if (!c || !p || p->struct_size != sizeof(*p) || p->n_layers < 0 || (p->n_layers > 0 && !p->layers)) return NTSCSIM_E_ARG;
    if (p->delay < 1 || p->delay > 256) return NTSCSIM_E_PARAM;                 // :647-650
    if (p->width < 1 || p->height < 1 || p->width > (1 << 16) || p->height > (1 << 16) ||
        (uint64_t)p->width * (uint64_t)p->height >= (1ull << 31)) return NTSCSIM_E_SIZE;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    AvgState *k = *v.avg;
    if (!k) {
        k = new (std::nothrow) AvgState();
        if (!k) return NTSCSIM_E_NOMEM;
        *v.avg = k;
    }
    const int rc = k->slots.wait_all(v);                                        // launches in flight read the layer settings
    if (rc != NTSCSIM_OK) return rc;
    k->prm = *p;
    k->prm.layers = nullptr;
    k->prm.output_path = nullptr;
    k->prm.layers_cap = 0;
    k->cfg.clear();
    for (int l = 0; l < p->n_layers; l++) k->cfg.push_back((uint32_t)p->layers[l].newlevel);   // int -> unsigned, as :819 converts it
    if (k->cfg_dev) { (void)hipFree(k->cfg_dev); k->cfg_dev = nullptr; }
    if (p->n_layers > 0) {
        STAGECHK(v, hipMalloc((void **)&k->cfg_dev, k->cfg.size() * sizeof(uint32_t)));
        STAGECHK(v, hipMemcpy(k->cfg_dev, k->cfg.data(), k->cfg.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    return NTSCSIM_OK;
}

namespace {

// One launch over descriptors that do not depend on each other, or -- clip != NULL -- over the frames of a clip,
// whose chains the kernel itself walks in order.
int avg_launch(ntscsim_ctx *c, const ntscsim_avg_desc *descs, int n, const AvgClip *clip, void *const *ring_host, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    AvgState *k = *v.avg;
    const int W = k->prm.width, H = k->prm.height, nl = k->prm.n_layers;
    const uint64_t delay = (uint64_t)k->prm.delay;
    const bool general = nl > AVG_FAST || (clip && nl == 0);    // the fast clip form is instantiated for 1 .. 4 layers

    // records | layer lists (general) | ring pointers (clip) go up through a pinned slot of their own
    const size_t rec_bytes = (size_t)n * sizeof(AvgRec);
    const size_t lay_bytes = general ? (size_t)n * (size_t)nl * sizeof(AvgLayerDev) : 0;
    const size_t ring_bytes = clip ? (size_t)clip->delay * sizeof(uint8_t *) : 0;
    const size_t bytes = rec_bytes + lay_bytes + ring_bytes;
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    RecordSlot &s = *slot;
    AvgRec *recs = reinterpret_cast<AvgRec *>(s.host);
    AvgLayerDev *lays = reinterpret_cast<AvgLayerDev *>(s.host + rec_bytes);
    uint8_t **ringp = reinterpret_cast<uint8_t **>(s.host + rec_bytes + lay_bytes);
    const AvgLayerDev *lays_dev = reinterpret_cast<const AvgLayerDev *>(s.dev + rec_bytes);

    uintptr_t allbits = 0;
    if (clip) {
        allbits |= (uintptr_t)clip->ring_ls;
        for (int i = 0; i < clip->delay; i++) { ringp[i] = static_cast<uint8_t *>(ring_host[i]); allbits |= (uintptr_t)ring_host[i]; }
    }
    for (int i = 0; i < n; i++) {
        const ntscsim_avg_desc &d = descs[i];
        AvgRec &r = recs[i];
        std::memset(&r, 0, sizeof(r));
        r.dst = static_cast<uint8_t *>(d.dst_dev);
        r.dst_ls = d.dst_linesize;
        r.e = (uint32_t)(d.field / delay);                                      // :802, 64-bit
        uintptr_t bits = (uintptr_t)d.dst_dev | (uintptr_t)d.dst_linesize;
        for (int l = 0; l < nl; l++) {
            const ntscsim_avg_src &sl = d.layers[l];
            if (sl.src_dev) bits |= (uintptr_t)sl.src_dev | (uintptr_t)sl.src_linesize;
            if (general) {
                AvgLayerDev &L = lays[(size_t)i * (size_t)nl + (size_t)l];
                L.src = static_cast<const uint8_t *>(sl.src_dev);
                L.ls = sl.src_linesize;
                L._pad = 0;
            } else {
                r.src[l] = static_cast<const uint8_t *>(sl.src_dev);
                r.src_ls[l] = sl.src_linesize;
            }
        }
        if (general) r.layers = lays_dev + (size_t)i * (size_t)nl;
        r.vec = (bits & 15) == 0;
        allbits |= bits;
    }
    STAGECHK(v, hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, st));

    AvgCfg cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    for (int l = 0; l < nl && l < AVG_FAST; l++) cfg.n[l] = k->cfg[(size_t)l];
    const AvgRec *recs_dev = reinterpret_cast<const AvgRec *>(s.dev);
    if (clip) {
        AvgClip cd = *clip;
        cd.ring = reinterpret_cast<uint8_t *const *>(s.dev + rec_bytes + lay_bytes);
        cd.vec = (allbits & 15) == 0;
        // every quad (every pixel where the clip moves as dwords) has a lane of its own: a lane's chain is long
        const long long items = cd.vec ? std::max((long long)(W >> 2) * H, (long long)(W & 3) * H) : (long long)W * H;
        const long long slices = std::max(1LL, ((general ? (long long)((W + 3) / 4) * H : items) + AVG_CLIP_THREADS - 1) / AVG_CLIP_THREADS);
        const dim3 grid((unsigned)slices, (unsigned)std::min(clip->delay, clip->T)), block(AVG_CLIP_THREADS);
        if (general) hipLaunchKernelGGL(k_avg_clip_general, grid, block, 0, st, recs_dev, cd, k->cfg_dev, W, H, nl);
        else {
            switch (nl) {
            case 1: hipLaunchKernelGGL(k_avg_clip_fast<1>, grid, block, 0, st, recs_dev, cd, cfg, W, H); break;
            case 2: hipLaunchKernelGGL(k_avg_clip_fast<2>, grid, block, 0, st, recs_dev, cd, cfg, W, H); break;
            case 3: hipLaunchKernelGGL(k_avg_clip_fast<3>, grid, block, 0, st, recs_dev, cd, cfg, W, H); break;
            default: hipLaunchKernelGGL(k_avg_clip_fast<4>, grid, block, 0, st, recs_dev, cd, cfg, W, H); break;
            }
        }
    } else {
        const long long slices = ((long long)((W + 3) / 4) * H + AVG_THREADS - 1) / AVG_THREADS;
        // a short call still spreads over the machine: about 8192 workgroups in all
        const long long per = std::max(1LL, std::min(slices, (8192LL + n - 1) / n));
        const dim3 grid((unsigned)per, (unsigned)n), block(AVG_THREADS);
        if (general) hipLaunchKernelGGL(k_avg_general, grid, block, 0, st, recs_dev, k->cfg_dev, W, H, nl);
        else hipLaunchKernelGGL(k_avg_fast, grid, block, 0, st, recs_dev, cfg, W, H, nl);
    }
    return stage_launched(v, &s, st, clip ? (general ? "k_avg_clip_general" : "k_avg_clip_fast<" + std::to_string(nl) + ">") : (general ? "k_avg_general" : "k_avg_fast"));
}

} // namespace

extern "C" int ntscsim_avg_frames_device(ntscsim_ctx *c, const ntscsim_avg_desc *descs, int n, void *hip_stream)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    AvgState *k = *v.avg;
    if (!k) return NTSCSIM_E_ARG;                                               // ntscsim_avg_bind() first
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream;
    return layer_frames_in_order(k->geom(), descs, n, 65535,
                                 [&](const ntscsim_avg_desc *d, int m) { return avg_launch(c, d, m, nullptr, nullptr, st); });
}

extern "C" int ntscsim_avg_clip_device(ntscsim_ctx *c, void *const *ring_dev, int ring_linesize, int32_t *ring_index,
                                       const void *const *src_dev, const int32_t *src_linesize, void *const *out_dev,
                                       int out_linesize, int T, uint64_t *field, void *hip_stream)
{
    if (!c || !ring_dev || !ring_index || !field || T < 0 || (T > 0 && !out_dev)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    AvgState *k = *v.avg;
    if (!k) return NTSCSIM_E_ARG;
    const int nl = k->prm.n_layers, delay = k->prm.delay;
    if (nl > 0 && (!src_dev || !src_linesize)) return NTSCSIM_E_ARG;
    if (*ring_index < 0 || *ring_index >= delay) return NTSCSIM_E_ARG;
    if (T > (1 << 24)) return NTSCSIM_E_SIZE;                                   // the kernels count frames in int
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    std::vector<ntscsim_avg_desc> descs;
    std::vector<ntscsim_avg_src> lays;
    int rc = layer_clip_descs(k->geom(), delay, ring_dev, ring_linesize, src_dev, src_linesize, out_dev, out_linesize, T, true, descs, lays);
    if (rc != NTSCSIM_OK) return rc;
    AvgClip clip;
    std::memset(&clip, 0, sizeof(clip));
    clip.ring_ls = ring_linesize; clip.ri = *ring_index; clip.delay = delay; clip.T = T; clip.out_ls = out_linesize;
    for (int l = 0; l < nl && l < AVG_FAST; l++) clip.src_ls[l] = src_linesize[l];
    for (int t = 0; t < T; t++) descs[(size_t)t].field = *field + (uint64_t)t;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream;
    if (T > 0) {
        // a chain's efield grows by one per step only from the chain's own first frame: the records carry it
        rc = avg_launch(c, descs.data(), T, &clip, ring_dev, st);
        if (rc != NTSCSIM_OK) return rc;
    }
    *ring_index = (int)(((long long)*ring_index + T) % delay);
    *field += (uint64_t)T;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_avg_frames_host(ntscsim_ctx *c, const ntscsim_avg_desc *descs, int n)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    AvgState *k = *v.avg;
    if (!k) return NTSCSIM_E_ARG;
    return layer_frames_host(v, k->frames, k->geom(), descs, n,
                             [&](const ntscsim_avg_desc *d, int m, hipStream_t st) { return ntscsim_avg_frames_device(c, d, m, st); });
}
