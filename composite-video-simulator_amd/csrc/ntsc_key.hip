// ntsc_key.hip -- device half of the colorkey stage (include/ntscsim.h: ntscsim_key_*): composite_layer() of
// ffmpeg_colorkey.cpp:844-885 for all layers of a frame in one pass, and the tool's frame loop over its ring of
// destination frames (:1118-1171) with the destination pixel held in registers.
//
// One lane = 4 pixels = one 16-byte load per present layer, one for the destination and one 16-byte store (frames
// whose pointers and linesizes are all multiples of 16; any other frame, and the last width % 4 pixels of a row,
// move as dwords).  The tool's rand() draws (-noise: three per pixel and noisy layer, one serial stream) are made
// by k_key_draw in front of the pixel kernel: a lane owns 256 consecutive pixels of one (frame, layer), reaches
// its start by jump61 from the layer's window with a per-lane polynomial, and leaves one hit bit per pixel; the
// pixel kernel reads the bits coalesced with its pixels.  The forms without noise contain none of this.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "key_host.hpp"
#include "ntscsim.h"
#include "ntsc_layer_frames.hpp"
#include "ntsc_px4.hpp"

namespace ntscsim {

#define KDEV __device__ __forceinline__

constexpr int KEY_FAST = NTSCSIM_KEY_FAST_LAYERS;
constexpr int KEY_THREADS = 256;
constexpr int KEY_DRAW_THREADS = 64;     // one wave, one rand() ring in LDS

struct KeyCfgLayer {                     // ntscsim_key_layer without the path
    uint32_t color;
    int32_t thr;
    uint32_t fade, xdivr, invert, noisekey;
};
struct KeyCfg { KeyCfgLayer l[KEY_FAST]; };   // fast forms: a kernel argument

struct KeyLayerDev {                     // general forms: the layer lists, in device memory behind the records
    const uint8_t *src;                  // NULL: absent
    const uint32_t *bits;                // NULL: the layer draws nothing
    int32_t ls, _pad;
};

struct KeyRec {                          // one output frame
    uint8_t *dst;
    const uint8_t *src[KEY_FAST];        // fast forms
    const uint32_t *bits[KEY_FAST];
    const KeyLayerDev *layers;           // general forms
    int32_t src_ls[KEY_FAST];
    int32_t dst_ls;
    uint32_t vec;                        // every pointer and linesize of the frame is a multiple of 16
    uint32_t _pad[2];
};

struct KeyJob {                          // one noisy (frame, layer) of k_key_draw
    uint32_t st[31];                     // the rand() window at its first draw
    uint32_t noisekey;
    uint32_t *bits;
};

struct KeyClip {                         // the clip forms: the ring behind the records
    uint8_t *const *ring;
    int32_t ring_ls, ri, delay, T;
};

// ---- k_key_draw -----------------------------------------------------------------------------------------------
// (this kernel's starting window is the job's, the same for every lane: the compiler keeps it in scalar registers and
//  folds it into v_mul_lo_u32 as such.  The one-instruction product of the simulator's kernels takes vector operands
//  only -- 100 registers here instead of 66 -- and was not measured in this kernel, which keeps the form it has)
#define NTSC_JUMP61_MUL_ADD
#include "lane_rand.hpp"   // LaneRand, jump61 (shared with the simulator's kernels)

__global__ __launch_bounds__(KEY_DRAW_THREADS) void k_key_draw(const KeyJob *__restrict__ jobs, const uint32_t *__restrict__ polys,
                                                               uint32_t lanes)
{
    __shared__ uint32_t ring[31 * 64];
    const int lane = threadIdx.x;
    const uint32_t j = blockIdx.x * KEY_DRAW_THREADS + lane;
    const uint32_t jj = j < lanes ? j : lanes - 1;   // surplus lanes of the last wave repeat its last run and store nothing
    const KeyJob &job = jobs[blockIdx.y];
    uint32_t w[61], c[31], st[31];
#pragma unroll
    for (int i = 0; i < 31; i++) w[i] = job.st[i];
#pragma unroll
    for (int i = 31; i < 61; i++) w[i] = w[i - 31] + w[i - 3];
#pragma unroll
    for (int k = 0; k < 31; k++) c[k] = polys[(size_t)k * lanes + jj];
    jump61(c, w, st);
#pragma unroll
    for (int i = 0; i < 31; i++) ring[i * 64 + lane] = st[i];
    LaneRand g;
    g.p3 = st[28]; g.p2 = st[29]; g.p1 = st[30];
    g.slot = 0;
    const uint32_t nk = job.noisekey;
    uint32_t *out = job.bits + (size_t)jj * KEY_RUN_WORDS;
#pragma unroll 1
    for (int wi = 0; wi < KEY_RUN_WORDS; wi++) {
        uint32_t word = 0;
#pragma unroll 4
        for (int b = 0; b < 32; b++) {
            const uint32_t r1 = g.next(ring, lane), r2 = g.next(ring, lane), r3 = g.next(ring, lane);   // :861
            const uint32_t x = (r1 * r2 * r3) % 20001u;                                                  // :862
            word |= (x < nk ? 1u : 0u) << b;                                                             // :863
        }
        if (j < lanes) gst(out + wi, word);
    }
}

// ---- the pixel kernels ----------------------------------------------------------------------------------------

KDEV int key_dist(uint32_t px, uint32_t color)                                   // :854-857
{
    int dR = (int)((px >> 16) & 0xFF); dR -= (int)((color >> 16) & 0xFF);
    int dG = (int)((px >> 8) & 0xFF);  dG -= (int)((color >> 8) & 0xFF);
    int dB = (int)(px & 0xFF);         dB -= (int)(color & 0xFF);
    return abs(dR) + abs(dG) + abs(dB);
}

KDEV uint32_t key_fade(uint32_t px, uint32_t fade)                               // :869-873, unsigned throughout
{
    const uint32_t f = 256u - fade;
    const uint32_t r = (((px >> 16) & 0xFF) * f) >> 8;
    const uint32_t g = (((px >> 8) & 0xFF) * f) >> 8;
    const uint32_t b = ((px & 0xFF) * f) >> 8;
    return (r << 16) + (g << 8) + b;
}

// any hit bit in [a, b), a < b
KDEV bool key_any(const uint32_t *__restrict__ bits, uint32_t a, uint32_t b)
{
    const uint32_t wa = a >> 5, wb = (b - 1) >> 5;
    const uint32_t first = ~0u << (a & 31), last = ~0u >> (31 - ((b - 1) & 31));
    if (wa == wb) return (gld(bits + wa) & first & last) != 0;
    uint32_t any = gld(bits + wa) & first;
    for (uint32_t w = wa + 1; w < wb; w++) any |= gld(bits + w);
    any |= gld(bits + wb) & last;
    return any != 0;
}

// What a lane holds of one layer's source: its 4 pixels, and the pixel its hold group started at when that lies left of
// the quad (xdivc of the lane's first pixel is not 0).
struct KeyPx { uint32_t s[4], left; };

// xdivc at pixel x: 0 at the row start :847, back to 0 every xdivr pixels :883
KDEV uint32_t key_xdivc(uint32_t xdivr, int x) { return xdivr > 1 ? (uint32_t)x % xdivr : 0; }

// all loads of one layer's source for one quad; VEC: one 16-byte load
template <bool VEC>
KDEV void key_load_src(KeyPx &v, const uint8_t *__restrict__ srow, int x, uint32_t r0, int npx)
{
    px4_load<VEC>(v.s, srow + (size_t)x * 4u, npx);
    v.left = gld(srow + (size_t)((uint32_t)x - r0) * 4u);      // r0 == 0: the quad's own first pixel, not used
}

// One layer on the pixels x .. x + npx - 1 of a row: d[] the destination pixels, v the layer's source, r0 = xdivc at x,
// bits the layer's hit bits or NULL, rowbit the bit index of the row's first pixel.  The loop is the tool's own.
template <bool NOISE>
KDEV void key_layer(uint32_t (&d)[4], const KeyPx &v, int npx, const KeyCfgLayer &c, uint32_t r0, const uint32_t *__restrict__ bits,
                    uint32_t rowbit, int x)
{
    const uint32_t xd = c.xdivr;
    uint32_t r = r0;
    uint32_t hits = 0;
    if (NOISE && bits) {
        const uint32_t i = rowbit + (uint32_t)x;
        const uint64_t two = (uint64_t)gld(bits + (i >> 5)) | ((uint64_t)gld(bits + (i >> 5) + 1) << 32);
        hits = (uint32_t)(two >> (i & 31)) & 15u;
    }
    int dist = 0;
    if (r != 0) {                                                                // the group started left of this quad: d is held
        dist = key_dist(v.left, c.color);
        if (NOISE && bits && key_any(bits, rowbit + (uint32_t)x - r, rowbit + (uint32_t)x)) dist = 0xFFFF;
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        if (p < npx) {
            if (r == 0) dist = key_dist(v.s[p], c.color);                        // :853-858
            if (NOISE && ((hits >> p) & 1u)) dist = 0xFFFF;                      // :860-864
            if (c.fade != 0) d[p] = key_fade(d[p], c.fade);                      // :866-874
            const bool copy = c.invert ? dist < c.thr : dist >= c.thr;           // :876-881
            if (copy) d[p] = v.s[p];
            if (++r >= xd) r = 0;                                                // :883
        }
    }
}

// fast forms: the sources of one frame.  The record's pointers and linesizes are read first, then every vector load is
// issued: the layers' sources are independent of each other and of the destination.
template <bool VEC>
KDEV void key_load_fast(KeyPx (&v)[KEY_FAST], const KeyRec &r, int nl, const uint32_t (&r0)[KEY_FAST], int y, int x, int npx)
{
    const uint8_t *row[KEY_FAST];
#pragma unroll
    for (int k = 0; k < KEY_FAST; k++) row[k] = k < nl && r.src[k] ? r.src[k] + (size_t)y * (size_t)r.src_ls[k] : nullptr;
#pragma unroll
    for (int k = 0; k < KEY_FAST; k++)
        if (row[k]) key_load_src<VEC>(v[k], row[k], x, r0[k], npx);
}

template <bool NOISE>
KDEV void key_apply_fast(uint32_t (&d)[4], const KeyPx (&v)[KEY_FAST], const KeyRec &r, const KeyCfg &cfg, int nl,
                         const uint32_t (&r0)[KEY_FAST], int W, int y, int x, int npx)
{
#pragma unroll
    for (int k = 0; k < KEY_FAST; k++)
        if (k < nl && r.src[k])
            key_layer<NOISE>(d, v[k], npx, cfg.l[k], r0[k], NOISE ? r.bits[k] : nullptr, (uint32_t)y * (uint32_t)W, x);
}

template <bool NOISE, bool VEC>
KDEV void key_apply_general(uint32_t (&d)[4], const KeyRec &r, const KeyCfgLayer *__restrict__ gcfg, int nl, int W, int y, int x, int npx)
{
    for (int k = 0; k < nl; k++) {
        const KeyLayerDev L = r.layers[k];
        if (!L.src) continue;
        const KeyCfgLayer c = gcfg[k];
        const uint32_t r0 = key_xdivc(c.xdivr, x);
        KeyPx v;
        key_load_src<VEC>(v, L.src + (size_t)y * (size_t)L.ls, x, r0, npx);
        key_layer<NOISE>(d, v, npx, c, r0, NOISE ? L.bits : nullptr, (uint32_t)y * (uint32_t)W, x);
    }
}

template <bool NOISE, bool VEC>
KDEV void key_item_fast(const KeyRec &r, const KeyCfg &cfg, int W, int nl, int y, int x, int npx)
{
    uint8_t *dp = r.dst + (size_t)y * (size_t)r.dst_ls + (size_t)x * 4u;
    uint32_t d[4], r0[KEY_FAST];
    KeyPx v[KEY_FAST];
#pragma unroll
    for (int k = 0; k < KEY_FAST; k++) r0[k] = key_xdivc(cfg.l[k].xdivr, x);
    px4_load<VEC>(d, dp, npx);
    key_load_fast<VEC>(v, r, nl, r0, y, x, npx);
    key_apply_fast<NOISE>(d, v, r, cfg, nl, r0, W, y, x, npx);
    px4_store<VEC>(dp, d, npx);
}

// <NOISE>: a present layer has noisekey > 0 and k_key_draw has left its hit bits
template <bool NOISE>
__global__ __launch_bounds__(KEY_THREADS) void k_key_fast(const KeyRec *__restrict__ recs, KeyCfg cfg, int W, int H, int nl)
{
    const KeyRec &r = recs[blockIdx.y];
    const int Q = (W + 3) >> 2, total = Q * H;
    for (int item = blockIdx.x * KEY_THREADS + threadIdx.x; item < total; item += gridDim.x * KEY_THREADS) {
        const int y = item / Q, x = (item - y * Q) << 2;
        const int npx = W - x < 4 ? W - x : 4;
        if (r.vec && npx == 4) key_item_fast<NOISE, true>(r, cfg, W, nl, y, x, 4);
        else key_item_fast<NOISE, false>(r, cfg, W, nl, y, x, npx);
    }
}

template <bool NOISE, bool VEC>
KDEV void key_item_general(const KeyRec &r, const KeyCfgLayer *__restrict__ gcfg, int W, int nl, int y, int x, int npx)
{
    uint8_t *dp = r.dst + (size_t)y * (size_t)r.dst_ls + (size_t)x * 4u;
    uint32_t d[4];
    px4_load<VEC>(d, dp, npx);
    key_apply_general<NOISE, VEC>(d, r, gcfg, nl, W, y, x, npx);
    px4_store<VEC>(dp, d, npx);
}

template <bool NOISE>
__global__ __launch_bounds__(KEY_THREADS) void k_key_general(const KeyRec *__restrict__ recs, const KeyCfgLayer *__restrict__ gcfg,
                                                             int W, int H, int nl)
{
    const KeyRec &r = recs[blockIdx.y];
    const int Q = (W + 3) >> 2, total = Q * H;
    for (int item = blockIdx.x * KEY_THREADS + threadIdx.x; item < total; item += gridDim.x * KEY_THREADS) {
        const int y = item / Q, x = (item - y * Q) << 2;
        const int npx = W - x < 4 ? W - x : 4;
        if (r.vec && npx == 4) key_item_general<NOISE, true>(r, gcfg, W, nl, y, x, 4);
        else key_item_general<NOISE, false>(r, gcfg, W, nl, y, x, npx);
    }
}

// The clip forms: blockIdx.y is a chain -- the frames t = chain, chain + delay, ... that share ring slot
// (ri + chain) % delay.  The destination quad is read from the ring once, written to recs[t].dst at every step and to
// the ring at the end.  The sources do not depend on the recurrence, so the fast form keeps the loads of the chain's next
// KEY_AHEAD frames in flight: KEY_AHEAD + 1 register buffers, the step loop unrolled over them so that no buffer is
// ever copied (a copy would wait for the loads it copies).
constexpr int KEY_AHEAD = 2;
constexpr int KEY_BUFS = KEY_AHEAD + 1;

// sources of one frame for the clip form: NL layers, no branch between the loads -- an absent layer reads the ring row
// instead (valid memory, a cache hit) and is skipped when the layers are applied
template <bool VEC, int NL>
KDEV void key_load_chain(KeyPx (&v)[NL], const KeyRec &r, const uint8_t *ringrow, const uint32_t (&r0)[NL], int y, int x)
{
    const uint8_t *row[NL];
#pragma unroll
    for (int k = 0; k < NL; k++) row[k] = r.src[k] ? r.src[k] + (size_t)y * (size_t)r.src_ls[k] : ringrow;
#pragma unroll
    for (int k = 0; k < NL; k++) key_load_src<VEC>(v[k], row[k], x, r0[k], VEC ? 4 : 1);
}

template <bool NOISE, bool VEC, int NL>
KDEV void key_chain_fast(const KeyRec *__restrict__ recs, const KeyClip &clip, uint8_t *ring, const KeyCfg &cfg, int W,
                         int chain, int y, int x)
{
    // VEC: the lane's 4 pixels; otherwise ONE pixel per lane (x counts pixels), so that neither form has a per-lane branch
    const uint8_t *ringrow = ring + (size_t)y * (size_t)clip.ring_ls;
    uint8_t *rp = ring + (size_t)y * (size_t)clip.ring_ls + (size_t)x * 4u;
    const int dl = clip.delay, T = clip.T, npx = VEC ? 4 : 1;
    uint32_t d[4], r0[NL];
    KeyPx v[KEY_BUFS][NL];
#pragma unroll
    for (int k = 0; k < NL; k++) r0[k] = key_xdivc(cfg.l[k].xdivr, x);
    px4_load<VEC>(d, rp, npx);
#pragma unroll
    for (int j = 0; j < KEY_AHEAD; j++)       // past the chain's end: a frame of the chain again, loaded and not used
        key_load_chain<VEC, NL>(v[j], recs[chain + j * dl < T ? chain + j * dl : chain], ringrow, r0, y, x);
    for (int t = chain; t < T; t += KEY_BUFS * dl) {
#pragma unroll
        for (int j = 0; j < KEY_BUFS; j++) {
            const int tj = t + j * dl;
            if (tj < T) {
                const int tp = tj + KEY_AHEAD * dl;
                // unconditional, so that the number of loads in flight behind this step's sources is the same on every
                // path and the wait in front of the step can leave them in flight
                key_load_chain<VEC, NL>(v[(j + KEY_AHEAD) % KEY_BUFS], recs[tp < T ? tp : tj], ringrow, r0, y, x);
                const KeyRec &r = recs[tj];
#pragma unroll
                for (int k = 0; k < NL; k++)
                    if (r.src[k])
                        key_layer<NOISE>(d, v[j][k], npx, cfg.l[k], r0[k], NOISE ? r.bits[k] : nullptr, (uint32_t)y * (uint32_t)W, x);
                px4_store<VEC>(r.dst + (size_t)y * (size_t)r.dst_ls + (size_t)x * 4u, d, npx);
            }
        }
    }
    px4_store<VEC>(rp, d, npx);
}

// <NOISE, NL>: NL = number of layers, 1 .. NTSCSIM_KEY_FAST_LAYERS
template <bool NOISE, int NL>
__global__ __launch_bounds__(KEY_THREADS) void k_key_clip_fast(const KeyRec *__restrict__ recs, KeyClip clip, KeyCfg cfg, int W, int H)
{
    const int chain = blockIdx.y;
    uint8_t *ring = clip.ring[(clip.ri + chain) % clip.delay];
    if (recs[0].vec != 0) {                  // every pointer and linesize of the clip is a multiple of 16
        const int Q = W >> 2, total = Q * H;
        for (int item = blockIdx.x * KEY_THREADS + threadIdx.x; item < total; item += gridDim.x * KEY_THREADS) {
            const int y = item / Q;
            key_chain_fast<NOISE, true, NL>(recs, clip, ring, cfg, W, chain, y, (item - y * Q) << 2);
        }
        const int rest = W & 3, total1 = rest * H;      // the last width % 4 pixels of every row, one per lane
        for (int item = blockIdx.x * KEY_THREADS + threadIdx.x; item < total1; item += gridDim.x * KEY_THREADS) {
            const int y = item / rest;
            key_chain_fast<NOISE, false, NL>(recs, clip, ring, cfg, W, chain, y, (W & ~3) + (item - y * rest));
        }
    } else {
        const int total = W * H;
        for (int item = blockIdx.x * KEY_THREADS + threadIdx.x; item < total; item += gridDim.x * KEY_THREADS) {
            const int y = item / W;
            key_chain_fast<NOISE, false, NL>(recs, clip, ring, cfg, W, chain, y, item - y * W);
        }
    }
}

template <bool NOISE, bool VEC>
KDEV void key_chain_general(const KeyRec *__restrict__ recs, const KeyClip &clip, uint8_t *ring, const KeyCfgLayer *__restrict__ gcfg,
                            int W, int nl, int chain, int y, int x, int npx)
{
    uint8_t *rp = ring + (size_t)y * (size_t)clip.ring_ls + (size_t)x * 4u;
    uint32_t d[4];
    px4_load<VEC>(d, rp, npx);
    for (int t = chain; t < clip.T; t += clip.delay) {
        const KeyRec &r = recs[t];
        key_apply_general<NOISE, VEC>(d, r, gcfg, nl, W, y, x, npx);
        px4_store<VEC>(r.dst + (size_t)y * (size_t)r.dst_ls + (size_t)x * 4u, d, npx);
    }
    px4_store<VEC>(rp, d, npx);
}

template <bool NOISE>
__global__ __launch_bounds__(KEY_THREADS) void k_key_clip_general(const KeyRec *__restrict__ recs, KeyClip clip,
                                                                  const KeyCfgLayer *__restrict__ gcfg, int W, int H, int nl)
{
    const int chain = blockIdx.y;
    uint8_t *ring = clip.ring[(clip.ri + chain) % clip.delay];
    const int Q = (W + 3) >> 2, total = Q * H;
    const bool allvec = recs[0].vec != 0;
    for (int item = blockIdx.x * KEY_THREADS + threadIdx.x; item < total; item += gridDim.x * KEY_THREADS) {
        const int y = item / Q, x = (item - y * Q) << 2;
        const int npx = W - x < 4 ? W - x : 4;
        if (allvec && npx == 4) key_chain_general<NOISE, true>(recs, clip, ring, gcfg, W, nl, chain, y, x, 4);
        else key_chain_general<NOISE, false>(recs, clip, ring, gcfg, W, nl, chain, y, x, npx);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------

struct KeySlot : RecordSlot {            // records and jobs of one launch, and its hit bits
    uint32_t *bits = nullptr;
    size_t bits_cap = 0;                 // words
};

struct KeyState {
    ntscsim_key_params prm;
    std::vector<KeyCfgLayer> cfg;
    bool any_noise = false;
    KeyCfgLayer *cfg_dev = nullptr;      // general forms
    uint32_t *polys_dev = nullptr;       // k_key_draw: x^(768 j), coefficient-major
    uint32_t lanes = 0;                  // draw lanes per noisy (frame, layer)
    size_t bits_limit = (size_t)128 << 20;   // hit bits of one launch, bytes (ntscsim_key_debug_set_bits_limit)
    RecordSlots<KeySlot> slots;
    // the rand() window of the last job, and x^n of the distances met so far: consecutive jobs are a fixed distance apart
    bool have_state = false;
    uint64_t state_pos = 0;
    RandState state;
    std::map<uint64_t, RandPoly> deltas;
    FrameArena frames;                   // ntscsim_key_frames_host()
    LayerGeom geom() const { return LayerGeom{prm.width, prm.height, prm.n_layers}; }
};

void key_state_destroy(KeyState *k)
{
    if (!k) return;
    if (k->cfg_dev) (void)hipFree(k->cfg_dev);
    if (k->polys_dev) (void)hipFree(k->polys_dev);
    for (KeySlot &s : k->slots.slot)
        if (s.bits) (void)hipFree(s.bits);
    k->slots.release();
    k->frames.release();
    delete k;
}

} // namespace ntscsim

using namespace ntscsim;

extern "C" int ntscsim_key_bind(ntscsim_ctx *c, const ntscsim_key_params *p)
{
    if (!c || !p || p->struct_size != sizeof(*p) || p->n_layers < 0 || (p->n_layers > 0 && !p->layers)) return NTSCSIM_E_ARG;
    if (p->delay < 1 || p->delay > 256) return NTSCSIM_E_PARAM;                 // :652-655
    if (p->width < 1 || p->height < 1 || p->width > (1 << 16) || p->height > (1 << 16) ||
        (uint64_t)p->width * (uint64_t)p->height >= (1ull << 31)) return NTSCSIM_E_SIZE;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    KeyState *k = *v.key;
    if (!k) {
        k = new (std::nothrow) KeyState();
        if (!k) return NTSCSIM_E_NOMEM;
        *v.key = k;
    }
    const int rc = k->slots.wait_all(v);                                        // launches in flight read the layer settings and the polynomials
    if (rc != NTSCSIM_OK) return rc;
    k->prm = *p;
    k->prm.layers = nullptr;
    k->prm.output_path = nullptr;
    k->prm.layers_cap = 0;
    k->cfg.clear();
    k->any_noise = false;
    for (int l = 0; l < p->n_layers; l++) {
        const ntscsim_key_layer &L = p->layers[l];
        k->cfg.push_back(KeyCfgLayer{L.color, L.threshhold, L.fade, L.xdivr, L.invert != 0 ? 1u : 0u, L.noisekey});
        if (L.noisekey > 0) k->any_noise = true;
    }
    if (k->cfg_dev) { (void)hipFree(k->cfg_dev); k->cfg_dev = nullptr; }
    if (k->polys_dev) { (void)hipFree(k->polys_dev); k->polys_dev = nullptr; }
    if (p->n_layers > 0) {
        STAGECHK(v, hipMalloc((void **)&k->cfg_dev, k->cfg.size() * sizeof(KeyCfgLayer)));
        STAGECHK(v, hipMemcpy(k->cfg_dev, k->cfg.data(), k->cfg.size() * sizeof(KeyCfgLayer), hipMemcpyHostToDevice));
    }
    k->lanes = key_lanes_per_job(p->width, p->height);
    if (k->any_noise) {
        std::vector<uint32_t> polys;
        key_lane_polys(k->lanes, polys);
        STAGECHK(v, hipMalloc((void **)&k->polys_dev, polys.size() * sizeof(uint32_t)));
        STAGECHK(v, hipMemcpy(k->polys_dev, polys.data(), polys.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    k->have_state = false;
    return NTSCSIM_OK;
}

namespace {

// the rand() window at `pos`: from the last one by the polynomial of the distance where that is ahead of it
const RandState &key_state_at(KeyState *k, uint64_t pos)
{
    if (k->have_state && pos >= k->state_pos) {
        const uint64_t d = pos - k->state_pos;
        if (d != 0) {
            auto it = k->deltas.find(d);
            if (it == k->deltas.end()) {
                if (k->deltas.size() > 64) k->deltas.clear();
                it = k->deltas.emplace(d, rand_poly_pow(d)).first;
            }
            k->state = rand_state_apply(it->second, k->state);
        }
    } else k->state = rand_state_at(pos);
    k->have_state = true;
    k->state_pos = pos;
    return k->state;
}

// One pixel launch (with k_key_draw in front where a present layer draws) over descriptors that do not depend on each
// other, or -- clip != NULL -- over the frames of a clip, whose chains the kernel itself walks in order.
int key_launch(ntscsim_ctx *c, const ntscsim_key_desc *descs, int n, const KeyClip *clip, void *const *ring_host, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    KeyState *k = *v.key;
    const int W = k->prm.width, H = k->prm.height, nl = k->prm.n_layers;
    const bool general = nl > KEY_FAST || (clip && nl == 0);    // the fast clip form is instantiated for 1 .. 4 layers
    const size_t job_words = (size_t)k->lanes * KEY_RUN_WORDS + KEY_RUN_WORDS;   // the pixel kernel reads one word past a quad's
    size_t njobs = 0;
    for (int i = 0; i < n; i++)
        for (int l = 0; l < nl; l++)
            if (descs[i].layers[l].src_dev && k->cfg[(size_t)l].noisekey > 0) njobs++;
    const bool noise = njobs > 0;

    // records | layer lists (general) | jobs | ring pointers (clip) go up through a pinned slot of their own
    const size_t rec_bytes = (size_t)n * sizeof(KeyRec);
    const size_t lay_bytes = general ? (size_t)n * (size_t)nl * sizeof(KeyLayerDev) : 0;
    const size_t job_bytes = njobs * sizeof(KeyJob);
    const size_t ring_bytes = clip ? (size_t)clip->delay * sizeof(uint8_t *) : 0;
    const size_t bytes = rec_bytes + lay_bytes + job_bytes + ring_bytes;
    KeySlot *slot = nullptr;
    const int rc = k->slots.acquire(v, bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    KeySlot &s = *slot;
    if (njobs * job_words > s.bits_cap) {
        if (s.bits) { (void)hipFree(s.bits); s.bits = nullptr; }
        s.bits_cap = 0;
        const size_t want = njobs * job_words + njobs * job_words / 4;
        STAGECHK(v, hipMalloc((void **)&s.bits, want * sizeof(uint32_t)));
        s.bits_cap = want;
    }
    KeyRec *recs = reinterpret_cast<KeyRec *>(s.host);
    KeyLayerDev *lays = reinterpret_cast<KeyLayerDev *>(s.host + rec_bytes);
    KeyJob *jobs = reinterpret_cast<KeyJob *>(s.host + rec_bytes + lay_bytes);
    uint8_t **ringp = reinterpret_cast<uint8_t **>(s.host + rec_bytes + lay_bytes + job_bytes);
    const KeyLayerDev *lays_dev = reinterpret_cast<const KeyLayerDev *>(s.dev + rec_bytes);
    const KeyJob *jobs_dev = reinterpret_cast<const KeyJob *>(s.dev + rec_bytes + lay_bytes);

    uintptr_t allbits = 0;
    if (clip) {
        allbits |= (uintptr_t)clip->ring_ls;
        for (int i = 0; i < clip->delay; i++) { ringp[i] = static_cast<uint8_t *>(ring_host[i]); allbits |= (uintptr_t)ring_host[i]; }
    }
    size_t job_at = 0;
    for (int i = 0; i < n; i++) {
        const ntscsim_key_desc &d = descs[i];
        KeyRec &r = recs[i];
        std::memset(&r, 0, sizeof(r));
        r.dst = static_cast<uint8_t *>(d.dst_dev);
        r.dst_ls = d.dst_linesize;
        uintptr_t bits = (uintptr_t)d.dst_dev | (uintptr_t)d.dst_linesize;
        uint64_t pos = d.rand_pos;
        for (int l = 0; l < nl; l++) {
            const ntscsim_key_src &sl = d.layers[l];
            const uint32_t *hit = nullptr;
            if (sl.src_dev) {
                bits |= (uintptr_t)sl.src_dev | (uintptr_t)sl.src_linesize;
                if (k->cfg[(size_t)l].noisekey > 0) {
                    KeyJob &j = jobs[job_at];
                    std::memcpy(j.st, key_state_at(k, pos).w, sizeof(j.st));
                    j.noisekey = k->cfg[(size_t)l].noisekey;
                    j.bits = s.bits + job_at * job_words;
                    hit = j.bits;
                    job_at++;
                    pos += 3ull * (uint64_t)W * (uint64_t)H;
                }
            }
            if (general) {
                KeyLayerDev &L = lays[(size_t)i * (size_t)nl + (size_t)l];
                L.src = static_cast<const uint8_t *>(sl.src_dev);
                L.bits = hit;
                L.ls = sl.src_linesize;
                L._pad = 0;
            } else {
                r.src[l] = static_cast<const uint8_t *>(sl.src_dev);
                r.bits[l] = hit;
                r.src_ls[l] = sl.src_linesize;
            }
        }
        if (general) r.layers = lays_dev + (size_t)i * (size_t)nl;
        r.vec = (bits & 15) == 0;
        allbits |= bits;
    }
    if (clip)
        for (int i = 0; i < n; i++) recs[i].vec = (allbits & 15) == 0;
    STAGECHK(v, hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, st));

    if (noise) {
        for (size_t at = 0; at < njobs; at += 65535) {
            const dim3 grid((k->lanes + KEY_DRAW_THREADS - 1) / KEY_DRAW_THREADS, (unsigned)std::min<size_t>(65535, njobs - at));
            hipLaunchKernelGGL(k_key_draw, grid, dim3(KEY_DRAW_THREADS), 0, st, jobs_dev + at, k->polys_dev, k->lanes);
        }
        const int drc = stage_launched(v, nullptr, st, "k_key_draw");                // the slot stays with the kernel below
        if (drc != NTSCSIM_OK) return drc;
    }

    KeyCfg cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    for (int l = 0; l < nl && l < KEY_FAST; l++) cfg.l[l] = k->cfg[(size_t)l];
    const KeyRec *recs_dev = reinterpret_cast<const KeyRec *>(s.dev);
    const long long slices = ((long long)((W + 3) / 4) * H + KEY_THREADS - 1) / KEY_THREADS;
    const dim3 block(KEY_THREADS);
    if (clip) {
        KeyClip cd = *clip;
        cd.ring = reinterpret_cast<uint8_t *const *>(s.dev + rec_bytes + lay_bytes + job_bytes);
        const dim3 grid((unsigned)slices, (unsigned)std::min(clip->delay, clip->T));
        if (general) {
            if (noise) hipLaunchKernelGGL(k_key_clip_general<true>, grid, block, 0, st, recs_dev, cd, k->cfg_dev, W, H, nl);
            else hipLaunchKernelGGL(k_key_clip_general<false>, grid, block, 0, st, recs_dev, cd, k->cfg_dev, W, H, nl);
        } else {
#define KEY_CLIP_LAUNCH(N)                                                                                          \
    do {                                                                                                            \
        if (noise) hipLaunchKernelGGL((k_key_clip_fast<true, N>), grid, block, 0, st, recs_dev, cd, cfg, W, H);     \
        else hipLaunchKernelGGL((k_key_clip_fast<false, N>), grid, block, 0, st, recs_dev, cd, cfg, W, H);          \
    } while (0)
            switch (nl) {
            case 1: KEY_CLIP_LAUNCH(1); break;
            case 2: KEY_CLIP_LAUNCH(2); break;
            case 3: KEY_CLIP_LAUNCH(3); break;
            default: KEY_CLIP_LAUNCH(4); break;
            }
#undef KEY_CLIP_LAUNCH
        }
    } else {
        // a short call still spreads over the machine: about 8192 workgroups in all
        const long long per = std::max(1LL, std::min(slices, (8192LL + n - 1) / n));
        const dim3 grid((unsigned)per, (unsigned)n);
        if (general) {
            if (noise) hipLaunchKernelGGL(k_key_general<true>, grid, block, 0, st, recs_dev, k->cfg_dev, W, H, nl);
            else hipLaunchKernelGGL(k_key_general<false>, grid, block, 0, st, recs_dev, k->cfg_dev, W, H, nl);
        } else {
            if (noise) hipLaunchKernelGGL(k_key_fast<true>, grid, block, 0, st, recs_dev, cfg, W, H, nl);
            else hipLaunchKernelGGL(k_key_fast<false>, grid, block, 0, st, recs_dev, cfg, W, H, nl);
        }
    }
    std::string name = clip ? (general ? "k_key_clip_general<" : "k_key_clip_fast<") : (general ? "k_key_general<" : "k_key_fast<");
    name += noise ? "true" : "false";
    if (clip && !general) name += "," + std::to_string(nl);
    return stage_launched(v, &s, st, name + ">");
}

// frames a launch may carry: the hit bits of one launch stay below the limit (128 MiB), one frame at the least
int key_frames_per_launch(const KeyState *k)
{
    int noisy = 0;
    for (const KeyCfgLayer &l : k->cfg) noisy += l.noisekey > 0;
    if (!noisy) return 65535;
    const size_t per = (size_t)noisy * ((size_t)k->lanes * KEY_RUN_WORDS + KEY_RUN_WORDS) * sizeof(uint32_t);
    return (int)std::max<size_t>(1, std::min<size_t>(65535, k->bits_limit / per));
}

} // namespace

extern "C" int ntscsim_key_debug_set_bits_limit(ntscsim_ctx *c, size_t bytes)
{
    if (!c) return NTSCSIM_E_ARG;
    KeyState *k = *ctx_stage_view(c).key;
    if (!k) return NTSCSIM_E_ARG;                                               // ntscsim_key_bind() first
    k->bits_limit = bytes ? bytes : (size_t)128 << 20;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_key_frames_device(ntscsim_ctx *c, const ntscsim_key_desc *descs, int n, void *hip_stream)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    KeyState *k = *v.key;
    if (!k) return NTSCSIM_E_ARG;                                               // ntscsim_key_bind() first
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream;
    return layer_frames_in_order(k->geom(), descs, n, key_frames_per_launch(k),
                                 [&](const ntscsim_key_desc *d, int m) { return key_launch(c, d, m, nullptr, nullptr, st); });
}

extern "C" int ntscsim_key_clip_device(ntscsim_ctx *c, void *const *ring_dev, int ring_linesize, int32_t *ring_index,
                                       const void *const *src_dev, const int32_t *src_linesize, void *const *out_dev,
                                       int out_linesize, int T, uint64_t *rand_pos, void *hip_stream)
{
    if (!c || !ring_dev || !ring_index || !rand_pos || T < 0 || (T > 0 && !out_dev)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    KeyState *k = *v.key;
    if (!k) return NTSCSIM_E_ARG;
    const int W = k->prm.width, H = k->prm.height, nl = k->prm.n_layers, delay = k->prm.delay;
    if (nl > 0 && (!src_dev || !src_linesize)) return NTSCSIM_E_ARG;
    if (*ring_index < 0 || *ring_index >= delay) return NTSCSIM_E_ARG;
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    std::vector<ntscsim_key_desc> descs;
    std::vector<ntscsim_key_src> lays;
    const int rc = layer_clip_descs(k->geom(), delay, ring_dev, ring_linesize, src_dev, src_linesize, out_dev, out_linesize, T, false, descs, lays);
    if (rc != NTSCSIM_OK) return rc;
    uint64_t pos = *rand_pos;
    for (int t = 0; t < T; t++) {
        descs[(size_t)t].rand_pos = pos;
        for (int l = 0; l < nl; l++)
            if (lays[(size_t)t * (size_t)nl + (size_t)l].src_dev && k->cfg[(size_t)l].noisekey > 0) pos += 3ull * (uint64_t)W * (uint64_t)H;
    }
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream;
    // one launch for the whole clip, or one per run of frames whose hit bits fit the bound: the ring carries over
    const int cap = key_frames_per_launch(k);
    int ri = *ring_index;
    std::string names;
    for (int at = 0; at < T; at += cap) {
        const int m = std::min(cap, T - at);
        const KeyClip clip{nullptr, ring_linesize, ri, delay, m};
        v.kernels->clear();
        const int lrc = key_launch(c, descs.data() + at, m, &clip, ring_dev, st);
        if (lrc != NTSCSIM_OK) return lrc;
        if (names.empty()) names = *v.kernels;
        ri = (int)(((long long)ri + m) % delay);
    }
    *v.kernels = names;
    *ring_index = ri;
    *rand_pos = pos;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_key_frames_host(ntscsim_ctx *c, const ntscsim_key_desc *descs, int n)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    KeyState *k = *v.key;
    if (!k) return NTSCSIM_E_ARG;
    return layer_frames_host(v, k->frames, k->geom(), descs, n,
                             [&](const ntscsim_key_desc *d, int m, hipStream_t st) { return ntscsim_key_frames_device(c, d, m, st); });
}
