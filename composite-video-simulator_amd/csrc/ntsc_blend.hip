// ntsc_blend.hip -- device half of the frameblend stage (include/ntscsim.h: ntscsim_blend_*): the pixel loops of
// frameblend.cpp:1032-1081 as one launch over any number of output frames.
//
// One lane = 4 pixels = one 16-byte load per tap and one 16-byte store (frames whose pointers and linesizes are all
// multiples of 16; any other frame, and the last width % 4 pixels of a row, move as dwords).  The gamma tables live in
// LDS -- dec as 256 x u16, enc as 8193 x u8, 8.7 KiB -- filled once per workgroup, and a workgroup walks several
// 256-quad slices of its frame so that the fill is small against the pixels it serves.  The sums are 32-bit while
// 8192 * sum(weight16) < 2^32 (255 * sum without gamma), which the host checks per descriptor, and 64-bit otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "ntscsim.h"
#include "ntsc_frames.hpp"
#include "ntsc_stage.hpp"

namespace ntscsim {

struct BlendTapDev {                     // general form: the tap lists, in device memory behind the records
    const uint8_t *src;
    int32_t ls;
    uint32_t w;
};

struct BlendRec {
    uint8_t *dst;
    const uint8_t *src[NTSCSIM_BLEND_FAST_TAPS];   // fast form
    const BlendTapDev *taps;                       // general form
    int32_t src_ls[NTSCSIM_BLEND_FAST_TAPS];
    uint32_t w[NTSCSIM_BLEND_FAST_TAPS];
    int32_t dst_ls, W, H, ntaps;
    uint32_t vec;                        // every pointer and linesize of the frame is a multiple of 16
    uint32_t _pad[3];
};

constexpr int BLEND_THREADS = 256;
constexpr int ENC_WORDS = (8193 + 3) / 4;          // enc[] padded to whole dwords: 8196 bytes

template <bool GAMMA, typename ACC>
__device__ __forceinline__ void blend_add(uint32_t px, uint32_t w, ACC acc[3], const uint16_t *dec)
{
    const uint32_t b = px & 255u, g = (px >> 8) & 255u, r = (px >> 16) & 255u;
    acc[0] += (ACC)(GAMMA ? (uint32_t)dec[b] : b) * w;        // :1043-1045 / :1068-1070
    acc[1] += (ACC)(GAMMA ? (uint32_t)dec[g] : g) * w;
    acc[2] += (ACC)(GAMMA ? (uint32_t)dec[r] : r) * w;
}

template <bool GAMMA, typename ACC>
__device__ __forceinline__ uint32_t blend_pack(const ACC acc[3], const uint8_t *enc)
{
    uint32_t o[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const ACC v = acc[c] >> 16;
        if (GAMMA) o[c] = enc[v > (ACC)8192 ? 8192u : (uint32_t)v];        // gamma_enc16() :716-722
        else o[c] = v > (ACC)255 ? 255u : (uint32_t)v;                     // clamp255() :685-691
    }
    return o[0] | (o[1] << 8) | (o[2] << 16) | 0xFF000000u;                // :1048-1051
}

template <bool GAMMA, bool WIDE, bool GENERAL>
__device__ __forceinline__ void blend_body(const BlendRec *__restrict__ recs, const uint16_t *__restrict__ gdec,
                                           const uint32_t *__restrict__ genc)
{
    typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type ACC;
    __shared__ uint16_t dec[GAMMA ? 256 : 1];
    __shared__ uint32_t encw[GAMMA ? ENC_WORDS : 1];
    if (GAMMA) {
        if (threadIdx.x < 256) dec[threadIdx.x] = gdec[threadIdx.x];
        for (int i = threadIdx.x; i < ENC_WORDS; i += BLEND_THREADS) encw[i] = genc[i];
        __syncthreads();
    }
    const uint8_t *enc = reinterpret_cast<const uint8_t *>(encw);
    const BlendRec &r = recs[blockIdx.y];
    const int W = r.W, nt = r.ntaps;
    const int Q = (W + 3) >> 2;
    const int total = Q * r.H;
    for (int item = blockIdx.x * BLEND_THREADS + threadIdx.x; item < total; item += gridDim.x * BLEND_THREADS) {
        const int y = item / Q;
        const int x = (item - y * Q) << 2;
        const int npx = W - x < 4 ? W - x : 4;
        uint8_t *drow = r.dst + (size_t)y * (size_t)r.dst_ls + (size_t)x * 4u;
        if (r.vec && npx == 4) {
            ACC acc[4][3] = {};
            if (GENERAL) {
                for (int k = 0; k < nt; k++) {
                    const BlendTapDev t = r.taps[k];
                    if (t.w == 0) continue;
                    const uint4 v = *reinterpret_cast<const uint4 *>(t.src + (size_t)y * (size_t)t.ls + (size_t)x * 4u);
                    blend_add<GAMMA, ACC>(v.x, t.w, acc[0], dec);
                    blend_add<GAMMA, ACC>(v.y, t.w, acc[1], dec);
                    blend_add<GAMMA, ACC>(v.z, t.w, acc[2], dec);
                    blend_add<GAMMA, ACC>(v.w, t.w, acc[3], dec);
                }
            } else {
                uint4 v[NTSCSIM_BLEND_FAST_TAPS];
#pragma unroll
                for (int k = 0; k < NTSCSIM_BLEND_FAST_TAPS; k++)       // all loads first: the taps are independent
                    if (k < nt && r.w[k] != 0)
                        v[k] = *reinterpret_cast<const uint4 *>(r.src[k] + (size_t)y * (size_t)r.src_ls[k] + (size_t)x * 4u);
#pragma unroll
                for (int k = 0; k < NTSCSIM_BLEND_FAST_TAPS; k++)
                    if (k < nt && r.w[k] != 0) {
                        blend_add<GAMMA, ACC>(v[k].x, r.w[k], acc[0], dec);
                        blend_add<GAMMA, ACC>(v[k].y, r.w[k], acc[1], dec);
                        blend_add<GAMMA, ACC>(v[k].z, r.w[k], acc[2], dec);
                        blend_add<GAMMA, ACC>(v[k].w, r.w[k], acc[3], dec);
                    }
            }
            uint4 o;
            o.x = blend_pack<GAMMA, ACC>(acc[0], enc);
            o.y = blend_pack<GAMMA, ACC>(acc[1], enc);
            o.z = blend_pack<GAMMA, ACC>(acc[2], enc);
            o.w = blend_pack<GAMMA, ACC>(acc[3], enc);
            *reinterpret_cast<uint4 *>(drow) = o;
        } else {
            for (int p = 0; p < npx; p++) {                              // dword form
                ACC acc[3] = {};
                for (int k = 0; k < nt; k++) {
                    const uint8_t *s;
                    int ls;
                    uint32_t w;
                    if (GENERAL) { const BlendTapDev t = r.taps[k]; s = t.src; ls = t.ls; w = t.w; }
                    else { s = r.src[k & (NTSCSIM_BLEND_FAST_TAPS - 1)]; ls = r.src_ls[k & (NTSCSIM_BLEND_FAST_TAPS - 1)]; w = r.w[k & (NTSCSIM_BLEND_FAST_TAPS - 1)]; }
                    if (w == 0) continue;
                    const uint32_t px = *reinterpret_cast<const uint32_t *>(s + (size_t)y * (size_t)ls + (size_t)(x + p) * 4u);
                    blend_add<GAMMA, ACC>(px, w, acc, dec);
                }
                *reinterpret_cast<uint32_t *>(drow + p * 4) = blend_pack<GAMMA, ACC>(acc, enc);
            }
        }
    }
}

// <GAMMA, WIDE>: gamma tables on / off, 64-bit / 32-bit sums
template <bool GAMMA, bool WIDE>
__global__ __launch_bounds__(BLEND_THREADS) void k_blend_fast(const BlendRec *recs, const uint16_t *gdec, const uint32_t *genc)
{
    blend_body<GAMMA, WIDE, false>(recs, gdec, genc);
}

template <bool GAMMA, bool WIDE>
__global__ __launch_bounds__(BLEND_THREADS) void k_blend_general(const BlendRec *recs, const uint16_t *gdec, const uint32_t *genc)
{
    blend_body<GAMMA, WIDE, true>(recs, gdec, genc);
}

// ---- host side -----------------------------------------------------------------------------------------------

struct BlendState {
    ntscsim_blend_params prm;
    bool gamma = false;
    uint16_t *dec_dev = nullptr;
    uint32_t *enc_dev = nullptr;
    unsigned char *tab_host = nullptr;   // pinned: 512 bytes dec + 8196 bytes enc
    RecordSlots<> slots;
    FrameArena frames;                   // ntscsim_blend_frames_host(): sources of the call + one chunk of outputs
};

void blend_state_destroy(BlendState *b)
{
    if (!b) return;
    if (b->dec_dev) (void)hipFree(b->dec_dev);
    if (b->enc_dev) (void)hipFree(b->enc_dev);
    if (b->tab_host) (void)hipHostFree(b->tab_host);
    b->slots.release();
    b->frames.release();
    delete b;
}

} // namespace ntscsim

using namespace ntscsim;

extern "C" int ntscsim_blend_bind(ntscsim_ctx *c, const ntscsim_blend_params *p)
{
    if (!c || !p || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    if (p->framealt < 1 || p->framealt > 8 || p->rate_num <= 0 || p->rate_den <= 0) return NTSCSIM_E_PARAM;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    BlendState *b = *v.blend;
    if (!b) {
        b = new (std::nothrow) BlendState();
        if (!b) return NTSCSIM_E_NOMEM;
        *v.blend = b;
    }
    const int wrc = b->slots.wait_all(v);                                       // launches in flight read the tables and their records
    if (wrc != NTSCSIM_OK) return wrc;
    b->prm = *p;
    b->prm.input_path = b->prm.output_path = nullptr;
    b->gamma = p->gamma_correction > 1;                                        // :1032
    if (b->gamma) {
        if (!b->dec_dev) STAGECHK(v, hipMalloc((void **)&b->dec_dev, 256 * sizeof(uint16_t)));
        if (!b->enc_dev) STAGECHK(v, hipMalloc((void **)&b->enc_dev, ENC_WORDS * 4));
        if (!b->tab_host) STAGECHK(v, hipHostMalloc((void **)&b->tab_host, 512 + ENC_WORDS * 4, hipHostMallocPortable));
        std::memset(b->tab_host, 0, 512 + ENC_WORDS * 4);
        const int rc = ntscsim_blend_tables(p->gamma_correction, (uint16_t *)b->tab_host, b->tab_host + 512);
        if (rc != NTSCSIM_OK) return rc;
        STAGECHK(v, hipMemcpy(b->dec_dev, b->tab_host, 512, hipMemcpyHostToDevice));
        STAGECHK(v, hipMemcpy(b->enc_dev, b->tab_host + 512, ENC_WORDS * 4, hipMemcpyHostToDevice));
    }
    return NTSCSIM_OK;
}

namespace {

template <bool GENERAL>
void launch_form(bool gamma, bool wide, dim3 grid, hipStream_t st, const BlendRec *recs, const uint16_t *dec, const uint32_t *enc)
{
    const dim3 block(BLEND_THREADS);
#define BLEND_LAUNCH(G, Wd)                                                                             \
    do {                                                                                                \
        if (GENERAL) hipLaunchKernelGGL((k_blend_general<G, Wd>), grid, block, 0, st, recs, dec, enc);  \
        else hipLaunchKernelGGL((k_blend_fast<G, Wd>), grid, block, 0, st, recs, dec, enc);             \
    } while (0)
    if (gamma && wide) BLEND_LAUNCH(true, true);
    else if (gamma) BLEND_LAUNCH(true, false);
    else if (wide) BLEND_LAUNCH(false, true);
    else BLEND_LAUNCH(false, false);
#undef BLEND_LAUNCH
}

// one launch of at most 65535 descriptors
int blend_launch(ntscsim_ctx *c, const ntscsim_blend_desc *descs, int n, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    BlendState *b = *v.blend;
    const uint64_t mul = b->gamma ? 8192u : 255u;
    bool general = false, wide = false;
    size_t n_taps_total = 0;
    long long max_items = 0;
    for (int i = 0; i < n; i++) {
        const ntscsim_blend_desc &d = descs[i];
        if (!d.dst_dev || d.n_taps < 0 || (d.n_taps > 0 && !d.taps)) return NTSCSIM_E_ARG;
        if (d.width <= 0 || d.height <= 0 || d.width > (1 << 16) || d.height > (1 << 16)) return NTSCSIM_E_SIZE;   // Q * H fits an int
        if (plane_check(d.dst_dev, d.dst_linesize, d.width, true)) return NTSCSIM_E_SIZE;
        uint64_t sum = 0;
        const Span ds = span_of(d.dst_dev, d.dst_linesize, d.height);
        for (int k = 0; k < d.n_taps; k++) {
            const ntscsim_blend_tap &t = d.taps[k];
            if (!t.src_dev) return NTSCSIM_E_ARG;
            if (plane_check(t.src_dev, t.src_linesize, d.width, true)) return NTSCSIM_E_SIZE;
            if (overlaps(ds, span_of(t.src_dev, t.src_linesize, d.height))) return NTSCSIM_E_ARG;   // a destination that is also a source
            sum += t.weight16;
            if (sum >= (1ull << 38)) return NTSCSIM_E_ARG;
        }
        if (mul * sum >= (1ull << 32)) wide = true;
        if (d.n_taps > NTSCSIM_BLEND_FAST_TAPS) general = true;
        n_taps_total += (size_t)d.n_taps;
        max_items = std::max(max_items, (long long)((d.width + 3) / 4) * d.height);
    }

    // records (and, for the general form, the tap lists behind them) go up through a pinned slot of their own
    const size_t rec_bytes = (size_t)n * sizeof(BlendRec);
    const size_t bytes = rec_bytes + (general ? n_taps_total * sizeof(BlendTapDev) : 0);
    RecordSlot *slot = nullptr;
    const int rc = b->slots.acquire(v, bytes, slot);
    if (rc != NTSCSIM_OK) return rc;
    RecordSlot &s = *slot;
    BlendRec *recs = reinterpret_cast<BlendRec *>(s.host);
    BlendTapDev *taps = reinterpret_cast<BlendTapDev *>(s.host + rec_bytes);
    const BlendTapDev *taps_dev = reinterpret_cast<const BlendTapDev *>(s.dev + rec_bytes);
    size_t tap_at = 0;
    for (int i = 0; i < n; i++) {
        const ntscsim_blend_desc &d = descs[i];
        BlendRec &r = recs[i];
        std::memset(&r, 0, sizeof(r));
        r.dst = static_cast<uint8_t *>(d.dst_dev);
        r.dst_ls = d.dst_linesize; r.W = d.width; r.H = d.height; r.ntaps = d.n_taps;
        uintptr_t bits = (uintptr_t)d.dst_dev | (uintptr_t)d.dst_linesize;
        for (int k = 0; k < d.n_taps; k++) {
            const ntscsim_blend_tap &t = d.taps[k];
            bits |= (uintptr_t)t.src_dev | (uintptr_t)t.src_linesize;
            if (general) {
                taps[tap_at + k].src = static_cast<const uint8_t *>(t.src_dev);
                taps[tap_at + k].ls = t.src_linesize;
                taps[tap_at + k].w = t.weight16;
            } else {
                r.src[k] = static_cast<const uint8_t *>(t.src_dev);
                r.src_ls[k] = t.src_linesize;
                r.w[k] = t.weight16;
            }
        }
        if (general) { r.taps = taps_dev + tap_at; tap_at += (size_t)d.n_taps; }
        r.vec = (bits & 15) == 0;
    }
    STAGECHK(v, hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, st));

    // a workgroup walks several 256-quad slices of its frame (the LDS fill is then small against its pixels), but a short
    // call still spreads over the machine: about 8192 workgroups in all
    const long long slices = (max_items + BLEND_THREADS - 1) / BLEND_THREADS;
    const long long per = std::max(1LL, std::min(slices, (8192LL + n - 1) / n));
    const dim3 grid((unsigned)per, (unsigned)n);
    if (general) launch_form<true>(b->gamma, wide, grid, st, reinterpret_cast<const BlendRec *>(s.dev), b->dec_dev, b->enc_dev);
    else launch_form<false>(b->gamma, wide, grid, st, reinterpret_cast<const BlendRec *>(s.dev), b->dec_dev, b->enc_dev);
    return stage_launched(v, &s, st, std::string(general ? "k_blend_general<" : "k_blend_fast<") + (b->gamma ? "true," : "false,") + (wide ? "true>" : "false>"));
}

} // namespace

extern "C" int ntscsim_blend_frames_device(ntscsim_ctx *c, const ntscsim_blend_desc *descs, int n, void *hip_stream)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    if (!*v.blend) return NTSCSIM_E_ARG;                                        // ntscsim_blend_bind() first
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream;
    for (int at = 0; at < n; at += 65535) {
        const int rc = blend_launch(c, descs + at, std::min(65535, n - at), st);
        if (rc != NTSCSIM_OK) return rc;
    }
    return NTSCSIM_OK;
}

extern "C" int ntscsim_blend_clip_device(ntscsim_ctx *c, const void *const *src_dev, int src_linesize,
                                         const double *frame_t, int n_src, void *const *dst_dev, int dst_linesize,
                                         int width, int height, int64_t first, int64_t last, void *hip_stream)
{
    if (!c || !src_dev || !frame_t || n_src <= 0 || first < 0 || last < first || (last > first && !dst_dev)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    BlendState *b = *v.blend;
    if (!b) return NTSCSIM_E_ARG;
    ntscsim_blend_plan *pl = nullptr;
    int rc = ntscsim_blend_plan_create(&b->prm, &pl);
    if (rc != NTSCSIM_OK) return rc;
    std::vector<ntscsim_blend_desc> descs;
    std::vector<ntscsim_blend_tap> taps;
    std::vector<size_t> tap_at;
    std::vector<int64_t> ids(16);
    std::vector<uint32_t> w16(16);
    int pushed = 0;
    ntscsim_blend_plan_push(pl, frame_t[pushed++]);                             // :904-907
    for (int64_t current = 0; current < last && rc == NTSCSIM_OK; current++) {
        while (pushed < n_src && frame_t[pushed - 1] < (double)(current + 30)) // the read-ahead :910-922
            ntscsim_blend_plan_push(pl, frame_t[pushed++]);
        int nt = 0;
        rc = ntscsim_blend_plan_next(pl, current, ids.data(), w16.data(), (int)ids.size(), &nt, nullptr);
        if (rc == NTSCSIM_E_SIZE) {
            ids.resize((size_t)nt); w16.resize((size_t)nt);
            rc = ntscsim_blend_plan_next(pl, current, ids.data(), w16.data(), nt, &nt, nullptr);
        }
        if (rc != NTSCSIM_OK || current < first) continue;
        ntscsim_blend_desc d;
        d.dst_dev = dst_dev[current - first];
        d.dst_linesize = dst_linesize; d.width = width; d.height = height; d.n_taps = nt; d.taps = nullptr;
        tap_at.push_back(taps.size());
        for (int k = 0; k < nt; k++)
            taps.push_back(ntscsim_blend_tap{src_dev[ids[(size_t)k]], src_linesize, w16[(size_t)k]});
        descs.push_back(d);
    }
    ntscsim_blend_plan_destroy(pl);
    if (rc != NTSCSIM_OK) return rc;
    for (size_t i = 0; i < descs.size(); i++) descs[i].taps = taps.data() + tap_at[i];
    return ntscsim_blend_frames_device(c, descs.data(), (int)descs.size(), hip_stream);
}

extern "C" int ntscsim_blend_frames_host(ntscsim_ctx *c, const ntscsim_blend_desc *descs, int n)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    BlendState *b = *v.blend;
    if (!b) return NTSCSIM_E_ARG;
    STAGECHK(v, hipSetDevice(v.device));
    const int CHUNK = 16;                // output frames per launch; staging holds as many frames
    auto pitch = [](int w) { return ((size_t)w * 4 + 15) & ~(size_t)15; };
    // distinct sources of the call (pointer + linesize + geometry) -> offset in the device arena
    struct Key { const void *p; int ls, w, h; bool operator<(const Key &o) const { return std::tie(p, ls, w, h) < std::tie(o.p, o.ls, o.w, o.h); } };
    std::map<Key, size_t> where;
    std::vector<Key> order;
    size_t src_bytes = 0, frame_max = 0, chunk_max = 0;
    for (int at = 0; at < n; at += CHUNK) {
        size_t cb = 0;
        for (int i = at; i < std::min(n, at + CHUNK); i++) {
            const ntscsim_blend_desc &d = descs[i];
            if (!d.dst_dev || d.n_taps < 0 || (d.n_taps > 0 && !d.taps)) return NTSCSIM_E_ARG;
            if (d.width <= 0 || d.height <= 0 || d.width > (1 << 16) || d.height > (1 << 16) || plane_check(d.dst_dev, d.dst_linesize, d.width, false)) return NTSCSIM_E_SIZE;
            const size_t fb = pitch(d.width) * (size_t)d.height;
            frame_max = std::max(frame_max, fb);
            cb += fb;
            for (int k = 0; k < d.n_taps; k++) {
                const ntscsim_blend_tap &t = d.taps[k];
                if (!t.src_dev) return NTSCSIM_E_ARG;
                if (plane_check(t.src_dev, t.src_linesize, d.width, false)) return NTSCSIM_E_SIZE;
                const Key key{t.src_dev, t.src_linesize, d.width, d.height};
                if (where.emplace(key, src_bytes).second) { order.push_back(key); src_bytes += fb; }
            }
        }
        chunk_max = std::max(chunk_max, cb);
    }
    if (n == 0) return NTSCSIM_OK;
    const size_t stage_bytes = std::max(chunk_max, frame_max * (size_t)CHUNK);
    FrameArena &fa = b->frames;
    const int arc = fa.reserve(v, src_bytes + chunk_max, stage_bytes);
    if (arc != NTSCSIM_OK) return arc;
    hipStream_t st = v.stream;
    // every source once: packed to 16-byte pitched rows in staging, up in runs that fill the staging buffer
    for (size_t i = 0; i < order.size();) {
        size_t fill = 0, j = i;
        const size_t run_at = where[order[i]];
        for (; j < order.size(); j++) {
            const Key &k = order[j];
            const size_t pb = pitch(k.w), fb = pb * (size_t)k.h;
            if (fill + fb > fa.staging_cap) break;
            copy_rows(fa.staging + fill, pb, k.p, (size_t)k.ls, (size_t)k.w * 4, k.h);
            fill += fb;
        }
        STAGECHK(v, hipMemcpyAsync(fa.arena + run_at, fa.staging, fill, hipMemcpyHostToDevice, st));
        STAGECHK(v, hipStreamSynchronize(st));
        i = j;
    }
    std::vector<ntscsim_blend_desc> dd;
    std::vector<ntscsim_blend_tap> tt;
    std::string names;
    for (int at = 0; at < n; at += CHUNK) {
        const int m = std::min(CHUNK, n - at);
        dd.assign(descs + at, descs + at + m);
        tt.clear();
        size_t ntap = 0;
        for (int i = 0; i < m; i++) ntap += (size_t)dd[i].n_taps;
        tt.reserve(ntap);
        size_t off = 0;
        for (int i = 0; i < m; i++) {
            ntscsim_blend_desc &d = dd[i];
            d.dst_dev = fa.arena + src_bytes + off;
            d.dst_linesize = (int)pitch(d.width);
            off += pitch(d.width) * (size_t)d.height;
            const ntscsim_blend_tap *first = tt.data() + tt.size();
            for (int k = 0; k < d.n_taps; k++) {
                const ntscsim_blend_tap &t = descs[at + i].taps[k];
                tt.push_back(ntscsim_blend_tap{fa.arena + where[Key{t.src_dev, t.src_linesize, d.width, d.height}], (int)pitch(d.width), t.weight16});
            }
            d.taps = first;
        }
        const int rc = ntscsim_blend_frames_device(c, dd.data(), m, st);
        if (rc != NTSCSIM_OK) return rc;
        if (names.empty()) names = *v.kernels;
        STAGECHK(v, hipMemcpyAsync(fa.staging, fa.arena + src_bytes, off, hipMemcpyDeviceToHost, st));
        STAGECHK(v, hipStreamSynchronize(st));
        off = 0;
        for (int i = 0; i < m; i++) {
            const ntscsim_blend_desc &d = descs[at + i];
            const size_t pb = pitch(d.width);
            copy_rows(d.dst_dev, (size_t)d.dst_linesize, fa.staging + off, pb, (size_t)d.width * 4, d.height);
            off += pb * (size_t)d.height;
        }
    }
    *v.kernels = names;
    return NTSCSIM_OK;
}
