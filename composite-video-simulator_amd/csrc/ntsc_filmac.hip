// ntsc_filmac.hip -- device half of the filmac stage (include/ntscsim.h: ntscsim_filmac_*): the film auto-contrast of
// filmac.cpp:857-1006 as a reduction, a short serial chain and a pixel map.  Line numbers refer to that file; the
// arithmetic itself is csrc/filmac_levels.hpp, which the kernels and the host code share.
//
// k_filmac_stats   grid (blocks of a frame, frames): one workgroup reduces one clipped 128 x 128 block of the picture's
//                  middle to {sum of min(B, G, R), pixels, largest byte}.
// k_filmac_frame_levels  grid (frames / 4): the frame levels from the block records, a wavefront per frame.
// k_filmac_levels  one workgroup per launch: the recurrence over the launch's frames walked by one lane on the
//                  device-resident state, the levels passing through LDS.
// k_filmac_tables  grid (frames): the 256-entry byte table of a frame, one 64-bit division per lane.
//                  Both were parts of k_filmac_levels at first; on its one CU they took longer than the walk itself
//                  (DESIGN.md section 7j has the numbers).
// k_filmac_apply   grid (bands of rows, frames): the frame's table in LDS, every B, G, R byte looked up, alpha 0xFF.
//
// The five run once per launch group, over all of its frames, so the level state never visits the host: a call of n
// frames that do not depend on each other is five launches.  
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ntscsim.h"
#include "filmac_levels.hpp"
#include "ntsc_frames.hpp"
#include "ntsc_px4.hpp"
#include "ntsc_stage.hpp"

namespace ntscsim {

#define FDEV __device__ __forceinline__

constexpr int FILMAC_THREADS = 256;
constexpr int FILMAC_WAVES = FILMAC_THREADS / 64;
constexpr int FILMAC_QUADS = FILMAC_BLOCK / 4;                 // 16-byte quads in a row of a block: 32, half a wavefront
constexpr int FILMAC_ROWS_PER_STEP = FILMAC_THREADS / FILMAC_QUADS;   // rows of a block the workgroup loads at once: 8
constexpr int FILMAC_FLIGHT = 8;                               // quads a lane requests before its first wait
constexpr int FILMAC_LEVEL_THREADS = 1024;
constexpr int FILMAC_CHUNK = 1024;                             // frames whose levels pass through LDS together
constexpr int FILMAC_BAND = 8;                                 // rows a workgroup of k_filmac_apply maps
constexpr int FILMAC_UNROLL = 4;                               // quads of the map a lane has in flight
static_assert(FILMAC_BLOCK % (FILMAC_ROWS_PER_STEP * FILMAC_FLIGHT) == 0, "a block is a whole number of flights");

struct FilmacRec {                       // one frame
    uint8_t *dst;
    const uint8_t *src;
    int32_t dst_ls, src_ls;
    uint32_t vec;                        // dst and dst_ls are multiples of 16
    uint32_t _pad;
};

struct FilmacTap { int64_t minv, maxv, final_minv, final_maxv; };   // ntscsim_filmac_debug_levels()

FDEV uint32_t min3(uint32_t p) { return min(min(p & 0xFFu, (p >> 8) & 0xFFu), (p >> 16) & 0xFFu); }
FDEV uint32_t max3(uint32_t p) { return max(max(p & 0xFFu, (p >> 8) & 0xFFu), (p >> 16) & 0xFFu); }

// GAMMA: the sum is of gamma_dec16 of the smallest byte (dec, 256 entries), otherwise of the byte itself
template <bool GAMMA>
__global__ __launch_bounds__(FILMAC_THREADS) void k_filmac_stats(const FilmacRec *__restrict__ recs, const uint16_t *__restrict__ dec,
                                                                 FilmacBlockRec *__restrict__ blocks, int W, int H)
{
    __shared__ uint16_t s_dec[256];
    __shared__ uint32_t s_sum[FILMAC_WAVES], s_top[FILMAC_WAVES];

    const FilmacRec &r = recs[blockIdx.y];
    const uint8_t *const src = r.src;
    const int src_ls = r.src_ls;
    const FilmacGrid g = filmac_grid(W, H);
    const FilmacBox box = filmac_box(g, W, H, (int)blockIdx.x);
    if (GAMMA) {
        s_dec[threadIdx.x] = dec[threadIdx.x];
        __syncthreads();
    }

    // lane -> quad q of row `row0 + step * 8` of the block; n: pixels of the quad inside the block (the frame)
    const int q = (int)(threadIdx.x % FILMAC_QUADS), row0 = (int)(threadIdx.x / FILMAC_QUADS);
    const int left = box.w - 4 * q, n = left < 0 ? 0 : left > 4 ? 4 : left;
    const uint8_t *const at = src + 4 * (size_t)(box.x + 4 * q);
    uint32_t sum = 0, top = 0;
    for (int y0 = row0; y0 < box.h; y0 += FILMAC_ROWS_PER_STEP * FILMAC_FLIGHT) {
        px4_u4 v[FILMAC_FLIGHT];
        // every load of the flight is requested before the first is looked at; a pixel outside the block reads as 0
        // and is taken out of the sum below
#pragma unroll
        for (int k = 0; k < FILMAC_FLIGHT; k++) {
            const int y = y0 + k * FILMAC_ROWS_PER_STEP;
            v[k] = px4_u4{0, 0, 0, 0};
            if (y < box.h && n > 0) {
                const uint8_t *p = at + (size_t)(box.y + y) * (size_t)src_ls;
                if (n == 4) v[k] = gld4a(p);
                else {
                    v[k].x = gld(p);
                    if (n > 1) v[k].y = gld(p + 4);
                    if (n > 2) v[k].z = gld(p + 8);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < FILMAC_FLIGHT; k++) {
            const int y = y0 + k * FILMAC_ROWS_PER_STEP;
            const int m = y < box.h ? n : 0;
            const uint32_t px[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < m) {
                    const uint32_t lo = min3(px[i]);
                    sum += GAMMA ? (uint32_t)s_dec[lo] : lo;
                    top = max(top, max3(px[i]));
                }
        }
    }
    // the wave, then the four waves through LDS
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += (uint32_t)__shfl_xor((int)sum, d);
        top = max(top, (uint32_t)__shfl_xor((int)top, d));
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_top[threadIdx.x >> 6] = top;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        FilmacBlockRec o;
        o.sum = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        o.top = max(max(s_top[0], s_top[1]), max(s_top[2], s_top[3]));
        o.count = (uint32_t)(box.w * box.h);
        o._pad = 0;
        blocks[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = o;
    }
}

FDEV int64_t shfl_xor64(int64_t v, int d)
{
    const int lo = __shfl_xor((int)(uint32_t)(uint64_t)v, d), hi = __shfl_xor((int)(uint32_t)((uint64_t)v >> 32), d);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// The levels of a frame :887-925 from its block records: a wavefront per frame, lanes over its blocks (one 64-bit
// division per block for the mean), four frames per workgroup.  dec: the gamma decode table or NULL.  tap: per frame
// of the call, what the next two kernels go by and ntscsim_filmac_debug_levels() reads.
__global__ __launch_bounds__(FILMAC_THREADS) void k_filmac_frame_levels(const FilmacBlockRec *__restrict__ blocks, int nblocks, int m,
                                                                       const uint16_t *__restrict__ dec, FilmacTap *__restrict__ tap)
{
    const int f = (int)(blockIdx.x * FILMAC_WAVES + (threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    if (f >= m) return;
    const FilmacBlockRec *rec = blocks + (size_t)f * (size_t)nblocks;
    FilmacLevels l = filmac_levels_start(filmac_scale(dec != nullptr));
    for (int b = lane; b < nblocks; b += 64) l = filmac_levels_add(l, rec[b], dec);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) l = filmac_levels_join(l, FilmacLevels{shfl_xor64(l.minv, d), shfl_xor64(l.maxv, d)});
    l = filmac_levels_end(l);
    if (lane == 0) {
        tap[f].minv = l.minv;
        tap[f].maxv = l.maxv;
    }
}

// The serial part :927-942, one workgroup.  Frames go through LDS in chunks of FILMAC_CHUNK: all lanes fetch the
// chunk's levels, lane 0 walks the recurrence from LDS to LDS, all lanes write the results.  run: the device-resident
// state, read once and written once.
__global__ __launch_bounds__(FILMAC_LEVEL_THREADS) void k_filmac_levels(int m, FilmacRun *__restrict__ run, FilmacTap *__restrict__ tap)
{
    __shared__ int64_t s_lo[FILMAC_CHUNK], s_hi[FILMAC_CHUNK];       // minv / maxv, then final_minv / final_maxv
    __shared__ FilmacRun s_run;

    if (threadIdx.x == 0) s_run = *run;
    for (int base = 0; base < m; base += FILMAC_CHUNK) {
        const int frames = m - base < FILMAC_CHUNK ? m - base : FILMAC_CHUNK;
        __syncthreads();                                                         // s_run; the final levels of the chunk before
        for (int f = (int)threadIdx.x; f < frames; f += FILMAC_LEVEL_THREADS) {
            s_lo[f] = tap[base + f].minv;
            s_hi[f] = tap[base + f].maxv;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            FilmacRun s = s_run;
            for (int f = 0; f < frames; f++) {
                s = filmac_step(s, FilmacLevels{s_lo[f], s_hi[f]});
                s_lo[f] = s.final_minv;
                s_hi[f] = s.final_maxv;
            }
            s_run = s;
        }
        __syncthreads();
        for (int f = (int)threadIdx.x; f < frames; f += FILMAC_LEVEL_THREADS) {
            tap[base + f].final_minv = s_lo[f];
            tap[base + f].final_maxv = s_hi[f];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *run = s_run;
}

// the stretch of frame blockIdx.x as a byte table :946-1006; lane: the input byte
__global__ __launch_bounds__(256) void k_filmac_tables(const FilmacTap *__restrict__ tap, const uint16_t *__restrict__ dec,
                                                      const uint8_t *__restrict__ enc, uint8_t *__restrict__ tables)
{
    const FilmacTap &t = tap[blockIdx.x];
    tables[(size_t)blockIdx.x * 256 + threadIdx.x] = filmac_map(threadIdx.x, t.final_minv, t.final_maxv, dec, enc);
}

// B, G, R through the table, alpha 0xFF :986-989 / :1000-1003
FDEV uint32_t filmac_px(const uint8_t *t, uint32_t p)
{
    return (uint32_t)t[p & 0xFFu] | ((uint32_t)t[(p >> 8) & 0xFFu] << 8) | ((uint32_t)t[(p >> 16) & 0xFFu] << 16) | 0xFF000000u;
}

// pixels [first, first + per) of each of the band's rows as dwords, one per lane
FDEV void filmac_map_dwords(const uint8_t *t, uint8_t *dst, int dst_ls, const uint8_t *src, int src_ls, int y0, int rows, int first, int per)
{
    const int total = per * rows;
    for (int base = threadIdx.x; base < total; base += FILMAC_UNROLL * FILMAC_THREADS) {
        uint32_t v[FILMAC_UNROLL];
        uint8_t *dp[FILMAC_UNROLL];
#pragma unroll
        for (int k = 0; k < FILMAC_UNROLL; k++) {
            const int item = base + k * FILMAC_THREADS;
            if (item < total) {
                const int row = item / per, i = first + (item - row * per);
                dp[k] = dst + (size_t)(y0 + row) * (size_t)dst_ls + 4 * (size_t)i;
                v[k] = gld(src + (size_t)(y0 + row) * (size_t)src_ls + 4 * (size_t)i);
            }
        }
#pragma unroll
        for (int k = 0; k < FILMAC_UNROLL; k++)
            if (base + k * FILMAC_THREADS < total) gst(dp[k], filmac_px(t, v[k]));
    }
}

// A lane reads a pixel before it writes it and no other lane touches that pixel, so dst may be src.
__global__ __launch_bounds__(FILMAC_THREADS) void k_filmac_apply(const FilmacRec *__restrict__ recs, const uint8_t *__restrict__ tables, int W, int H)
{
    __shared__ uint8_t s_t[256];

    const FilmacRec &r = recs[blockIdx.y];
    uint8_t *const dst = r.dst;
    const uint8_t *const src = r.src;
    const int dst_ls = r.dst_ls, src_ls = r.src_ls;
    const bool vec = r.vec != 0;
    s_t[threadIdx.x] = tables[(size_t)blockIdx.y * 256 + threadIdx.x];
    __syncthreads();

    const int y0 = (int)blockIdx.x * FILMAC_BAND;
    const int rows = H - y0 < FILMAC_BAND ? H - y0 : FILMAC_BAND;
    if (vec) {
        const int Q = W >> 2, total = Q * rows;
        for (int base = threadIdx.x; base < total; base += FILMAC_UNROLL * FILMAC_THREADS) {
            px4_u4 v[FILMAC_UNROLL];
            uint8_t *dp[FILMAC_UNROLL];
#pragma unroll
            for (int k = 0; k < FILMAC_UNROLL; k++) {
                const int item = base + k * FILMAC_THREADS;
                if (item < total) {
                    const int row = item / Q, i = (item - row * Q) << 2;
                    dp[k] = dst + (size_t)(y0 + row) * (size_t)dst_ls + 4 * (size_t)i;
                    v[k] = gld4a(src + (size_t)(y0 + row) * (size_t)src_ls + 4 * (size_t)i);
                }
            }
#pragma unroll
            for (int k = 0; k < FILMAC_UNROLL; k++)
                if (base + k * FILMAC_THREADS < total)
                    gst4(dp[k], px4_u4{filmac_px(s_t, v[k].x), filmac_px(s_t, v[k].y), filmac_px(s_t, v[k].z), filmac_px(s_t, v[k].w)});
        }
        if (W & 3) filmac_map_dwords(s_t, dst, dst_ls, src, src_ls, y0, rows, W & ~3, W & 3);
    } else
        filmac_map_dwords(s_t, dst, dst_ls, src, src_ls, y0, rows, 0, W);
}

// ---- host side -----------------------------------------------------------------------------------------------

struct FilmacState {
    ntscsim_filmac_params prm;
    bool gamma = false;                  // gamma_correction > 1 :859
    RecordSlots<> slots;
    FrameArena frames;                   // ntscsim_filmac_frames_host()
    FilmacRun *run = nullptr;            // device: final_init, final_minv, final_maxv
    uint16_t *dec = nullptr;             // device: gamma_dec16_table, gamma_enc16_table behind it (NULL without gamma)
    uint8_t *enc = nullptr;
    unsigned char *scratch = nullptr;    // device: block records | tables of one launch
    size_t scratch_cap = 0;
    FilmacTap *tap = nullptr;            // device: one per frame of the last call
    size_t tap_cap = 0;
    int tap_frames = 0;
    bool timing = false;                 // ntscsim_filmac_debug_time_kernels()
    std::vector<hipEvent_t> marks;       // six per launch group of the last call: around each of the five kernels
};

void filmac_drop_marks(FilmacState *k)
{
    for (hipEvent_t e : k->marks) (void)hipEventDestroy(e);
    k->marks.clear();
}

void filmac_state_destroy(FilmacState *k)
{
    if (!k) return;
    if (k->run) (void)hipFree(k->run);
    if (k->dec) (void)hipFree(k->dec);
    if (k->scratch) (void)hipFree(k->scratch);
    if (k->tap) (void)hipFree(k->tap);
    filmac_drop_marks(k);
    k->slots.release();
    k->frames.release();
    delete k;
}

} // namespace ntscsim

using namespace ntscsim;

namespace {

constexpr size_t FILMAC_SCRATCH_MAX = (size_t)64 << 20;         // a launch takes fewer frames rather than more scratch

bool filmac_size_ok(int w, int h) { return w >= FILMAC_MIN_SIZE && w <= FILMAC_MAX_SIZE && h >= FILMAC_MIN_SIZE && h <= FILMAC_MAX_SIZE; }

size_t filmac_frame_scratch(int nblocks) { return (size_t)nblocks * sizeof(FilmacBlockRec) + 256; }

// frames one launch may take
int filmac_launch_cap(int nblocks) { return (int)std::max<size_t>(1, std::min<size_t>(65535, FILMAC_SCRATCH_MAX / filmac_frame_scratch(nblocks))); }

// aligned: a device call; a host frame may lie anywhere and have any linesize that holds a row
int filmac_check_desc(const FilmacState *k, const ntscsim_filmac_desc &d, bool aligned)
{
    const int W = k->prm.width, H = k->prm.height;
    if (!d.dst || !d.src) return NTSCSIM_E_ARG;
    if (plane_check(d.dst, d.dst_linesize, W, aligned)) return NTSCSIM_E_SIZE;
    if (plane_check(d.src, d.src_linesize, W, aligned)) return NTSCSIM_E_SIZE;
    const bool in_place = d.dst == d.src && d.dst_linesize == d.src_linesize;
    if (!in_place && overlaps(span_of(d.dst, d.dst_linesize, H), span_of(d.src, d.src_linesize, H))) return NTSCSIM_E_ARG;
    return NTSCSIM_OK;
}

// what descriptor i touches, for frames_in_order()
Span filmac_touch(const ntscsim_filmac_desc &d, int H, std::vector<Span> &rd)
{
    rd.push_back(span_of(d.src, d.src_linesize, H));
    return span_of(d.dst, d.dst_linesize, H);
}

// five launches over descriptors that do not depend on each other; frame0: index of descs[0] in the call
int filmac_launch(ntscsim_ctx *c, const ntscsim_filmac_desc *descs, int m, int frame0, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    FilmacState *k = *v.filmac;
    const int W = k->prm.width, H = k->prm.height;
    const FilmacGrid g = filmac_grid(W, H);
    const int nblocks = g.nbx * g.nby;
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, (size_t)m * sizeof(FilmacRec), slot);
    if (rc != NTSCSIM_OK) return rc;
    RecordSlot &s = *slot;
    FilmacRec *recs = reinterpret_cast<FilmacRec *>(s.host);
    for (int i = 0; i < m; i++) {
        const ntscsim_filmac_desc &d = descs[i];
        FilmacRec &r = recs[i];
        std::memset(&r, 0, sizeof(r));
        r.dst = static_cast<uint8_t *>(d.dst);
        r.src = static_cast<const uint8_t *>(d.src);
        r.dst_ls = d.dst_linesize;
        r.src_ls = d.src_linesize;
        r.vec = (((uintptr_t)d.dst | (uintptr_t)d.dst_linesize) & 15) == 0;
    }
    STAGECHK(v, hipMemcpyAsync(s.dev, s.host, (size_t)m * sizeof(FilmacRec), hipMemcpyHostToDevice, st));
    const FilmacRec *recs_dev = reinterpret_cast<const FilmacRec *>(s.dev);
    const uint16_t *dec = k->gamma ? k->dec : nullptr;
    const uint8_t *enc = k->gamma ? k->enc : nullptr;
    FilmacBlockRec *blocks = reinterpret_cast<FilmacBlockRec *>(k->scratch);
    uint8_t *tables = k->scratch + (size_t)m * (size_t)nblocks * sizeof(FilmacBlockRec);
    const dim3 block(FILMAC_THREADS);
    const auto mark = [&]() -> int {                                            // between the kernels, while they are timed
        if (!k->timing) return NTSCSIM_OK;
        hipEvent_t e = nullptr;
        STAGECHK(v, hipEventCreate(&e));
        k->marks.push_back(e);
        STAGECHK(v, hipEventRecord(e, st));
        return NTSCSIM_OK;
    };
    int lrc = mark();
    if (lrc != NTSCSIM_OK) return lrc;
    if (k->gamma) hipLaunchKernelGGL(k_filmac_stats<true>, dim3((unsigned)nblocks, (unsigned)m), block, 0, st, recs_dev, dec, blocks, W, H);
    else hipLaunchKernelGGL(k_filmac_stats<false>, dim3((unsigned)nblocks, (unsigned)m), block, 0, st, recs_dev, dec, blocks, W, H);
    lrc = stage_launched(v, nullptr, st, "k_filmac_stats");
    if (lrc == NTSCSIM_OK) lrc = mark();
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_filmac_frame_levels, dim3((unsigned)((m + FILMAC_WAVES - 1) / FILMAC_WAVES)), block, 0, st, blocks, nblocks, m, dec, k->tap + frame0);
    lrc = stage_launched(v, nullptr, st, "k_filmac_frame_levels");
    if (lrc == NTSCSIM_OK) lrc = mark();
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_filmac_levels, dim3(1), dim3(FILMAC_LEVEL_THREADS), 0, st, m, k->run, k->tap + frame0);
    lrc = stage_launched(v, nullptr, st, "k_filmac_levels");
    if (lrc == NTSCSIM_OK) lrc = mark();
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_filmac_tables, dim3((unsigned)m), dim3(256), 0, st, k->tap + frame0, dec, enc, tables);
    lrc = stage_launched(v, nullptr, st, "k_filmac_tables");
    if (lrc == NTSCSIM_OK) lrc = mark();
    if (lrc != NTSCSIM_OK) return lrc;
    hipLaunchKernelGGL(k_filmac_apply, dim3((unsigned)((H + FILMAC_BAND - 1) / FILMAC_BAND), (unsigned)m), block, 0, st, recs_dev, tables, W, H);
    lrc = stage_launched(v, &s, st, "k_filmac_apply");
    return lrc == NTSCSIM_OK ? mark() : lrc;
}

// every descriptor checked, then launch groups, cut where descriptors depend on each other (frames_in_order()) and
// where the scratch of a launch ends
int filmac_frames(ntscsim_ctx *c, const ntscsim_filmac_desc *descs, int n, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    FilmacState *k = *v.filmac;
    const int W = k->prm.width, H = k->prm.height;
    for (int i = 0; i < n; i++) {
        const int rc = filmac_check_desc(k, descs[i], true);
        if (rc != NTSCSIM_OK) return rc;
    }
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    k->tap_frames = 0;
    filmac_drop_marks(k);
    if (n == 0) return NTSCSIM_OK;
    const FilmacGrid g = filmac_grid(W, H);
    const int nblocks = g.nbx * g.nby, cap = filmac_launch_cap(nblocks);
    const size_t want = (size_t)std::min(n, cap) * filmac_frame_scratch(nblocks);
    if (want > k->scratch_cap || (size_t)n > k->tap_cap) {
        const int rc = k->slots.wait_all(v);                                    // launches in flight use what is replaced
        if (rc != NTSCSIM_OK) return rc;
        if (want > k->scratch_cap) {
            if (k->scratch) { (void)hipFree(k->scratch); k->scratch = nullptr; k->scratch_cap = 0; }
            STAGECHK(v, hipMalloc((void **)&k->scratch, want));
            k->scratch_cap = want;
        }
        if ((size_t)n > k->tap_cap) {
            if (k->tap) { (void)hipFree(k->tap); k->tap = nullptr; k->tap_cap = 0; }
            STAGECHK(v, hipMalloc((void **)&k->tap, (size_t)n * sizeof(FilmacTap)));
            k->tap_cap = (size_t)n;
        }
    }
    const int rc = frames_in_order(n, cap, [&](int i, std::vector<Span> &rd) { return filmac_touch(descs[i], H, rd); },
                                   [&](int first, int m) { return filmac_launch(c, descs + first, m, first, st); });
    if (rc != NTSCSIM_OK) return rc;
    k->tap_frames = n;
    return NTSCSIM_OK;
}

// everything enqueued on the device has finished: the state and the tap are read and written with plain copies
int filmac_quiet(const CtxStageView &v)
{
    STAGECHK(v, hipSetDevice(v.device));
    STAGECHK(v, hipDeviceSynchronize());
    return NTSCSIM_OK;
}

} // namespace

extern "C" int ntscsim_filmac_bind(ntscsim_ctx *c, const ntscsim_filmac_params *p)
{
    if (!c || !p || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    if (!filmac_size_ok(p->width, p->height)) return NTSCSIM_E_SIZE;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    FilmacState *k = *v.filmac;
    if (!k) {
        k = new (std::nothrow) FilmacState();
        if (!k) return NTSCSIM_E_NOMEM;
        *v.filmac = k;
    }
    const int rc = k->slots.wait_all(v);                                        // launches in flight use the tables and the state
    if (rc != NTSCSIM_OK) return rc;
    const bool gamma = p->gamma_correction > 1;
    if (gamma) {
        std::vector<unsigned char> host(512 + 8193);
        const int trc = ntscsim_blend_tables(p->gamma_correction, reinterpret_cast<uint16_t *>(host.data()), host.data() + 512);
        if (trc != NTSCSIM_OK) return trc;
        if (!k->dec) STAGECHK(v, hipMalloc((void **)&k->dec, host.size()));
        STAGECHK(v, hipMemcpy(k->dec, host.data(), host.size(), hipMemcpyHostToDevice));
        k->enc = reinterpret_cast<uint8_t *>(k->dec) + 512;
    }
    if (!k->run) STAGECHK(v, hipMalloc((void **)&k->run, sizeof(FilmacRun)));
    STAGECHK(v, hipMemset(k->run, 0, sizeof(FilmacRun)));
    k->prm = *p;
    k->prm.input_path = nullptr;
    k->prm.output_path = nullptr;
    k->gamma = gamma;
    k->tap_frames = 0;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_filmac_frames_device(ntscsim_ctx *c, const ntscsim_filmac_desc *descs, int n, void *hip_stream)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    if (!*v.filmac) return NTSCSIM_E_ARG;                                       // ntscsim_filmac_bind() first
    return filmac_frames(c, descs, n, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

extern "C" int ntscsim_filmac_frames_host(ntscsim_ctx *c, const ntscsim_filmac_desc *descs, int n)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    FilmacState *k = *v.filmac;
    if (!k) return NTSCSIM_E_ARG;
    const int W = k->prm.width, H = k->prm.height;
    for (int i = 0; i < n; i++) {
        const int rc = filmac_check_desc(k, descs[i], false);
        if (rc != NTSCSIM_OK) return rc;
    }
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    // Batches of frames through the arena: source | destination per frame, rows packed to a 16-byte pitch.  Only the
    // 4 * width bytes of a row travel either way, so what the device call leaves alone keeps what the host frame held.
    // A batch ends in front of a descriptor that touches a frame an earlier one of the batch wrote, or writes one it
    // read: descriptors take effect in order, through host memory.  The level state stays on the device between batches.
    hipStream_t st = v.stream;
    const size_t row = (size_t)W * 4, pitch = (row + 15) & ~(size_t)15, fbytes = pitch * (size_t)H;
    const int cap = (int)std::max<size_t>(1, std::min<size_t>(65535, ((size_t)256 << 20) / (2 * fbytes)));
    std::string kernels;
    std::vector<ntscsim_filmac_desc> dev;
    std::vector<FilmacTap> taps;                                                // the call's, gathered batch by batch
    const auto touch = [&](int i, std::vector<Span> &rd) { return filmac_touch(descs[i], H, rd); };
    const int rc = frames_in_order(n, cap, touch, [&](int first, int m) -> int {
        const int arc = k->frames.reserve(v, 2 * fbytes * (size_t)m, fbytes * (size_t)m);
        if (arc != NTSCSIM_OK) return arc;
        unsigned char *stage = k->frames.staging, *arena = k->frames.arena;
        dev.assign(descs + first, descs + first + m);
        for (int i = 0; i < m; i++) {
            ntscsim_filmac_desc &d = dev[(size_t)i];
            copy_rows(stage + (size_t)i * fbytes, pitch, d.src, (size_t)d.src_linesize, row, H);
            d.src = arena + (size_t)i * fbytes;
            d.dst = arena + (size_t)(m + i) * fbytes;
            d.src_linesize = d.dst_linesize = (int)pitch;
        }
        STAGECHK(v, hipMemcpyAsync(arena, stage, fbytes * (size_t)m, hipMemcpyHostToDevice, st));
        const int frc = filmac_frames(c, dev.data(), m, st);
        if (frc != NTSCSIM_OK) return frc;
        if (!kernels.empty()) kernels += ';';
        kernels += *v.kernels;
        STAGECHK(v, hipMemcpyAsync(stage, arena + (size_t)m * fbytes, fbytes * (size_t)m, hipMemcpyDeviceToHost, st));
        taps.resize((size_t)(first + m));
        STAGECHK(v, hipMemcpyAsync(taps.data() + first, k->tap, (size_t)m * sizeof(FilmacTap), hipMemcpyDeviceToHost, st));
        STAGECHK(v, hipStreamSynchronize(st));
        for (int i = 0; i < m; i++)
            copy_rows(descs[first + i].dst, (size_t)descs[first + i].dst_linesize, stage + (size_t)i * fbytes, pitch, row, H);
        return NTSCSIM_OK;
    });
    if (rc != NTSCSIM_OK) return rc;
    *v.kernels = kernels;
    // the tap speaks of the whole call, not of its last batch
    if ((size_t)n > k->tap_cap) {
        if (k->tap) { (void)hipFree(k->tap); k->tap = nullptr; k->tap_cap = 0; }
        STAGECHK(v, hipMalloc((void **)&k->tap, (size_t)n * sizeof(FilmacTap)));
        k->tap_cap = (size_t)n;
    }
    if (n > 0) STAGECHK(v, hipMemcpy(k->tap, taps.data(), (size_t)n * sizeof(FilmacTap), hipMemcpyHostToDevice));
    k->tap_frames = n;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_filmac_reset(ntscsim_ctx *c)
{
    ntscsim_filmac_state s;
    std::memset(&s, 0, sizeof(s));
    return ntscsim_filmac_set_state(c, &s);
}

extern "C" int ntscsim_filmac_get_state(ntscsim_ctx *c, ntscsim_filmac_state *out)
{
    FilmacState *k = c ? *ctx_stage_view(c).filmac : nullptr;
    if (!k || !out) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = filmac_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    FilmacRun r;
    STAGECHK(v, hipMemcpy(&r, k->run, sizeof(r), hipMemcpyDeviceToHost));
    out->init = r.init != 0;
    out->_pad = 0;
    out->final_minv = r.final_minv;
    out->final_maxv = r.final_maxv;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_filmac_set_state(ntscsim_ctx *c, const ntscsim_filmac_state *in)
{
    FilmacState *k = c ? *ctx_stage_view(c).filmac : nullptr;
    if (!k || !in) return NTSCSIM_E_ARG;
    if (in->final_minv < -FILMAC_STATE_LIMIT || in->final_minv > FILMAC_STATE_LIMIT || in->final_maxv < -FILMAC_STATE_LIMIT ||
        in->final_maxv > FILMAC_STATE_LIMIT)
        return NTSCSIM_E_PARAM;
    CtxStageView v = ctx_stage_view(c);
    const int rc = filmac_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    const FilmacRun r{in->init != 0, in->final_minv, in->final_maxv};
    STAGECHK(v, hipMemcpy(k->run, &r, sizeof(r), hipMemcpyHostToDevice));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_filmac_debug_levels(ntscsim_ctx *c, int frame, int64_t out[4])
{
    FilmacState *k = c ? *ctx_stage_view(c).filmac : nullptr;
    if (!k || !out || !k->tap || frame < 0 || frame >= k->tap_frames) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = filmac_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpy(out, k->tap + frame, sizeof(FilmacTap), hipMemcpyDeviceToHost));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_filmac_debug_time_kernels(ntscsim_ctx *c, int on)
{
    FilmacState *k = c ? *ctx_stage_view(c).filmac : nullptr;
    if (!k) return NTSCSIM_E_ARG;
    k->timing = on != 0;
    if (!k->timing) filmac_drop_marks(k);
    return NTSCSIM_OK;
}

extern "C" int ntscsim_filmac_debug_kernel_ms(ntscsim_ctx *c, float out_ms[5])
{
    FilmacState *k = c ? *ctx_stage_view(c).filmac : nullptr;
    if (!k || !out_ms || k->marks.empty() || k->marks.size() % 6) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = filmac_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    for (int i = 0; i < 5; i++) out_ms[i] = 0.0f;
    for (size_t g = 0; g < k->marks.size(); g += 6)
        for (int i = 0; i < 5; i++) {
            float ms = 0.0f;
            STAGECHK(v, hipEventElapsedTime(&ms, k->marks[g + (size_t)i], k->marks[g + (size_t)i + 1]));
            out_ms[i] += ms;
        }
    return NTSCSIM_OK;
}
