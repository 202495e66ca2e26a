// ntsc_pixmap.hip -- device half of the posterize and colormap stages (include/ntscsim.h: ntscsim_post_*,
// ntscsim_cmap_*): the two tools whose frame body is `out = f(in)` pixel by pixel, ffmpeg_posterize.cpp:789-813 and
// ffmpeg_colormap.cpp:785-822.  One loop over a band of rows (pix_band) and one host side serve both; the stages differ
// in f, in what a record carries for it, and in the colormap's table, which is state.
//
// k_post_frames  grid (bands of rows, frames): out = in & mask, the mask in the record.
// k_cmap_frames  grid (bands of rows, frames): every workgroup fills a 256-dword table in LDS -- from the middle row of
//                the map its record names, or from the ctx's table -- and then out = table[green of in].
// k_cmap_take    256 lanes, behind k_cmap_frames of a launch group that had a map: the ctx's table from the group's
//                last map, so that later groups and later calls start from it.  
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ntscsim.h"
#include "ntsc_frames.hpp"
#include "ntsc_px4.hpp"
#include "ntsc_stage.hpp"

namespace ntscsim {

constexpr int PIX_THREADS = 256;
constexpr int PIX_BAND = 8;              // rows a workgroup maps
constexpr int PIX_UNROLL = 4;            // quads a lane requests before its first store
constexpr int PIX_MIN_SIZE = 1, PIX_MAX_SIZE = 16384;

struct PixRec {                          // one frame
    uint8_t *dst;
    const uint8_t *src;
    const uint8_t *table;                // colormap: a map's middle row, or the ctx's table
    int32_t dst_ls, src_ls;
    uint32_t vec;                        // dst and dst_ls are multiples of 16
    uint32_t arg;                        // posterize: the mask; colormap: `table` is a map's row (entry i at pixel i * W / 256)
};

// Rows y0 .. of frame r, out = f(in): a lane takes quads of pixels (the last of a row may hold fewer), requests
// PIX_UNROLL of them before it stores the first, and reads a pixel before it writes it while no other lane touches
// that pixel, so dst may be src.  VEC: whole quads are stored as 16 bytes.
template <bool VEC, class F>
PX4_DEV void pix_band(const PixRec &r, int W, int H, F f)
{
    uint8_t *const dst = r.dst;
    const uint8_t *const src = r.src;
    const int dst_ls = r.dst_ls, src_ls = r.src_ls;
    const int y0 = (int)blockIdx.x * PIX_BAND;
    const int rows = H - y0 < PIX_BAND ? H - y0 : PIX_BAND;
    const int Q = (W + 3) >> 2, total = Q * rows;
    for (int base = threadIdx.x; base < total; base += PIX_UNROLL * PIX_THREADS) {
        uint32_t v[PIX_UNROLL][4] = {};
        uint8_t *dp[PIX_UNROLL];
        int n[PIX_UNROLL];
#pragma unroll
        for (int k = 0; k < PIX_UNROLL; k++) {
            const int item = base + k * PIX_THREADS;
            if (item < total) {
                const int row = item / Q, i = (item - row * Q) << 2;
                const uint8_t *sp = src + (size_t)(y0 + row) * (size_t)src_ls + 4 * (size_t)i;
                dp[k] = dst + (size_t)(y0 + row) * (size_t)dst_ls + 4 * (size_t)i;
                n[k] = W - i < 4 ? W - i : 4;
                if (n[k] == 4) {
                    const px4_u4 q = gld4a(sp);
                    v[k][0] = q.x; v[k][1] = q.y; v[k][2] = q.z; v[k][3] = q.w;
                } else
                    px4_load<false>(v[k], sp, n[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < PIX_UNROLL; k++)
            if (base + k * PIX_THREADS < total) {
#pragma unroll
                for (int j = 0; j < 4; j++) v[k][j] = f(v[k][j]);
                if (VEC && n[k] == 4) px4_store<true>(dp[k], v[k], 4);
                else px4_store<false>(dp[k], v[k], n[k]);
            }
    }
}

template <class F>
PX4_DEV void pix_frame(const PixRec &r, int W, int H, F f)
{
    if (r.vec) pix_band<true>(r, W, H, f);
    else pix_band<false>(r, W, H, f);
}

__global__ __launch_bounds__(PIX_THREADS) void k_post_frames(const PixRec *__restrict__ recs, int W, int H)
{
    const PixRec &r = recs[blockIdx.y];
    const uint32_t mask = r.arg;
    pix_frame(r, W, H, [mask](uint32_t p) { return p & mask; });
}

// entry i of the table `from` names: take_colormap() :795-798 on a map's row, or the table as it stands
PX4_DEV uint32_t cmap_entry(const uint8_t *from, bool is_row, int W, unsigned i)
{
    return gld(from + 4 * (size_t)(is_row ? (i * (unsigned)W) / 256u : i));
}

__global__ __launch_bounds__(PIX_THREADS) void k_cmap_frames(const PixRec *__restrict__ recs, int W, int H)
{
    __shared__ uint32_t s_t[256];
    static_assert(PIX_THREADS == 256, "a lane per table entry");

    const PixRec &r = recs[blockIdx.y];
    s_t[threadIdx.x] = cmap_entry(r.table, r.arg != 0, W, threadIdx.x);
    __syncthreads();
    pix_frame(r, W, H, [](uint32_t p) { return s_t[(p >> 8) & 0xFFu]; });        // :818-819
}

__global__ __launch_bounds__(256) void k_cmap_take(const uint8_t *__restrict__ row, uint32_t *__restrict__ table, int W)
{
    gst(table + threadIdx.x, cmap_entry(row, true, W, threadIdx.x));
}

// ---- host side -----------------------------------------------------------------------------------------------

struct PixState {                        // what the two stages keep alike
    int W = 0, H = 0;
    RecordSlots<> slots;
    FrameArena frames;                   // *_frames_host()
};

struct PostState : PixState {
    std::vector<uint32_t> masks;         // per bound input: ((0xFF << (8 - threshhold)) & 0xFF) * 0x01010101 :796-797
};

struct CmapState : PixState {
    uint32_t *table = nullptr;           // device: colormap[256] :58
};

void post_state_destroy(PostState *k)
{
    if (!k) return;
    k->slots.release();
    k->frames.release();
    delete k;
}

void cmap_state_destroy(CmapState *k)
{
    if (!k) return;
    if (k->table) (void)hipFree(k->table);
    k->slots.release();
    k->frames.release();
    delete k;
}

} // namespace ntscsim

using namespace ntscsim;

namespace {

// A descriptor of either stage.  row: the middle row of the colormap's map, NULL without one (posterize: always).
struct PixJob {
    const void *src;
    void *dst;
    const void *row;
    int32_t src_ls, dst_ls;
    uint32_t mask;
};

Span row_span(const void *row, int W) { return Span{(uintptr_t)row, (uintptr_t)row + 4 * (size_t)W}; }

// aligned: a device call; a host frame may lie anywhere and have any linesize that holds a row
int pix_check(const PixState &k, const PixJob &j, bool aligned)
{
    if (!j.dst || !j.src) return NTSCSIM_E_ARG;
    if (plane_check(j.dst, j.dst_ls, k.W, aligned)) return NTSCSIM_E_SIZE;
    if (plane_check(j.src, j.src_ls, k.W, aligned)) return NTSCSIM_E_SIZE;
    const Span wr = span_of(j.dst, j.dst_ls, k.H);
    const bool in_place = j.dst == j.src && j.dst_ls == j.src_ls;
    if (!in_place && overlaps(wr, span_of(j.src, j.src_ls, k.H))) return NTSCSIM_E_ARG;
    if (j.row && overlaps(wr, row_span(j.row, k.W))) return NTSCSIM_E_ARG;      // the table would depend on the band order
    return NTSCSIM_OK;
}

// what a job touches, for frames_in_order()
Span pix_touch(const PixState &k, const PixJob &j, std::vector<Span> &rd)
{
    rd.push_back(span_of(j.src, j.src_ls, k.H));
    if (j.row) rd.push_back(row_span(j.row, k.W));
    return span_of(j.dst, j.dst_ls, k.H);
}

int post_job(const PostState &k, const ntscsim_post_desc &d, bool aligned, PixJob &j)
{
    if (d.layer < 0 || (size_t)d.layer >= k.masks.size()) return NTSCSIM_E_ARG;
    j = PixJob{d.src, d.dst, nullptr, d.src_linesize, d.dst_linesize, k.masks[(size_t)d.layer]};
    return pix_check(k, j, aligned);
}

int cmap_job(const CmapState &k, const ntscsim_cmap_desc &d, bool aligned, PixJob &j)
{
    j = PixJob{d.src, d.dst, nullptr, d.src_linesize, d.dst_linesize, 0};
    if (d.map) {
        if (plane_check(d.map, d.map_linesize, k.W, aligned)) return NTSCSIM_E_SIZE;
        j.row = static_cast<const uint8_t *>(d.map) + (size_t)(k.H / 2) * (size_t)d.map_linesize;   // :793-794
    }
    return pix_check(k, j, aligned);
}

// One launch group: jobs that do not depend on each other.  table: the colormap's (NULL: posterize).  A colormap job
// without a map goes by the nearest map before it in the group, and by the table where there is none; the group's last
// map becomes the table behind it.
int pix_launch(const CtxStageView &v, PixState &k, uint32_t *table, const PixJob *jobs, int m, hipStream_t st)
{
    RecordSlot *slot = nullptr;
    const int rc = k.slots.acquire(v, (size_t)m * sizeof(PixRec), slot);
    if (rc != NTSCSIM_OK) return rc;
    RecordSlot &s = *slot;
    PixRec *recs = reinterpret_cast<PixRec *>(s.host);
    const void *row = nullptr;
    for (int i = 0; i < m; i++) {
        const PixJob &j = jobs[i];
        PixRec &r = recs[i];
        std::memset(&r, 0, sizeof(r));
        if (j.row) row = j.row;
        r.dst = static_cast<uint8_t *>(j.dst);
        r.src = static_cast<const uint8_t *>(j.src);
        r.table = static_cast<const uint8_t *>(row ? row : table);
        r.dst_ls = j.dst_ls;
        r.src_ls = j.src_ls;
        r.vec = (((uintptr_t)j.dst | (uintptr_t)j.dst_ls) & 15) == 0;
        r.arg = table ? (row != nullptr) : j.mask;
    }
    STAGECHK(v, hipMemcpyAsync(s.dev, s.host, (size_t)m * sizeof(PixRec), hipMemcpyHostToDevice, st));
    const PixRec *recs_dev = reinterpret_cast<const PixRec *>(s.dev);
    const dim3 grid((unsigned)((k.H + PIX_BAND - 1) / PIX_BAND), (unsigned)m), block(PIX_THREADS);
    if (!table) {
        hipLaunchKernelGGL(k_post_frames, grid, block, 0, st, recs_dev, k.W, k.H);
        return stage_launched(v, &s, st, "k_post_frames");
    }
    hipLaunchKernelGGL(k_cmap_frames, grid, block, 0, st, recs_dev, k.W, k.H);
    const int lrc = stage_launched(v, &s, st, "k_cmap_frames");
    if (lrc != NTSCSIM_OK || !row) return lrc;
    hipLaunchKernelGGL(k_cmap_take, dim3(1), dim3(256), 0, st, static_cast<const uint8_t *>(row), table, k.W);
    return stage_launched(v, nullptr, st, "k_cmap_take");
}

// launches of at most 65535 jobs, cut where jobs depend on each other: they take effect in order
int pix_frames(const CtxStageView &v, PixState &k, uint32_t *table, const std::vector<PixJob> &jobs, hipStream_t st)
{
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    return frames_in_order((int)jobs.size(), 65535, [&](int i, std::vector<Span> &rd) { return pix_touch(k, jobs[(size_t)i], rd); },
                           [&](int first, int m) { return pix_launch(v, k, table, jobs.data() + first, m, st); });
}

// Host frames in batches through the arena: sources | map rows (colormap) | destinations, rows packed to a 16-byte
// pitch.  Only the 4 * width bytes of a row travel either way, so what the device call leaves alone keeps what the
// host frame held.  A batch ends in front of a job that touches a frame an earlier one of the batch wrote, or writes
// what it read: jobs take effect in order, through host memory.  The colormap's table stays on the device throughout.
int pix_frames_host(const CtxStageView &v, PixState &k, uint32_t *table, const std::vector<PixJob> &jobs)
{
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    hipStream_t st = v.stream;
    const int H = k.H;
    const size_t row = (size_t)k.W * 4, pitch = (row + 15) & ~(size_t)15, fbytes = pitch * (size_t)H;
    const size_t up = fbytes + (table ? pitch : 0);                             // bytes of a job that go up
    const int cap = (int)std::max<size_t>(1, std::min<size_t>(65535, ((size_t)256 << 20) / (up + fbytes)));
    std::string kernels;
    std::vector<PixJob> dev;
    const auto touch = [&](int i, std::vector<Span> &rd) { return pix_touch(k, jobs[(size_t)i], rd); };
    const int rc = frames_in_order((int)jobs.size(), cap, touch, [&](int first, int m) -> int {
        const size_t M = (size_t)m;
        const int arc = k.frames.reserve(v, (up + fbytes) * M, up * M);
        if (arc != NTSCSIM_OK) return arc;
        unsigned char *stage = k.frames.staging, *arena = k.frames.arena;
        unsigned char *rows_h = stage + fbytes * M, *rows_d = arena + fbytes * M, *dst_d = arena + up * M;
        dev.assign(jobs.begin() + first, jobs.begin() + first + m);
        for (size_t i = 0; i < M; i++) {
            PixJob &j = dev[i];
            copy_rows(stage + i * fbytes, pitch, j.src, (size_t)j.src_ls, row, H);
            j.src = arena + i * fbytes;
            j.dst = dst_d + i * fbytes;
            j.src_ls = j.dst_ls = (int)pitch;
            if (j.row) {
                std::memcpy(rows_h + i * pitch, j.row, row);
                j.row = rows_d + i * pitch;
            }
        }
        STAGECHK(v, hipMemcpyAsync(arena, stage, up * M, hipMemcpyHostToDevice, st));
        const int frc = pix_frames(v, k, table, dev, st);
        if (frc != NTSCSIM_OK) return frc;
        if (!kernels.empty()) kernels += ';';
        kernels += *v.kernels;
        STAGECHK(v, hipMemcpyAsync(stage, dst_d, fbytes * M, hipMemcpyDeviceToHost, st));
        STAGECHK(v, hipStreamSynchronize(st));
        for (size_t i = 0; i < M; i++) {
            const PixJob &j = jobs[(size_t)first + i];
            copy_rows(j.dst, (size_t)j.dst_ls, stage + i * fbytes, pitch, row, H);
        }
        return NTSCSIM_OK;
    });
    if (rc != NTSCSIM_OK) return rc;
    *v.kernels = kernels;
    return NTSCSIM_OK;
}

// the descriptors of a call as checked jobs
template <class State, class Desc, class ToJob>
int pix_jobs(const State *k, const Desc *descs, int n, bool aligned, ToJob to_job, std::vector<PixJob> &jobs)
{
    if (!k || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;                  // *_bind() first
    jobs.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        const int rc = to_job(*k, descs[i], aligned, jobs[(size_t)i]);
        if (rc != NTSCSIM_OK) return rc;
    }
    return NTSCSIM_OK;
}

// what *_bind() asks of the parameters, before it looks at the ctx
int pix_params_check(const ntscsim_pixmap_params *p)
{
    if (!p || p->struct_size != sizeof(*p) || p->n_layers < 0 || (p->n_layers > 0 && !p->layers)) return NTSCSIM_E_ARG;
    if (p->width < PIX_MIN_SIZE || p->width > PIX_MAX_SIZE || p->height < PIX_MIN_SIZE || p->height > PIX_MAX_SIZE) return NTSCSIM_E_SIZE;
    return NTSCSIM_OK;
}

// *_bind(): the stage's state, made on the first call, with nothing of it in flight, holding the frame size
template <class State>
int pix_bind(const CtxStageView &v, State **at, const ntscsim_pixmap_params *p, State *&k)
{
    STAGECHK(v, hipSetDevice(v.device));
    if (!*at) {
        *at = new (std::nothrow) State();
        if (!*at) return NTSCSIM_E_NOMEM;
    }
    k = *at;
    const int rc = k->slots.wait_all(v);
    if (rc != NTSCSIM_OK) return rc;
    k->W = p->width;
    k->H = p->height;
    return NTSCSIM_OK;
}

// everything enqueued on the device has finished: the table is read and written with plain copies
int cmap_quiet(const CtxStageView &v)
{
    STAGECHK(v, hipSetDevice(v.device));
    STAGECHK(v, hipDeviceSynchronize());
    return NTSCSIM_OK;
}

} // namespace

extern "C" int ntscsim_post_bind(ntscsim_ctx *c, const ntscsim_post_params *p)
{
    int rc = pix_params_check(p);
    if (rc != NTSCSIM_OK) return rc;
    for (int i = 0; i < p->n_layers; i++)
        if (p->layers[i].threshhold < 0 || p->layers[i].threshhold > 8) return NTSCSIM_E_PARAM;
    if (!c) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    PostState *k = nullptr;
    rc = pix_bind(v, v.post, p, k);
    if (rc != NTSCSIM_OK) return rc;
    k->masks.clear();
    for (int i = 0; i < p->n_layers; i++)
        k->masks.push_back(((0xFFu << (8 - p->layers[i].threshhold)) & 0xFFu) * 0x01010101u);
    return NTSCSIM_OK;
}

extern "C" int ntscsim_post_frames_device(ntscsim_ctx *c, const ntscsim_post_desc *descs, int n, void *hip_stream)
{
    if (!c) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    std::vector<PixJob> jobs;
    const int rc = pix_jobs(*v.post, descs, n, true, post_job, jobs);
    return rc != NTSCSIM_OK ? rc : pix_frames(v, **v.post, nullptr, jobs, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

extern "C" int ntscsim_post_frames_host(ntscsim_ctx *c, const ntscsim_post_desc *descs, int n)
{
    if (!c) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    std::vector<PixJob> jobs;
    const int rc = pix_jobs(*v.post, descs, n, false, post_job, jobs);
    return rc != NTSCSIM_OK ? rc : pix_frames_host(v, **v.post, nullptr, jobs);
}

extern "C" int ntscsim_cmap_bind(ntscsim_ctx *c, const ntscsim_cmap_params *p)
{
    int rc = pix_params_check(p);
    if (rc != NTSCSIM_OK) return rc;
    if (!c) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    CmapState *k = nullptr;
    rc = pix_bind(v, v.cmap, p, k);
    if (rc != NTSCSIM_OK) return rc;
    if (!k->table) STAGECHK(v, hipMalloc((void **)&k->table, 256 * sizeof(uint32_t)));
    return ntscsim_cmap_reset(c);
}

extern "C" int ntscsim_cmap_frames_device(ntscsim_ctx *c, const ntscsim_cmap_desc *descs, int n, void *hip_stream)
{
    if (!c) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    std::vector<PixJob> jobs;
    const int rc = pix_jobs(*v.cmap, descs, n, true, cmap_job, jobs);
    return rc != NTSCSIM_OK ? rc : pix_frames(v, **v.cmap, (*v.cmap)->table, jobs, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

extern "C" int ntscsim_cmap_frames_host(ntscsim_ctx *c, const ntscsim_cmap_desc *descs, int n)
{
    if (!c) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    std::vector<PixJob> jobs;
    const int rc = pix_jobs(*v.cmap, descs, n, false, cmap_job, jobs);
    return rc != NTSCSIM_OK ? rc : pix_frames_host(v, **v.cmap, (*v.cmap)->table, jobs);
}

extern "C" int ntscsim_cmap_reset(ntscsim_ctx *c)
{
    uint32_t t[256];
    for (uint32_t i = 0; i < 256; i++) t[i] = i * 0x01010101u;                  // :833
    return ntscsim_cmap_set_table(c, t);
}

extern "C" int ntscsim_cmap_get_table(ntscsim_ctx *c, uint32_t out[256])
{
    CmapState *k = c ? *ctx_stage_view(c).cmap : nullptr;
    if (!k || !out) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = cmap_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpy(out, k->table, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NTSCSIM_OK;
}

extern "C" int ntscsim_cmap_set_table(ntscsim_ctx *c, const uint32_t in[256])
{
    CmapState *k = c ? *ctx_stage_view(c).cmap : nullptr;
    if (!k || !in) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    const int rc = cmap_quiet(v);
    if (rc != NTSCSIM_OK) return rc;
    STAGECHK(v, hipMemcpy(k->table, in, 256 * sizeof(uint32_t), hipMemcpyHostToDevice));
    return NTSCSIM_OK;
}
