// ntsc_led.hip -- device half of the vhsled stage (include/ntscsim.h: ntscsim_led_*): blackish(), the row walk, the
// nine-row mean and the shifted copy of ffmpeg_vhsled.cpp:682-692 and :866-931 in one pass over the frame.  Line
// numbers refer to that file.
//
// k_led_frames: a workgroup of four wavefronts owns a band of LED_BAND rows of one frame.  It scans those rows and
// the four above and below (clipped to the frame; the halo is scanned again by the neighbouring band, which costs
// little because a scan stops at the row's edge), keeps the edges in LDS, smooths, and then copies its rows with the
// per-row shift.  Nothing passes between workgroups, so n frames are one launch of (bands, frames) workgroups.
//
// The scan is bound by latency, not by bandwidth: a wavefront looks at 64 pixels per load, lane l at pixel base + l,
// and decides on the 64-bit ballot with scalar code (csrc/led_run.hpp).  Each wave therefore requests the first
// LED_PROBE chunks of ALL of its rows before it waits for the first of them; a row whose edge lies in those
// LED_PROBE * 64 pixels -- every row of a real capture -- costs no wait of its own.  Only a row without an early
// edge walks on, LED_WALK chunks per wait.  
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ntscsim.h"
#include "led_run.hpp"
#include "ntsc_frames.hpp"
#include "ntsc_px4.hpp"
#include "ntsc_stage.hpp"

namespace ntscsim {

#define LDEV __device__ __forceinline__

constexpr int LED_THREADS = 256;
constexpr int LED_WAVES = LED_THREADS / 64;
constexpr int LED_BAND = 16;             // rows a workgroup shifts
constexpr int LED_HALO = 4;              // rows above and below that the mean :903-906 reads
constexpr int LED_SCANS = LED_BAND + 2 * LED_HALO;
constexpr int LED_ROWS_PER_WAVE = LED_SCANS / LED_WAVES;
constexpr int LED_PROBE = 2;             // chunks of every row requested before the first wait: 128 pixels
constexpr int LED_WALK = 4;              // chunks per wait behind the probe
constexpr int LED_UNROLL = 4;            // quads (pixels) of the copy a lane has in flight
static_assert(LED_SCANS % LED_WAVES == 0, "every wave scans the same number of rows");

struct LedRec {                          // one frame
    uint8_t *dst;
    const uint8_t *src;
    int32_t *edges;                      // ntscsim_led_debug_keep_edges(): e[0 .. H) then x[0 .. H), or NULL
    int32_t dst_ls, src_ls;
    uint32_t vec;                        // dst and dst_ls are multiples of 16
    uint32_t _pad;
};

// e of one row whose probe has come back: p[c] is the lane's pixel of chunk c (anything where the pixel lies behind
// the row's end).  The masks and everything decided on them are wave-uniform.
LDEV int led_row_edge(const uint8_t *row, const uint32_t (&p)[LED_PROBE], int W, int lane)
{
    const uint32_t blue = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[0]) & 0xFFu;     // in[y][0], never shifted :877
    int carry = 0;
#pragma unroll
    for (int c = 0; c < LED_PROBE; c++) {
        const int px = c * LED_CHUNK + lane;
        const uint64_t mask = __ballot(px < W && led_not_blackish(p[c], blue));
        const LedRunStep s = led_run_step(mask, carry);
        if (s.hit >= 0) return c * LED_CHUNK + s.hit - (LED_RUN - 1);
        carry = s.carry;
    }
    for (int base = LED_PROBE * LED_CHUNK; base < W; base += LED_WALK * LED_CHUNK) {
        uint32_t q[LED_WALK];
#pragma unroll
        for (int c = 0; c < LED_WALK; c++) {
            const int px = base + c * LED_CHUNK + lane;
            q[c] = gld(row + 4 * (size_t)(px < W ? px : W - 1));
        }
#pragma unroll
        for (int c = 0; c < LED_WALK; c++) {
            const int px = base + c * LED_CHUNK + lane;
            const uint64_t mask = __ballot(px < W && led_not_blackish(q[c], blue));
            const LedRunStep s = led_run_step(mask, carry);
            if (s.hit >= 0) return base + c * LED_CHUNK + s.hit - (LED_RUN - 1);
            carry = s.carry;
        }
    }
    return W;                            // no run of nine: count ran out :876
}

// out[y][i .. i + 3] for a quad that lies wholly in front of or wholly behind `lim`, the first pixel that stays
LDEV px4_u4 led_quad(const uint8_t *srow, int i, int x, int lim, bool wide)
{
    if (i + 4 <= lim || i >= lim) {
        const uint8_t *p = srow + 4 * (size_t)(i + (i < lim ? x : 0));
        if (wide) return gld4a(p);
        return px4_u4{gld(p), gld(p + 4), gld(p + 8), gld(p + 12)};
    }
    px4_u4 v;                            // the one quad of a row that holds both kinds
    v.x = gld(srow + 4 * (size_t)(i + 0 + (i + 0 < lim ? x : 0)));
    v.y = gld(srow + 4 * (size_t)(i + 1 + (i + 1 < lim ? x : 0)));
    v.z = gld(srow + 4 * (size_t)(i + 2 + (i + 2 < lim ? x : 0)));
    v.w = gld(srow + 4 * (size_t)(i + 3 + (i + 3 < lim ? x : 0)));
    return v;
}

// pixels [first, first + per) of each of the band's rows as dwords, one per lane
LDEV void led_copy_dwords(uint8_t *dst, int dst_ls, const uint8_t *src, int src_ls, const int32_t *s_x, int W, int y0, int rows,
                          int first, int per)
{
    const int total = per * rows;
    for (int base = threadIdx.x; base < total; base += LED_UNROLL * LED_THREADS) {
        uint32_t v[LED_UNROLL];
        uint8_t *dp[LED_UNROLL];
#pragma unroll
        for (int k = 0; k < LED_UNROLL; k++) {
            const int item = base + k * LED_THREADS;
            if (item < total) {
                const int row = item / per, i = first + (item - row * per);
                const int x = s_x[row];                                         // 0 for a row that does not move
                dp[k] = dst + (size_t)(y0 + row) * (size_t)dst_ls + 4 * (size_t)i;
                v[k] = gld(src + (size_t)(y0 + row) * (size_t)src_ls + 4 * (size_t)(i + (i < W - x ? x : 0)));
            }
        }
#pragma unroll
        for (int k = 0; k < LED_UNROLL; k++)
            if (base + k * LED_THREADS < total) gst(dp[k], v[k]);
    }
}

// WIDE: the source quads of the vector path are one 16-byte load from a dword-aligned address; otherwise four dwords
template <bool WIDE>
__global__ __launch_bounds__(LED_THREADS) void k_led_frames(const LedRec *__restrict__ recs, int W, int H)
{
    __shared__ int32_t s_e[LED_SCANS];   // e of rows lo .. hi - 1
    __shared__ int32_t s_x[LED_BAND];    // the shift of rows y0 .. y0 + rows - 1; 0 where the row does not move

    const LedRec &r = recs[blockIdx.y];
    uint8_t *const dst = r.dst;
    const uint8_t *const src = r.src;
    int32_t *const edges = r.edges;
    const int dst_ls = r.dst_ls, src_ls = r.src_ls;
    const bool vec = r.vec != 0;

    const int y0 = (int)blockIdx.x * LED_BAND;
    const int rows = H - y0 < LED_BAND ? H - y0 : LED_BAND;
    const int lo = y0 - LED_HALO < 0 ? 0 : y0 - LED_HALO;
    const int hi = y0 + rows + LED_HALO > H ? H : y0 + rows + LED_HALO;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);

    // ---- scan: rows lo + wave, lo + wave + 4, ...; a row behind hi reads row hi - 1 instead and is not recorded, so
    // that the probe is the same straight line of loads in every wave
    {
        uint32_t p[LED_ROWS_PER_WAVE][LED_PROBE];
        const uint8_t *row[LED_ROWS_PER_WAVE];
#pragma unroll
        for (int j = 0; j < LED_ROWS_PER_WAVE; j++) {
            const int y = lo + wave + j * LED_WAVES;
            row[j] = src + (size_t)(y < hi ? y : hi - 1) * (size_t)src_ls;
        }
#pragma unroll
        for (int c = 0; c < LED_PROBE; c++)
#pragma unroll
            for (int j = 0; j < LED_ROWS_PER_WAVE; j++) {
                const int px = c * LED_CHUNK + lane;
                p[j][c] = gld(row[j] + 4 * (size_t)(px < W ? px : W - 1));
            }
#pragma unroll
        for (int j = 0; j < LED_ROWS_PER_WAVE; j++) {
            const int y = lo + wave + j * LED_WAVES;
            const int e = led_row_edge(row[j], p[j], W, lane);
            if (y < hi && lane == 0) s_e[y - lo] = e;
        }
    }
    __syncthreads();

    // ---- smoothing :900-906 and the shift :913-921, one lane per row of the band
    if ((int)threadIdx.x < rows) {
        const int y = y0 + (int)threadIdx.x;
        int32_t adj2 = s_e[y - lo] << 16;
        if (y >= LED_HALO && y < H - LED_HALO) {
            int32_t a[9];
#pragma unroll
            for (int i = 0; i < 9; i++) a[i] = s_e[y - LED_HALO + i - lo] << 16;
            adj2 = led_smooth(a);
        }
        const int32_t x = led_shift_of(adj2);
        s_x[threadIdx.x] = led_row_moves(x, W) ? x : 0;
        if (edges) {
            edges[y] = s_e[y - lo];
            edges[H + y] = x;
        }
    }
    __syncthreads();

    // ---- copy: out[y][i] = in[y][i + x] for i < W - x, in[y][i] behind that
    if (vec) {
        const int Q = W >> 2, total = Q * rows;
        for (int base = threadIdx.x; base < total; base += LED_UNROLL * LED_THREADS) {
            px4_u4 v[LED_UNROLL];
            uint8_t *dp[LED_UNROLL];
#pragma unroll
            for (int k = 0; k < LED_UNROLL; k++) {
                const int item = base + k * LED_THREADS;
                if (item < total) {
                    const int row = item / Q, i = (item - row * Q) << 2;
                    const int x = s_x[row];
                    dp[k] = dst + (size_t)(y0 + row) * (size_t)dst_ls + 4 * (size_t)i;
                    v[k] = led_quad(src + (size_t)(y0 + row) * (size_t)src_ls, i, x, W - x, WIDE);
                }
            }
#pragma unroll
            for (int k = 0; k < LED_UNROLL; k++)
                if (base + k * LED_THREADS < total) gst4(dp[k], v[k]);
        }
        if (W & 3) led_copy_dwords(dst, dst_ls, src, src_ls, s_x, W, y0, rows, W & ~3, W & 3);
    } else
        led_copy_dwords(dst, dst_ls, src, src_ls, s_x, W, y0, rows, 0, W);
}

// ---- host side -----------------------------------------------------------------------------------------------

struct LedState {
    ntscsim_led_params prm;
    RecordSlots<> slots;
    FrameArena frames;                   // ntscsim_led_frames_host()
    bool keep = false;                   // ntscsim_led_debug_keep_edges()
    int32_t *edges = nullptr;            // 2 * height words per frame of the last call
    size_t edges_cap = 0;                // in frames
    int edges_frames = 0, edges_h = 0;   // what the last call left there
    bool src_dwords = false;             // NTSCSIM_LED_SRC_DWORDS=1: developer A/B switch, k_led_frames<false>
};

void led_state_destroy(LedState *k)
{
    if (!k) return;
    if (k->edges) (void)hipFree(k->edges);
    k->slots.release();
    k->frames.release();
    delete k;
}

} // namespace ntscsim

using namespace ntscsim;

namespace {

bool led_size_ok(int w, int h) { return w >= LED_MIN_SIZE && w <= LED_MAX_WIDTH && h >= LED_MIN_SIZE && h <= LED_MAX_HEIGHT; }

// aligned: a device call; a host frame may lie anywhere and have any linesize that holds a row
int led_check_desc(const LedState *k, const ntscsim_led_desc &d, bool aligned)
{
    const int W = k->prm.width, H = k->prm.height;
    if (!d.dst_dev || !d.src_dev) return NTSCSIM_E_ARG;
    if (d.width != W || d.height != H) return NTSCSIM_E_SIZE;
    if (plane_check(d.dst_dev, d.dst_linesize, W, aligned)) return NTSCSIM_E_SIZE;
    if (plane_check(d.src_dev, d.src_linesize, W, aligned)) return NTSCSIM_E_SIZE;
    if (overlaps(span_of(d.dst_dev, d.dst_linesize, H), span_of(d.src_dev, d.src_linesize, H))) return NTSCSIM_E_ARG;
    return NTSCSIM_OK;
}

// what descriptor i touches, for frames_in_order()
Span led_touch(const ntscsim_led_desc &d, int H, std::vector<Span> &rd)
{
    rd.push_back(span_of(d.src_dev, d.src_linesize, H));
    return span_of(d.dst_dev, d.dst_linesize, H);
}

// one launch over descriptors that do not depend on each other; frame0: index of descs[0] in the call
int led_launch(ntscsim_ctx *c, const ntscsim_led_desc *descs, int m, int frame0, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    LedState *k = *v.led;
    const int W = k->prm.width, H = k->prm.height;
    RecordSlot *slot = nullptr;
    const int rc = k->slots.acquire(v, (size_t)m * sizeof(LedRec), slot);
    if (rc != NTSCSIM_OK) return rc;
    RecordSlot &s = *slot;
    LedRec *recs = reinterpret_cast<LedRec *>(s.host);
    for (int i = 0; i < m; i++) {
        const ntscsim_led_desc &d = descs[i];
        LedRec &r = recs[i];
        std::memset(&r, 0, sizeof(r));
        r.dst = static_cast<uint8_t *>(d.dst_dev);
        r.src = static_cast<const uint8_t *>(d.src_dev);
        r.dst_ls = d.dst_linesize;
        r.src_ls = d.src_linesize;
        r.vec = (((uintptr_t)d.dst_dev | (uintptr_t)d.dst_linesize) & 15) == 0;
        r.edges = k->keep ? k->edges + (size_t)(frame0 + i) * 2 * (size_t)H : nullptr;
    }
    STAGECHK(v, hipMemcpyAsync(s.dev, s.host, (size_t)m * sizeof(LedRec), hipMemcpyHostToDevice, st));
    const LedRec *recs_dev = reinterpret_cast<const LedRec *>(s.dev);
    const dim3 grid((unsigned)((H + LED_BAND - 1) / LED_BAND), (unsigned)m), block(LED_THREADS);
    if (k->src_dwords) hipLaunchKernelGGL(k_led_frames<false>, grid, block, 0, st, recs_dev, W, H);
    else hipLaunchKernelGGL(k_led_frames<true>, grid, block, 0, st, recs_dev, W, H);
    return stage_launched(v, &s, st, k->src_dwords ? "k_led_frames<dwords>" : "k_led_frames");
}

// every descriptor checked, then launches of at most 65535 descriptors, cut where descriptors depend on each other:
// they take effect in order (frames_in_order())
int led_frames(ntscsim_ctx *c, const ntscsim_led_desc *descs, int n, hipStream_t st)
{
    CtxStageView v = ctx_stage_view(c);
    LedState *k = *v.led;
    const int H = k->prm.height;
    for (int i = 0; i < n; i++) {
        const int rc = led_check_desc(k, descs[i], true);
        if (rc != NTSCSIM_OK) return rc;
    }
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    k->edges_frames = 0;
    if (n == 0) return NTSCSIM_OK;
    if (k->keep) {
        if ((size_t)n > k->edges_cap || k->edges_h != H) {
            const int rc = k->slots.wait_all(v);                                // launches in flight write the old plane
            if (rc != NTSCSIM_OK) return rc;
            if (k->edges) { (void)hipFree(k->edges); k->edges = nullptr; k->edges_cap = 0; }
            STAGECHK(v, hipMalloc((void **)&k->edges, (size_t)n * 2 * (size_t)H * sizeof(int32_t)));
            k->edges_cap = (size_t)n;
        }
        k->edges_h = H;
    }
    const int rc = frames_in_order(n, 65535, [&](int i, std::vector<Span> &rd) { return led_touch(descs[i], H, rd); },
                                   [&](int first, int m) { return led_launch(c, descs + first, m, first, st); });
    if (rc != NTSCSIM_OK) return rc;
    if (k->keep) k->edges_frames = n;
    return NTSCSIM_OK;
}

} // namespace

extern "C" int ntscsim_led_bind(ntscsim_ctx *c, const ntscsim_led_params *p)
{
    if (!c || !p || p->struct_size != sizeof(*p)) return NTSCSIM_E_ARG;
    if (!led_size_ok(p->width, p->height)) return NTSCSIM_E_SIZE;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    LedState *k = *v.led;
    if (!k) {
        k = new (std::nothrow) LedState();
        if (!k) return NTSCSIM_E_NOMEM;
        const char *ev = std::getenv("NTSCSIM_LED_SRC_DWORDS");
        k->src_dwords = ev && ev[0] == '1';
        *v.led = k;
    }
    const int rc = k->slots.wait_all(v);                                        // launches in flight use the edges plane
    if (rc != NTSCSIM_OK) return rc;
    k->prm = *p;
    k->prm.input_path = nullptr;
    k->prm.output_path = nullptr;
    k->edges_frames = 0;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_led_frames_device(ntscsim_ctx *c, const ntscsim_led_desc *descs, int n, void *hip_stream)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    if (!*v.led) return NTSCSIM_E_ARG;                                          // ntscsim_led_bind() first
    return led_frames(c, descs, n, hip_stream ? static_cast<hipStream_t>(hip_stream) : v.stream);
}

extern "C" int ntscsim_led_frames_host(ntscsim_ctx *c, const ntscsim_led_desc *descs, int n)
{
    if (!c || n < 0 || (n > 0 && !descs)) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    LedState *k = *v.led;
    if (!k) return NTSCSIM_E_ARG;
    const int W = k->prm.width, H = k->prm.height;
    for (int i = 0; i < n; i++) {
        const int rc = led_check_desc(k, descs[i], false);
        if (rc != NTSCSIM_OK) return rc;
    }
    STAGECHK(v, hipSetDevice(v.device));
    v.kernels->clear();
    // Batches of frames through the arena: source | destination per frame, rows packed to a 16-byte pitch.  Only the
    // 4 * width bytes of a row travel either way, so what the device call leaves alone keeps what the host frame held.
    // A batch ends in front of a descriptor that touches a frame an earlier one of the batch wrote, or writes one it
    // read: descriptors take effect in order, through host memory.
    hipStream_t st = v.stream;
    const size_t row = (size_t)W * 4, pitch = (row + 15) & ~(size_t)15, fbytes = pitch * (size_t)H;
    const int cap = (int)std::max<size_t>(1, std::min<size_t>(65535, ((size_t)256 << 20) / (2 * fbytes)));
    std::string kernels;
    std::vector<ntscsim_led_desc> dev;
    const auto touch = [&](int i, std::vector<Span> &rd) { return led_touch(descs[i], H, rd); };
    const int rc = frames_in_order(n, cap, touch, [&](int first, int m) -> int {
        const int arc = k->frames.reserve(v, 2 * fbytes * (size_t)m, fbytes * (size_t)m);
        if (arc != NTSCSIM_OK) return arc;
        unsigned char *stage = k->frames.staging, *arena = k->frames.arena;
        dev.assign(descs + first, descs + first + m);
        for (int i = 0; i < m; i++) {
            ntscsim_led_desc &d = dev[(size_t)i];
            copy_rows(stage + (size_t)i * fbytes, pitch, d.src_dev, (size_t)d.src_linesize, row, H);
            d.src_dev = arena + (size_t)i * fbytes;
            d.dst_dev = arena + (size_t)(m + i) * fbytes;
            d.src_linesize = d.dst_linesize = (int)pitch;
        }
        STAGECHK(v, hipMemcpyAsync(arena, stage, fbytes * (size_t)m, hipMemcpyHostToDevice, st));
        const int frc = led_frames(c, dev.data(), m, st);
        if (frc != NTSCSIM_OK) return frc;
        if (!kernels.empty()) kernels += ';';
        kernels += *v.kernels;
        STAGECHK(v, hipMemcpyAsync(stage, arena + (size_t)m * fbytes, fbytes * (size_t)m, hipMemcpyDeviceToHost, st));
        STAGECHK(v, hipStreamSynchronize(st));
        for (int i = 0; i < m; i++)
            copy_rows(descs[first + i].dst_dev, (size_t)descs[first + i].dst_linesize, stage + (size_t)i * fbytes, pitch, row, H);
        return NTSCSIM_OK;
    });
    if (rc != NTSCSIM_OK) return rc;
    *v.kernels = kernels;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_led_debug_keep_edges(ntscsim_ctx *c, int on)
{
    LedState *k = c ? *ctx_stage_view(c).led : nullptr;
    if (!k) return NTSCSIM_E_ARG;
    k->keep = on != 0;
    if (!k->keep) k->edges_frames = 0;
    return NTSCSIM_OK;
}

extern "C" int ntscsim_led_debug_edges(ntscsim_ctx *c, int frame, int32_t *e_host, int32_t *x_host)
{
    LedState *k = c ? *ctx_stage_view(c).led : nullptr;
    if (!k || !k->edges || frame < 0 || frame >= k->edges_frames) return NTSCSIM_E_ARG;
    CtxStageView v = ctx_stage_view(c);
    STAGECHK(v, hipSetDevice(v.device));
    STAGECHK(v, hipDeviceSynchronize());
    const size_t H = (size_t)k->edges_h;
    const int32_t *at = k->edges + (size_t)frame * 2 * H;
    if (e_host) STAGECHK(v, hipMemcpy(e_host, at, H * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (x_host) STAGECHK(v, hipMemcpy(x_host, at + H, H * sizeof(int32_t), hipMemcpyDeviceToHost));
    return NTSCSIM_OK;
}
